"""Partial decode, the part that needs no GPU: the fixture (tests/golden/partial_vectors.json) is well formed and, where the
reference is built, equals a live call of LZ4_decompress_safe_partial; the law the GPU test expects of well-formed blocks --
result = min(target, cap, n), bytes = the prefix -- holds on the reference for the targets that test uses; the header, the
Python binding and the Haskell shim declare the two new calls."""
import os
import random
import subprocess
import sys

import pytest

import partial_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3


@pytest.fixture(scope="module")
def raw():
    return P.load_raw()


@pytest.fixture(scope="module")
def cases(raw):
    return P.expand(raw)


@pytest.fixture(scope="module")
def ref_lib(reference):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_partial_golden as MG
    return MG, MG.load_reference()


def test_fixture_is_well_formed(raw, cases):
    assert os.path.getsize(P.PATH) < 512 * 1024
    assert [b["n"] for b in raw["bases"]] == [64, 300, 1500, 4096]
    for b in raw["bases"]:
        assert len(bytes.fromhex(b["data"])) == b["n"] and len(bytes.fromhex(b["block"])) > 0
    assert 550 <= len(cases) <= 650
    neg = sum(c.result < 0 for c in cases)
    assert neg >= 100 and len(cases) - neg >= 300
    for c, r in zip(cases, raw["cases"]):
        n = raw["bases"][c.base]["n"]
        assert 1 <= len(c.mutations) <= 3 and 0 <= c.target <= n + 40 and c.cap in (c.target, n, n + 64)
        assert c.block != bytes.fromhex(raw["bases"][c.base]["block"])          # every case is a mutated block
        assert c.result <= min(c.target, c.cap) and len(c.prefix) == max(c.result, 0)
        assert set(r) == {"base", "mut", "target", "cap", "result", "diff"}      # data only


def test_kernel_rules_model_equals_the_fixture(cases):
    """tests/partial_model.py restates decode_seq.hpp's partial mode; it gives the reference's result and bytes for every case"""
    import partial_model
    for i, c in enumerate(cases):
        r, pre = partial_model.model(c.block, c.target, c.cap, 0xEE)
        assert (r, pre if r >= 0 else b"") == (c.result, c.prefix), i


def test_fixture_equals_the_reference(cases, ref_lib):
    MG, L = ref_lib
    for i, c in enumerate(cases):
        for fill in (0x00, 0xEE):
            assert MG.ref_partial(L, c.block, c.target, c.cap, fill) == (c.result, c.prefix), i


def test_law_of_well_formed_blocks_on_the_reference(ref_lib, oracle):
    """result = min(target, cap, n) and the prefix, for the hand-built blocks and for compressor output, with the GPU test's targets"""
    MG, L = ref_lib
    rng = random.Random(11)
    blocks = P.hand_built_blocks()
    assert len(blocks) > 100
    for n in (0, 1, 12, 13, 1024, 65536):
        for kind in ("text", "lzsynth", "random"):
            data = oracle.gen(kind, 1, max(n, 1))[:n].tobytes()
            blocks.append(("%s %d" % (kind, n), oracle.compress_block(data), data))
        blocks.append(("run %d" % n, oracle.compress_block(b"r" * n), b"r" * n))
    checked = 0
    for name, block, data in blocks:
        n = len(data)
        ts = P.targets_for(n, P.boundaries_of(block), rng, 8 if n > 4096 else 32)
        if n > 4096:
            ts = ts[::3]                                # (the big blocks: every third target keeps this test quick)
        for k, t in enumerate(ts):
            cap = P.caps_for(t, n, k)
            want = min(t, cap, n)
            assert MG.ref_partial(L, block, t, cap, 0xEE) == (want, data[:want]), (name, t, cap)
            checked += 1
    assert checked > 10000


def test_symbols_declared():
    import streamly_lz4_amd as S
    hdr = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    for name in ("mi355lz4_decompress_partial_device", "mi355lz4_decompress_partial"):
        assert name in S.DECLARED_SYMBOLS and getattr(S.lib, name)
        assert "int %s(" % name in hdr
    assert S.lib.mi355lz4_decompress_partial_device.argtypes is not None and len(S.lib.mi355lz4_decompress_partial_device.argtypes) == 12
    assert len(S.lib.mi355lz4_decompress_partial.argtypes) == 13
    assert hasattr(S.Engine, "decompress_partial_device") and hasattr(S.Engine, "decompress_partial")
    hpp = open(os.path.join(ROOT, "include", "streamly_lz4.hpp")).read()
    assert "std::vector<Array> decompressPartial(const BlockConfig &cfg, const Array &framed, int target, int fixedUncomp = 0);" in hpp
    legacy = open(os.path.join(ROOT, "include", "lz4.h")).read()
    assert "partial" not in legacy                      # the legacy face stays at its seven symbols


def test_bad_arguments_need_no_device():
    import streamly_lz4_amd as S
    f = S.lib.mi355lz4_decompress_partial_device
    assert f(None, None, 0, None, 0, 8, 0, None, None, None, None, None) == E_ARG          # null ctx
    g = S.lib.mi355lz4_decompress_partial
    assert g(None, None, 0, 8, 0, None, 0, None, 0, None, None, 0, None) == E_ARG
    assert b"null ctx" in S.lib.mi355lz4_last_error()


def test_shim_passes_the_ffi_check():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_haskell_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mi355lz4_decompress_partial_device" in r.stdout and "mi355lz4_decompress_partial," in r.stdout + ","
    shim = open(os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")).read()
    assert "decompressChunksPrefix ::" in shim
