"""The shared-dictionary calls without a GPU: the model (tests/dict_model.py: LZ4_loadDict restated over the oracle's compress
stream) against the golden the reference wrote and against the reference itself, that the grid can see the loader's one ordering
rule, and the surface -- symbols, header, bindings, Haskell imports, the argument checks that need no device."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dict_cases as DC  # noqa: E402
import dict_model as M  # noqa: E402

E_ARG = -3
SYMBOLS = ["mi355lz4_cstreams_load_dict", "mi355lz4_compress_dict_device", "mi355lz4_decompress_dict_device",
           "mi355lz4_compress_dict", "mi355lz4_decompress_dict"]


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "dict_vectors.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def loaded():
    return {dl: M.model_load(DC.dictionary(dl)) for dl in DC.DICT_LENS}


def test_grid_is_the_golden_grid(vectors):
    keys = {DC.compress_key(dl, bl, a) for dl in DC.DICT_LENS for bl in DC.BLOCK_LENS for a in DC.ACCELS}
    assert set(vectors["compress"]) == keys and len(keys) == 260
    assert set(vectors["stream"]) == {str(dl) for dl in DC.DICT_LENS}
    assert [(n, d) for n, d, _, _ in vectors["decode"]] == [(n, d) for n, d, _, _ in DC.decode_cases()]


def test_model_compress_equals_golden(vectors, loaded):
    for dl in DC.DICT_LENS:
        for bl in DC.BLOCK_LENS:
            for a in DC.ACCELS:
                code, comp = M.model_compress(loaded[dl], DC.block(bl), a)
                assert [code, sha(comp)] == vectors["compress"][DC.compress_key(dl, bl, a)], (dl, bl, a)


def test_model_stream_equals_golden(vectors, loaded):
    for dl in DC.DICT_LENS:
        got = [[c, sha(b)] for c, b in M.model_stream(loaded[dl], DC.stream_blocks(), DC.STREAM_ACCEL)]
        assert got == vectors["stream"][str(dl)], dl


def test_short_dictionary_still_moves_the_offset(vectors, loaded):
    """LZ4_loadDict of fewer than 8 bytes leaves no dictionary and an empty table, but currentOffset = 65536 all the same (the
    blocks that follow take the dictSmall path; their bytes are in the golden like every other case's)"""
    for dl in (0, 3, 7):
        assert loaded[dl].s.currentOffset == 65536 and loaded[dl].s.dictSize == 0 and not any(loaded[dl].s.table)
    assert loaded[8].s.dictSize == 8 and sum(1 for v in loaded[8].s.table if v) == 1
    assert loaded[11].s.dictSize == 11 and sum(1 for v in loaded[11].s.table if v) == 2
    assert loaded[200000].s.dictSize == 65536


def test_first_writer_wins_changes_a_golden_case(vectors):
    """the loader's one ordering rule: with the FIRST writer of a bucket kept, some case of the grid gives other bytes"""
    changed = 0
    for dl in DC.DICT_LENS:
        if dl < 8:
            continue
        wrong = M.model_load(DC.dictionary(dl), first_writer_wins=True)
        for bl in DC.BLOCK_LENS:
            code, comp = M.model_compress(wrong, DC.block(bl), 1)
            changed += [code, sha(comp)] != vectors["compress"][DC.compress_key(dl, bl, 1)]
    assert changed > 0, "the grid cannot see which writer of a bucket LZ4_loadDict keeps"


def test_model_decode_equals_golden(vectors, oracle):
    for (name, dl, blk, cap), (_, _, code, digest) in zip(DC.decode_cases(), vectors["decode"]):
        got, out = oracle.decompress_block(blk, cap, DC.dictionary(dl))
        assert (got, sha(out)) == (code, digest), (name, dl)


def test_decode_cases_hit_their_edges(vectors):
    """the hand-built blocks do what their names say under the reference: the edges decode, the errors fail"""
    by = {(n, d): c for n, d, c, _ in vectors["decode"]}
    cases = {(n, d): (b, c) for n, d, b, c in DC.decode_cases()}
    for d in DC.DECODE_DICT_LENS:
        for n in ("offset onto the first reachable byte of the dictionary", "match from the dictionary into the block's own output",
                  "match inside the dictionary's last 4 bytes", "offset 0"):
            assert by[(n, d)] == cases[(n, d)][1], (n, d)
        for n in ("capacity one byte short", "truncated inside an offset field", "truncated inside an offset field, deep"):
            assert by[(n, d)] < 0, (n, d)
    assert by[("offset one byte in front of the dictionary", 100)] < 0
    assert by[("offset 65535", 70000)] > 0 and by[("offset 65535 deep in the block", 70000)] > 0


def test_golden_blocks_decode_with_their_dictionary(loaded, oracle):
    """the model's blocks decode to their sources with the dictionary"""
    for dl in (8, 100, 65536, 200000):
        for bl in (13, 1000, 100000):
            code, comp = M.model_compress(loaded[dl], DC.block(bl), 1)
            assert oracle.decompress_block(comp, bl, DC.dictionary(dl)) == (bl, DC.block(bl))


def test_model_equals_reference(reference):
    """the model against the real LZ4_loadDict + LZ4_compress_fast_continue, directly (where oracle/_ref exists)"""
    L = reference.lib
    vp = C.c_void_p
    for name, res, args in (("LZ4_initStream", vp, [vp, C.c_size_t]), ("LZ4_loadDict", C.c_int, [vp, vp, C.c_int]),
                            ("LZ4_compress_fast_continue", C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    for dl in (0, 7, 8, 11, 4095, 65537, 200000):
        d = C.create_string_buffer(DC.dictionary(dl) + bytes(64), dl + 64)
        for bl in (12, 13, 1000, 65536):
            for accel in DC.ACCELS:
                s = (C.c_uint64 * 2052)()
                assert L.LZ4_initStream(C.addressof(s), 16416)
                L.LZ4_loadDict(C.addressof(s), C.addressof(d), dl)
                data = DC.block(bl)
                src = C.create_string_buffer(data + bytes(64), bl + 64)
                cap = M.compress_bound(bl)
                dst = C.create_string_buffer(cap + 64)
                r = L.LZ4_compress_fast_continue(C.addressof(s), C.addressof(src), C.addressof(dst), bl, cap, accel)
                assert (r, dst.raw[:max(r, 0)]) == M.model_compress(DC.dictionary(dl), data, accel), (dl, bl, accel)


def test_symbols_declared_listed_and_exported(slz4):
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in include/mi355lz4.h"
        assert name in slz4.DECLARED_SYMBOLS, name
        assert getattr(slz4.lib, name).argtypes is not None, name + " has no sig() declaration"
    for m in ("compress_dict_device", "compress_dict", "decompress_dict_device", "decompress_dict"):
        assert hasattr(slz4.Engine, m)
    assert hasattr(slz4.CompressStreams, "load_dict")
    hpp = open(os.path.join(ROOT, "include", "streamly_lz4.hpp")).read()
    for m in ("loadDict", "compressWithDict", "decompressWithDict"):
        assert re.search(r"\b%s\s*\(" % m, hpp), m + " is not declared in include/streamly_lz4.hpp"


def test_header_states_the_contract():
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    top = header.split("engine lifecycle")[0]
    for name in ("_cstreams_load_dict", "_compress_dict_device", "_decompress_dict_device"):
        assert name in top, name + " is missing from the 'what a call may write' block"
    assert "mi355lz4_set_decoder is ignored by this call" in header
    assert "prefix mode the reference takes when a destination happens to lie directly behind the dictionary is not" in header
    assert "profiles/dict_rate.json" in header and os.path.exists(os.path.join(ROOT, "profiles", "dict_rate.json"))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7i" in design and "dictCtx" in design and "saveDict" in design


def test_null_and_argument_checks_need_no_device(slz4):
    L = slz4.lib
    sz, nb = C.c_size_t(7), C.c_int(7)
    assert L.mi355lz4_cstreams_load_dict(None, None, 0, None, 0) == E_ARG
    assert b"cstreams_load_dict" in L.mi355lz4_last_error()
    assert L.mi355lz4_compress_dict_device(None, None, 0, None, None, None, 0, 0, 0, 1, 8, None, 0, None) == E_ARG
    assert b"compress_dict_device" in L.mi355lz4_last_error()
    assert L.mi355lz4_decompress_dict_device(None, None, 0, None, 0, 8, 0, None, 0, None, None, None, None) == E_ARG
    assert L.mi355lz4_compress_dict(None, None, 0, None, None, 0, 1, 8, None, 0, C.byref(sz), None, None) == E_ARG
    assert sz.value == 0 and b"compress_dict" in L.mi355lz4_last_error()
    assert L.mi355lz4_decompress_dict(None, None, 0, 8, 0, None, 0, None, 0, C.byref(sz), None, 0, C.byref(nb)) == E_ARG


def test_haskell_shim_imports_match_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_haskell_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    shim = open(os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")).read()
    for name in SYMBOLS:
        assert '"mi355lz4.h %s"' % name in shim, name + " is not imported by the Haskell shim"
    assert "compressChunksWithDict" in shim and "decompressChunksWithDict" in shim


def test_argument_checks_under_sanitizers():
    """the host code of the five calls from a program of its own (tests/native/dict_args_main.cpp), ASan + UBSan, no device"""
    if shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("g++ or the HIP host headers are not available")
    r = subprocess.run(["make", "-C", ROOT, "asan-dict"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "dict_args_main ok" in r.stdout
    for bad in ("ERROR: AddressSanitizer", "runtime error:"):
        assert bad not in r.stdout + r.stderr
