"""Fast fixed-size output pages without a GPU (mi355lz4_compress_pages_fast_device, mi355lz4_compress_pages_fast): the contract as a
model (tests/fastpages_model.py) held to its own claims on the whole grid -- E from the CPU oracle and from hand-built blocks --,
the surface -- symbols, header, bindings, the C++ and Haskell mirrors -- and the argument checks that need no device, from Python
and from a program of its own under ASan + UBSan."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fastpages_model as FM  # noqa: E402
import lz4_check  # noqa: E402
import pages_cases as PC  # noqa: E402

E_ARG = -3
SYMBOLS = ["mi355lz4_compress_pages_fast_device", "mi355lz4_compress_pages_fast"]
GRID_T = range(0, 601)


def check_page(oracle, src, e, t):
    """every claim of the contract on the page of size t for the slice src with block e; returns (page, used, j)"""
    n = len(src)
    pg, used, j = FM.page(e, src, t)
    if t < 1:
        assert pg is None and used == 0
        return pg, used, j
    where = "T %d, n %d, |E| %d" % (t, n, len(e))
    assert len(pg) <= t, where
    lz4_check.check_block(pg, used)
    code, back = oracle.decompress_block(pg, used)
    assert code == used and back == src[:used], where
    cuts = FM.valid_cuts(e, n, t)
    assert cuts == sorted(cuts, reverse=True), where + ": a valid cut behind an invalid one"
    if len(e) <= t:
        assert pg == e and used == n and j is None, where
        assert all(cuts), where + ": a block that fits has a sequence without a valid cut"
        return pg, used, j
    assert j == sum(cuts) - 1, where
    assert used < n, where
    assert len(pg) >= t - 1, where + ": a page cut by T is full"
    assert used >= FM.min_progress(t), where + ": the progress bound"
    if t == 1:
        assert pg == b"\x00" and used == 0
    return pg, used, j


@pytest.fixture(scope="module")
def grid(oracle):
    """the model's chains over the five 2048-byte inputs at every T in 0..600, every page checked: {(name, T): chain}.  The
    oracle's block of a slice is computed once per (input, position)."""
    blocks = {}
    out = {}
    for name in PC.GRID_SMALL:
        src = PC.input_bytes(name)

        def encode(piece, pos, name=name):
            key = (name, pos)
            if key not in blocks:
                blocks[key] = oracle.compress_block(piece)
                lz4_check.check_block(blocks[key], len(piece))
            return blocks[key]

        for t in GRID_T:
            ch = FM.chain(src, t, encode)
            for pg, used, j, pos, n, cut in ch:
                got = check_page(oracle, src[pos: pos + n], encode(src[pos: pos + n], pos), t)
                assert got == (pg, used, j)
            out[(name, t)] = ch
    return out


def test_lit_closed_form_is_the_definition():
    for s in range(0, 70000):
        assert FM.lit_closed_form(s) == FM.lit(s), s
    assert all(FM.lit_closed_form(s) < 0 and FM.lit(s) < 0 for s in range(-300, 1))      # no room for a token
    assert [FM.lit(s) for s in (0, 1, 2, 15, 16, 17, 271, 272, 273)] == [-1, 0, 1, 14, 14, 15, 269, 269, 270]
    for t in range(1, 70000):
        assert FM.lit(t) == FM.min_progress(t), t     # the all-literals page is 7k's progress bound


def test_chains_consume_the_input_and_concatenate(grid):
    for name in PC.GRID_SMALL:
        src = PC.input_bytes(name)
        assert grid[(name, 0)] == []                                      # T < 1: no page
        assert [(p, u) for p, u, *_ in grid[(name, 1)]] == [(b"\x00", 0)]  # T = 1: a zero token, the chain ends
        for t in range(2, 601):
            ch = grid[(name, t)]
            assert sum(u for _, u, *_ in ch) == len(src), (name, t)
            assert [pos for _, _, _, pos, _, _ in ch] == list(np.cumsum([0] + [u for _, u, *_ in ch[:-1]])), (name, t)
            assert len(ch) <= -(-len(src) // FM.min_progress(t)), (name, t)


def test_the_grid_meets_every_kind_of_cut(grid):
    cuts = [(j, len(p)) for ch in grid.values() for p, _, j, _, _, cut in ch if cut]
    whole = [1 for ch in grid.values() for *_, cut in ch if not cut]
    js = {j for j, _ in cuts}
    assert -1 in js and 0 in js and max(js) >= 8 and whole
    assert {name for (name, t), ch in grid.items() if any(j == -1 and cut for _, _, j, _, _, cut in ch)} >= {"random2048"}


def build_block(seqs, tail, rng):
    """a block from [(literals, match length, offset)] and `tail` last literals, and what it decodes to"""
    out, src = bytearray(), bytearray()
    for ll, ml, off in seqs:
        lits = rng.randint(0, 256, size=ll).astype(np.uint8).tobytes()
        tok = (min(ll, 15) << 4) | min(ml - 4, 15)
        out.append(tok)
        if ll >= 15:
            out += b"\xff" * ((ll - 15) // 255) + bytes([(ll - 15) % 255])
        out += lits
        src += lits
        out += bytes([off & 255, off >> 8])
        if ml - 4 >= 15:
            out += b"\xff" * ((ml - 19) // 255) + bytes([(ml - 19) % 255])
        for _ in range(ml):
            src.append(src[-off])
    lits = rng.randint(0, 256, size=tail).astype(np.uint8).tobytes()
    out += FM.literal_run(lits)
    src += lits
    return bytes(out), bytes(src)


HAND = [(40, 20, 40), (300, 4, 7), (9, 6, 100), (33, 5, 350), (2, 40, 1), (700, 4, 3), (0, 4, 8), (20, 300, 21)]


def test_hand_built_block_falls_back_and_cuts_inside_long_runs(oracle):
    e, src = build_block(HAND, 30, np.random.RandomState(77))
    n = len(src)
    lz4_check.check_block(e, n)
    assert oracle.decompress_block(e, n) == (n, src)
    seqs, _ = FM.sequences(e, n)
    assert len(seqs) == len(HAND)
    fell_r = fell_12 = run32 = run270 = False
    for t in range(0, len(e) + 6):
        pg, used, j = check_page(oracle, src, e, t)
        if t < 1 or len(e) <= t:
            continue
        fits = [k for k, s in enumerate(seqs) if s[2] + 1 <= t]       # sequences that leave room for a token
        if fits and j < fits[-1]:
            ms, ie, oe = seqs[fits[-1]]
            r = min(n - ie, FM.lit(t - oe))
            fell_r |= r < 5
            fell_12 |= r >= 5 and ms + 12 > ie + r
        in_end = seqs[j][1] if j >= 0 else 0
        run = used - in_end
        nxt = seqs[j + 1][0] - in_end if j + 1 < len(seqs) else n - in_end     # the literal run of E that the page's end cuts into
        run32 |= 32 < run < nxt
        run270 |= 270 < run < nxt
    assert fell_r, "no page size left fewer than 5 literals behind the last sequence that fits"
    assert fell_12, "no page size put a match's start within 12 bytes of the page's end"
    assert run32 and run270, "no cut inside a literal run of over 32 / over 270 bytes"
    # the whole block at its own size, one byte less cuts it
    assert FM.page(e, src, len(e)) == (e, n, None)
    assert FM.page(e, src, len(e) - 1)[1] < n


def test_symbols_declared_listed_and_exported(slz4):
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in include/mi355lz4.h"
        assert name in slz4.DECLARED_SYMBOLS, name
        assert getattr(slz4.lib, name).argtypes is not None, name + " has no sig() declaration"
    assert len(slz4.lib.mi355lz4_compress_pages_fast_device.argtypes) == 15      # the exact call's, and accel
    assert len(slz4.lib.mi355lz4_compress_pages_fast.argtypes) == 14
    assert len(slz4.lib.mi355lz4_compress_pages_device.argtypes) == 14
    assert len(slz4.lib.mi355lz4_compress_pages.argtypes) == 13


def test_mirrors_are_present(slz4):
    for m in ("compress_pages_fast_device", "compress_pages_fast"):
        assert hasattr(slz4.Engine, m)
    hpp = open(os.path.join(ROOT, "include", "streamly_lz4.hpp")).read()
    assert re.search(r"\bcompressPagesFast\s*\(", hpp)
    cpp = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "host_stream.cpp")).read()
    assert "Engine::compressPagesFast" in cpp and "mi355lz4_compress_pages_fast(" in cpp
    shim = open(os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")).read()
    for name in SYMBOLS:
        assert '"mi355lz4.h %s"' % name in shim, name + " is not imported by the Haskell shim"
    assert "compressChunksPagedFast" in shim
    kh = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "kernels.h")).read()
    assert "launch_pages_fast" in kh and "PagesFastArgs" in kh


def test_header_states_the_contract():
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    top = header.split("engine lifecycle")[0]
    for name in ("_compress_pages_fast_device", "_compress_pages_fast:"):
        assert name in top, name + " is missing from the 'what a call may write' block"
    for phrase in ("A page never holds more than", "NOT full", "matchStart_j + 12 <= inEnd_j + r_j", "compLen >= T - 1",
                   "(T - 1) - (T + 240) / 256", "profiles/fastpages_rate.json", "The compression level must"):
        assert phrase in header, phrase
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7m" in design and "k_pages_fast" in design
    assert "compress_pages_fast" in open(os.path.join(ROOT, "README.md")).read()
    assert "compress_pages_fast" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fam = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "kernels.hip")).read()
    assert "k_pages_fast" in fam


def test_haskell_shim_imports_match_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_haskell_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    for name in SYMBOLS:
        assert name in r.stdout, name + " was not among the imports that were checked"


def test_null_and_argument_checks_need_no_device(slz4):
    """each returns E_ARG in front of the first HIP call, and mi355lz4_last_error() names the call"""
    L = slz4.lib
    assert L.mi355lz4_compress_pages_fast_device(None, None, None, None, 1, None, 1, 1, 8, None, 64, None, None, None, None) == E_ARG
    assert b"null ctx" in L.mi355lz4_last_error()
    assert L.mi355lz4_compress_pages_fast(None, None, None, 1, 16, 1, 1, 8, None, 64, None, None, None, None) == E_ARG
    assert b"null ctx" in L.mi355lz4_last_error()


def test_sanitizer_builds_list_the_stub():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    for var in ("SAN_SRCS", "DICT_SAN_SRCS", "HCDICT_SAN_SRCS", "PAGES_SAN_SRCS", "FASTDICT_SAN_SRCS", "FASTPAGES_SAN_SRCS"):
        line = [ln for ln in mk.splitlines() if ln.startswith(var + " ")][0]
        assert "tests/native/san_stubs_fastpages.cpp" in line, "%s: the fast page call's launcher would not link" % var
    assert re.search(r"^asan-fastpages:", mk, re.M)
    assert "launch_pages_fast" in open(os.path.join(ROOT, "tests", "native", "san_stubs_fastpages.cpp")).read()


def test_argument_checks_under_sanitizers():
    """the host code of the calls from a program of its own (tests/native/fastpages_args_main.cpp), ASan + UBSan, no device"""
    if shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("g++ or the HIP host headers are not available")
    r = subprocess.run(["make", "-C", ROOT, "asan-fastpages"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "fastpages_args_main ok" in r.stdout
    for bad in ("ERROR: AddressSanitizer", "runtime error:"):
        assert bad not in r.stdout + r.stderr
