"""Fast fixed-size output pages against a prepared dictionary without a GPU (mi355lz4_compress_pages_fastdict_device,
mi355lz4_compress_pages_fastdict): the contract as a model (tests/dictpages_model.py) held to its own claims -- E from the CPU
oracle's dictionary blocks and from hand-built ones --, the surface -- symbols, header, bindings, the C++ and Haskell mirrors -- and
the argument checks that need no device, from Python and from a program of its own under ASan + UBSan."""
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

import dict_cases  # noqa: E402
import dict_model  # noqa: E402
import dictpages_cases as DC  # noqa: E402
import dictpages_model as DM  # noqa: E402
import fastpages_model as FM  # noqa: E402
import lz4_check  # noqa: E402

E_ARG = -3
SYMBOLS = ["mi355lz4_compress_pages_fastdict_device", "mi355lz4_compress_pages_fastdict"]
DICT_LENS = (8, 100, 65536, 70000)
GRID_T = range(1, 701)


def check_page(oracle, dict_bytes, src, e, t):
    """every claim of the contract on the page of size t for the slice src with block e against dict_bytes; (page, used, j)"""
    n = len(src)
    pg, used, j = DM.page(e, src, t)
    where = "T %d, n %d, |E| %d, dictionary %d" % (t, n, len(e), len(dict_bytes))
    assert len(pg) <= t, where
    lz4_check.check_block(pg, used, dict_len=len(dict_bytes))
    code, back = oracle.decompress_block(pg, used, dict_bytes=dict_bytes)
    assert code == used and back == src[:used], where
    if len(e) <= t:
        assert pg == e and used == n and j is None, where
        return pg, used, j
    cuts = []                   # (up to the first sequence that leaves no room for a token: none behind it has a valid cut)
    for s in DM.iter_sequences(e, n):
        cuts.append(DM.cut_is_valid(s, n, t)[0])
        if s[2] + 1 > t:
            break
    assert j == (cuts + [False]).index(False) - 1, where + ": the leading run"
    if used < n:
        assert len(pg) >= t - 1, where + ": a page cut by T is full"
        assert used >= DM.min_progress(t), where + ": the progress bound"
    if t == 1:
        assert pg == b"\x00" and used == 0
    return pg, used, j


@pytest.fixture(scope="module")
def grid(oracle):
    """the model's chains over the 8 KiB input of every dictionary length at every T in 1..700, every page checked:
    {(d, T): chain}; per d the number of pages, of pages that 7m's rule (tests/fastpages_model.py) would make otherwise and of
    pages that open with a match; and the pages at which the leading run and the last valid cut differ.  The oracle's block of a
    slice is computed once per (dictionary, position)."""
    out, stats, differ = {}, {}, []
    for d in DICT_LENS:
        dic = dict_cases.dictionary(d)
        kept = dic[-65536:]
        loaded = dict_model.model_load(dic)
        assert loaded.keep == len(kept)
        src = DC.edge_input(dic)
        blocks = {}

        def encode(piece, pos):
            if pos not in blocks:
                code, e = dict_model.model_compress(loaded, piece)
                assert code == len(e) > 0
                if pos % 64 == 0:       # (E is the oracle's, pinned elsewhere: a sample of the slices shows that the window is right)
                    lz4_check.check_block(e, len(piece), dict_len=len(kept))
                blocks[pos] = e
            return blocks[pos]

        pages = changed = opens_with_match = 0
        for t in GRID_T:
            ch = DM.chain(src, t, encode)
            for pg, used, j, pos, n, cut in ch:
                if t == 1:
                    assert (pg, used) == (b"\x00", 0)
                    continue
                piece = src[pos: pos + n]
                assert check_page(oracle, kept, piece, encode(piece, pos), t) == (pg, used, j)
                pages += 1
                if t <= 16:     # (behind 13 consumed bytes the fourth condition holds, and a page of 17 bytes consumes them)
                    old = FM.page(encode(piece, pos), piece, t)
                    if old[:2] != (pg, used):
                        changed += 1
                        with pytest.raises(lz4_check.BlockRuleError) as err:
                            lz4_check.check_block(old[0], old[1], dict_len=len(kept))
                        assert err.value.rule == lz4_check.SHORT
                    if DM.page_last_valid(encode(piece, pos), piece, t)[:2] != (pg, used):
                        differ.append((d, t, pos, n))
                opens_with_match += cut and pg[0] >> 4 == 0 and used >= 13
            out[(d, t)] = ch
        stats[d] = (pages, changed, opens_with_match)
    return out, stats, differ


def test_chains_consume_the_input_and_concatenate(grid):
    chains, stats, _ = grid
    for d in DICT_LENS:
        n = len(DC.edge_input(dict_cases.dictionary(d)))
        assert n == 8192
        assert [(p, u) for p, u, *_ in chains[(d, 1)]] == [(b"\x00", 0)]          # T = 1: a zero token, the chain ends
        for t in range(2, 701):
            ch = chains[(d, t)]
            assert sum(u for _, u, *_ in ch) == n, (d, t)
            assert [pos for _, _, _, pos, _, _ in ch] == list(np.cumsum([0] + [u for _, u, *_ in ch[:-1]])), (d, t)
        assert stats[d][0] > 40000, stats[d]


def test_the_grid_meets_pages_that_open_with_a_match_and_the_new_rule(grid):
    """a dictionary makes pages whose first sequence has no literals, and at small page sizes 7m's three conditions would make a
    page of fewer than 13 bytes with a match in it (the fixture shows that each of those breaks the "short block" rule)"""
    _, stats, _ = grid
    for d in (65536, 70000):
        pages, changed, opens = stats[d]
        assert opens > 1000, (d, stats[d])
        assert changed > 0, (d, stats[d])
    chains = grid[0]
    assert any(j == -1 and cut for ch in chains.values() for _, _, j, _, _, cut in ch)
    assert any(j is None for ch in chains.values() for _, _, j, _, _, _ in ch)


def test_grid_pages_where_the_rule_and_the_last_valid_cut_differ(oracle, grid):
    """on the oracle's own blocks: the pages of the grid, if any, at which valid cuts are not a prefix (a match of 4 bytes at
    position 0, one of 7 or more directly behind it, T = 12: the hand-built block below is the case that is always there).  The
    leading run's page is the shorter prefix; both are valid blocks -- the rule is about not depending on how the encoder batches
    its sequences"""
    differ = grid[2]
    assert all(t == 12 for _, t, _, _ in differ)
    for d, t, pos, n in differ[:50]:
        dic = dict_cases.dictionary(d)[-65536:]
        src = DC.edge_input(dict_cases.dictionary(d))[pos: pos + n]
        code, e = dict_model.model_compress(dict_cases.dictionary(d), src)
        assert code == len(e) > t
        a, b = DM.page(e, src, t), DM.page_last_valid(e, src, t)
        assert a[2] < b[2], (d, t, pos)
        cuts = DM.valid_cuts(e, n, t)
        assert not cuts[a[2] + 1] and cuts[b[2]] and cuts != sorted(cuts, reverse=True)
        for pg, used, _ in (a, b):
            lz4_check.check_block(pg, used, dict_len=len(dic))
            assert oracle.decompress_block(pg, used, dict_bytes=dic) == (used, src[:used])


def build_block(seqs, tail, window, rng):
    """a block from [(literals, match length, offset)] and `tail` last literals against the bytes `window` in front of it, and what
    it decodes to"""
    out, src = bytearray(), bytearray()
    for ll, ml, off in seqs:
        lits = rng.randint(0, 256, size=ll).astype(np.uint8).tobytes()
        out.append((min(ll, 15) << 4) | min(ml - 4, 15))
        if ll >= 15:
            out += b"\xff" * ((ll - 15) // 255) + bytes([(ll - 15) % 255])
        out += lits
        src += lits
        out += bytes([off & 255, off >> 8])
        if ml - 4 >= 15:
            out += b"\xff" * ((ml - 19) // 255) + bytes([(ml - 19) % 255])
        for _ in range(ml):
            src.append((window + bytes(src))[len(window) + len(src) - off])
    lits = rng.randint(0, 256, size=tail).astype(np.uint8).tobytes()
    out += FM.literal_run(lits)
    src += lits
    return bytes(out), bytes(src)


def test_hand_built_block_the_leading_run_is_the_all_literals_page(oracle):
    """s_0 = a match of 4 at position 0, s_1 = a match of 7 directly behind it, T = 12: the cut behind s_0 would consume exactly 12
    bytes with a match in them, the cut behind s_1 is valid -- the page is the all-literals one, whatever comes behind"""
    rng = np.random.RandomState(5)
    window = rng.randint(0, 256, size=64).astype(np.uint8).tobytes()
    e, src = build_block([(0, 4, 64), (0, 7, 40), (3, 9, 20)], 20, window, rng)
    n = len(src)
    lz4_check.check_block(e, n, dict_len=64)
    assert oracle.decompress_block(e, n, dict_bytes=window) == (n, src)
    seqs, _ = DM.sequences(e, n)
    assert seqs[:2] == [(0, 4, 3), (4, 11, 6)]
    assert DM.valid_cuts(e, n, 12)[:2] == [False, True]
    assert DM.cut_is_valid(seqs[0], n, 12) == (False, 8)                  # 4 + 8 = 12 bytes: one short
    assert FM.cut_is_valid(seqs[0], n, 12)[0]                             # (7m's three conditions hold)
    pg, used, j = DM.page(e, src, 12)
    assert (pg, used, j) == (FM.literal_run(src[:11]), 11, -1)
    lz4_check.check_block(pg, used, dict_len=64)
    # what the page must not be: 12 bytes with a match in them
    bad = e[:3] + FM.literal_run(src[4:12])
    with pytest.raises(lz4_check.BlockRuleError) as err:
        lz4_check.check_block(bad, 12, dict_len=64)
    assert err.value.rule == lz4_check.SHORT
    # the last valid cut would keep both matches
    assert DM.page_last_valid(e, src, 12) == (e[:6] + FM.literal_run(src[11:16]), 16, 1)
    for t in range(1, len(e) + 3):
        check_page(oracle, window, src, e, t)
    assert DM.page(e, src, len(e)) == (e, n, None)


def test_a_block_that_fits_is_the_page_whatever_its_cuts(oracle):
    """|E| <= T comes first: a block of 12 bytes -- a match of 4 at position 0, one of 18, five literals -- at T = 12 is the page
    although the cut behind its first sequence is not valid"""
    rng = np.random.RandomState(6)
    window = rng.randint(0, 256, size=64).astype(np.uint8).tobytes()
    e, src = build_block([(0, 4, 64), (0, 18, 50)], 5, window, rng)
    assert len(e) == 12 and len(src) == 27
    lz4_check.check_block(e, 27, dict_len=64)
    assert oracle.decompress_block(e, 27, dict_bytes=window) == (27, src)
    assert DM.valid_cuts(e, 27, 12) == [False, True]
    assert DM.page(e, src, 12) == (e, 27, None)
    assert DM.page(e, src, 11)[2] == -1


def test_symbols_declared_listed_and_exported(slz4):
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in include/mi355lz4.h"
        assert name in slz4.DECLARED_SYMBOLS, name
        assert getattr(slz4.lib, name).argtypes is not None, name + " has no sig() declaration"
    assert len(slz4.lib.mi355lz4_compress_pages_fastdict_device.argtypes) == 16      # the fast call's, and hd
    assert len(slz4.lib.mi355lz4_compress_pages_fastdict.argtypes) == 15
    assert len(slz4.lib.mi355lz4_compress_pages_fast_device.argtypes) == 15
    assert len(slz4.lib.mi355lz4_compress_pages_fast.argtypes) == 14


def test_mirrors_are_present(slz4):
    for m in ("compress_pages_fastdict_device", "compress_pages_fastdict"):
        assert hasattr(slz4.Engine, m)
    hpp = open(os.path.join(ROOT, "include", "streamly_lz4.hpp")).read()
    assert re.search(r"\bcompressPagesWithDictFast\s*\(", hpp)
    cpp = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "host_stream.cpp")).read()
    assert "Engine::compressPagesWithDictFast" in cpp and "mi355lz4_compress_pages_fastdict(" in cpp
    shim = open(os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")).read()
    for name in SYMBOLS:
        assert '"mi355lz4.h %s"' % name in shim, name + " is not imported by the Haskell shim"
    assert "compressChunksPagedWithDictFast" in shim
    kh = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "kernels.h")).read()
    assert "launch_pages_fastdict" in kh and "PagesFastDictArgs" in kh


def test_header_states_the_contract():
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    top = header.split("engine lifecycle")[0]
    for name in ("_compress_pages_fastdict_device", "_compress_pages_fastdict:"):
        assert name in top, name + " is missing from the 'what a call may write' block"
    for phrase in ("inEnd_j + r_j >= 13", "leading sequences whose cuts are all valid", "all-literals page",
                   "compLen >= T - 1", "With keep == 0 the calls are legal", "The object is only", "profiles/dictpages_rate.json"):
        assert phrase in header, phrase
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 7n." in design and "k_pages_fastdict" in design
    assert "compress_pages_fastdict" in open(os.path.join(ROOT, "README.md")).read()
    assert "compress_pages_fastdict" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fam = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "kernels.hip")).read()
    assert "k_pages_fastdict" in fam


def test_haskell_shim_imports_match_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_haskell_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    for name in SYMBOLS:
        assert name in r.stdout, name + " was not among the imports that were checked"


def test_null_and_argument_checks_need_no_device(slz4):
    """each returns E_ARG in front of the first HIP call, and mi355lz4_last_error() names the call"""
    L = slz4.lib
    assert L.mi355lz4_compress_pages_fastdict_device(None, None, None, None, None, 1, None, 1, 1, 8, None, 64, None, None, None,
                                                     None) == E_ARG
    assert b"compress_pages_fastdict_device" in L.mi355lz4_last_error()
    assert L.mi355lz4_compress_pages_fastdict(None, None, None, None, 1, 16, 1, 1, 8, None, 64, None, None, None, None) == E_ARG
    assert b"compress_pages_fastdict" in L.mi355lz4_last_error()


def test_sanitizer_builds_list_the_stub():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    lists = [ln.split(" ")[0] for ln in mk.splitlines() if re.match(r"\w*SAN_SRCS :=", ln)]
    assert set(lists) >= {"SAN_SRCS", "DICT_SAN_SRCS", "HCDICT_SAN_SRCS", "PAGES_SAN_SRCS", "FASTDICT_SAN_SRCS", "FASTPAGES_SAN_SRCS",
                          "DICTPAGES_SAN_SRCS"}
    for var in lists:
        line = [ln for ln in mk.splitlines() if ln.startswith(var + " ")][0]
        assert "tests/native/san_stubs_dictpages.cpp" in line, "%s: the dictionary page call's launcher would not link" % var
    assert re.search(r"^asan-dictpages:", mk, re.M)
    assert "launch_pages_fastdict" in open(os.path.join(ROOT, "tests", "native", "san_stubs_dictpages.cpp")).read()


def test_argument_checks_under_sanitizers():
    """the host code of the calls from a program of its own (tests/native/dictpages_args_main.cpp), ASan + UBSan, no device"""
    if shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("g++ or the HIP host headers are not available")
    r = subprocess.run(["make", "-C", ROOT, "asan-dictpages"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "dictpages_args_main ok" in r.stdout
    for bad in ("ERROR: AddressSanitizer", "runtime error:"):
        assert bad not in r.stdout + r.stderr
