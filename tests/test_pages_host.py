"""Fixed-size output pages without a GPU (mi355lz4_compress_pages_device, mi355lz4_compress_pages): the CPU model of fill mode
(tests/native/fill_model.c) against the reference's recorded results on the whole grid -- and against the reference itself where
oracle/_ref is built --, which fill rule ends how many pages, the surface -- symbols, header, bindings, the C++ and Haskell
mirrors -- and the argument checks that need no device, from Python and from a program of its own under ASan + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pages_cases as PC  # noqa: E402
import pages_model as PM  # noqa: E402

E_ARG = -3
SYMBOLS = ["mi355lz4_compress_pages_device", "mi355lz4_compress_pages"]
REF_SO = os.path.join(ROOT, "oracle", "_ref", "liblz4ref.so")


@pytest.fixture(scope="module")
def model_grid():
    """the model on every single-page case: {series: [(ret, used, rule, bytes)]}; computed once, never changed"""
    return {key: [PM.page(PC.input_bytes(name), t) for t in sizes] for key, name, sizes in PC.singles()}


@pytest.fixture(scope="module")
def model_chains():
    """the model on every chain, maxPages large enough: {key: ([(page, compLen, srcLen, rule)], consumed)}"""
    return {PC.chain_key(name, t): PM.chain(PC.input_bytes(name), t, len(PC.input_bytes(name)) + 1) for name, t in PC.CHAINS}


def test_grid_is_the_one_the_golden_was_made_from():
    keys = {key for key, _, _ in PC.singles()} | {PC.chain_key(n, t) for n, t in PC.CHAINS}
    assert keys == set(PM.golden()), "tests/golden/pages_vectors.json is stale: python tests/golden/make_pages_golden.py"
    for key, _, sizes in PC.singles():
        assert len(PM.golden_pages(key)) == len(sizes), key
    assert sum(len(sizes) for _, _, sizes in PC.singles()) == 5 * 601 + 2 * 600 + 3 * 2 + 7 * 3


def test_model_equals_the_golden_on_the_grid(model_grid):
    for key, name, sizes in PC.singles():
        for t, got, want in zip(sizes, model_grid[key], PM.golden_pages(key)):
            assert (got[0], got[1], PM.sha(got[3])) == want, "%s at pageSize %d: model %r, reference %r" % (key, t, got[:2], want)


def test_model_equals_the_golden_on_the_chains(model_chains):
    for name, t in PC.CHAINS:
        key = PC.chain_key(name, t)
        pages, consumed = model_chains[key]
        want = PM.golden_pages(key)
        assert [(c, u, PM.sha(b)) for b, c, u, _ in pages] == want, key
        assert consumed == sum(u for _, u, _ in want), key
        n = len(PC.input_bytes(name))
        assert consumed == (0 if t == 1 else n), key          # pageSize 1: a zero token that consumes nothing


def test_the_seam_changes_the_bytes():
    """65546 bytes are the last length of the 16-bit table.  The three seam inputs are prefixes of one text and a page of 4096 bytes
    holds only their common front, so what the reference writes for it differs by the table type alone: 65546 against 65547
    differ, 65547 and 65548 (both 32-bit) agree."""
    a, b, c = (PC.input_bytes("text%d" % n) for n in (65546, 65547, 65548))
    assert b.startswith(a) and c.startswith(b)
    p16, p32, p32b = (PM.golden_pages("seam/text%d" % n)[0] for n in (65546, 65547, 65548))
    assert p16 != p32
    assert p32 == p32b


def test_model_equals_the_reference_itself(model_grid, model_chains):
    """where oracle/_ref is built: the same calls on the reference, bytes compared in full (the golden holds truncated sums)"""
    if not os.path.exists(REF_SO):
        assert PM.golden(), "no reference build here: the golden stands in for it (test_model_equals_the_golden_*)"
        return
    L = C.CDLL(REF_SO)
    L.LZ4_compress_destSize.restype = C.c_int
    L.LZ4_compress_destSize.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int]

    def ref(buf, pos, n, t):
        dst = np.zeros(max(t, 0) + 64, dtype=np.uint8)
        m = C.c_int(n)
        r = L.LZ4_compress_destSize(buf.ctypes.data + pos, dst.ctypes.data, C.byref(m), t)
        return r, m.value, dst[:max(r, 0)].tobytes()

    for key, name, sizes in PC.singles():
        data = PC.input_bytes(name)
        buf = np.frombuffer(data + bytes(64), dtype=np.uint8)
        for t, got in zip(sizes, model_grid[key]):
            assert (got[0], got[1], got[3]) == ref(buf, 0, len(data), t), "%s at pageSize %d" % (key, t)
    for name, t in PC.CHAINS:
        data = PC.input_bytes(name)
        buf = np.frombuffer(data + bytes(64), dtype=np.uint8)
        pos = 0
        for page, c, u, _ in model_chains[PC.chain_key(name, t)][0]:
            assert (c, u, page) == ref(buf, pos, len(data) - pos, t), "%s page at %d" % (PC.chain_key(name, t), pos)
            pos += u


def test_every_fill_rule_ends_pages_on_the_grid(model_grid, model_chains):
    """a grid that never reached a rule would test nothing of it"""
    counts = [0] * len(PM.RULES)
    for pages in model_grid.values():
        for p in pages:
            counts[p[2]] += 1
    for pages, _ in model_chains.values():
        for p in pages:
            counts[p[3]] += 1
    print(dict(zip(PM.RULES, counts)))
    for rule in (1, 2, 3, 4):
        assert counts[rule] >= 5, "%s ended %d pages" % (PM.RULES[rule], counts[rule])
    assert counts[3] >= 200, "the shortened match ended %d pages" % counts[3]
    # the long zeros carry the shortened matches, on both table types
    for key in ("grid/zeros65000", "grid/zeros70000"):
        assert sum(1 for p in model_grid[key] if p[2] == 3) >= 100, key


def test_progress_bound_on_the_grid(model_grid, model_chains):
    """every page that leaves input behind consumes at least (T - 1) - (T + 240) / 256 bytes"""
    for key, name, sizes in PC.singles():
        n = len(PC.input_bytes(name))
        for t, p in zip(sizes, model_grid[key]):
            if p[0] > 0 and p[1] < n:
                assert p[1] >= PC.min_progress(t), (key, t, p[:2])
    for name, t in PC.CHAINS:
        pages, consumed = model_chains[PC.chain_key(name, t)]
        for _, _, u, _ in pages[:-1]:
            assert u >= PC.min_progress(t), (name, t, u)


def test_model_under_sanitizers():
    """the model's own main: part of the grid with every page in a buffer of exactly its size, ASan + UBSan"""
    d = tempfile.mkdtemp(prefix="fillmodel_san")
    exe = os.path.join(d, "fill_model_san")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DFILL_MODEL_MAIN", "-o", exe, PM.SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    shutil.rmtree(d, ignore_errors=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "pages ok" in r.stdout
    for bad in ("ERROR: AddressSanitizer", "runtime error:", "FAIL"):
        assert bad not in r.stdout + r.stderr


# ---- the surface ------------------------------------------------------------------------------------------------------------------

def test_symbols_declared_listed_and_exported(slz4):
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in include/mi355lz4.h"
        assert name in slz4.DECLARED_SYMBOLS, name
        assert getattr(slz4.lib, name).argtypes is not None, name + " has no sig() declaration"
    assert len(slz4.lib.mi355lz4_compress_pages_device.argtypes) == 14
    assert len(slz4.lib.mi355lz4_compress_pages.argtypes) == 13


def test_mirrors_are_present(slz4):
    for m in ("compress_pages_device", "compress_pages"):
        assert hasattr(slz4.Engine, m)
    hpp = open(os.path.join(ROOT, "include", "streamly_lz4.hpp")).read()
    assert re.search(r"\bcompressPages\s*\(", hpp)
    cpp = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "host_stream.cpp")).read()
    assert "Engine::compressPages" in cpp
    shim = open(os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")).read()
    for name in SYMBOLS:
        assert '"mi355lz4.h %s"' % name in shim, name + " is not imported by the Haskell shim"
    assert "compressChunksPaged" in shim


def test_header_states_the_contract():
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    top = header.split("engine lifecycle")[0]
    assert "_compress_pages_device" in top, "missing from the 'what a call may write' block"
    assert "[0, headerKind + pageCompLen" in top
    assert "LZ4_compress_destSize" in header
    assert "(T - 1) - (T + 240) / 256" in header, "the progress bound a caller sizes maxPages by"
    assert "a call's parallelism is its number of inputs" in header
    assert "checksummed page format is out of scope" in header
    assert "profiles/pages_rate.json" in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7k" in design and "k_exact_pages" in design and "fill_encode_page" in design
    assert "compress_pages" in open(os.path.join(ROOT, "README.md")).read()
    assert "compress_pages" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_haskell_shim_imports_match_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_haskell_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    for name in SYMBOLS:
        assert name in r.stdout, name + " was not among the imports that were checked"


def test_null_and_argument_checks_need_no_device(slz4):
    """each returns E_ARG in front of the first HIP call, and mi355lz4_last_error() names the call"""
    L = slz4.lib
    assert L.mi355lz4_compress_pages_device(None, None, None, None, 1, None, 1, 8, None, 64, None, None, None, None) == E_ARG
    assert b"null ctx" in L.mi355lz4_last_error()
    assert L.mi355lz4_compress_pages(None, None, None, 1, 16, 1, 8, None, 64, None, None, None, None) == E_ARG
    assert b"null ctx" in L.mi355lz4_last_error()


def test_sanitizer_builds_list_the_stub():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    for var in ("SAN_SRCS", "DICT_SAN_SRCS", "HCDICT_SAN_SRCS", "PAGES_SAN_SRCS"):
        line = [ln for ln in mk.splitlines() if ln.startswith(var)][0]
        assert "tests/native/san_stubs_pages.cpp" in line, "%s would not link" % var
    assert re.search(r"^asan-pages:", mk, re.M)


def test_argument_checks_under_sanitizers():
    """the host code of the calls from a program of its own (tests/native/pages_args_main.cpp), ASan + UBSan, no device"""
    if shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("g++ or the HIP host headers are not available")
    r = subprocess.run(["make", "-C", ROOT, "asan-pages"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "pages_args_main ok" in r.stdout
    for bad in ("ERROR: AddressSanitizer", "runtime error:"):
        assert bad not in r.stdout + r.stderr
