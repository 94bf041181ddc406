"""The high-compression dictionary calls without a GPU (mi355lz4_hcdict_*, mi355lz4_compress_hcdict_device, mi355lz4_compress_hcdict):
the surface -- symbols, header, bindings, the C++ and Haskell mirrors -- and the argument checks that need no device, from Python and
from a program of its own under ASan + UBSan."""
import ctypes as C
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

E_ARG = -3
SYMBOLS = ["mi355lz4_hcdict_create", "mi355lz4_hcdict_destroy", "mi355lz4_hcdict_load", "mi355lz4_hcdict_size",
           "mi355lz4_compress_hcdict_device", "mi355lz4_compress_hcdict"]


def test_symbols_declared_listed_and_exported(slz4):
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    assert re.search(r"typedef\s+struct\s+mi355lz4_hcdict\s+mi355lz4_hcdict\s*;", header)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in include/mi355lz4.h"
        assert name in slz4.DECLARED_SYMBOLS, name
        assert getattr(slz4.lib, name).argtypes is not None, name + " has no sig() declaration"


def test_mirrors_are_present(slz4):
    for m in ("compress_hcdict_device", "compress_hcdict"):
        assert hasattr(slz4.Engine, m)
    for m in ("load", "__len__", "close", "image"):
        assert hasattr(slz4.HcDict, m)
    hpp = open(os.path.join(ROOT, "include", "streamly_lz4.hpp")).read()
    assert re.search(r"\bclass\s+HcDict\s*\{", hpp)
    assert re.search(r"\bcompressWithDictHC\s*\(", hpp)
    cpp = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "host_stream.cpp")).read()
    assert "Engine::compressWithDictHC" in cpp and "HcDict::load" in cpp
    shim = open(os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")).read()
    for name in SYMBOLS:
        assert '"mi355lz4.h %s"' % name in shim, name + " is not imported by the Haskell shim"
    assert "compressChunksWithDictHC" in shim and "newHcDict" in shim and "loadHcDict" in shim


def test_header_states_the_contract():
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    top = header.split("engine lifecycle")[0]
    for name in ("_hcdict_load", "_compress_hcdict_device", "_compress_hcdict "):
        assert name in top, name + " is missing from the 'what a call may write' block"
    assert "second block of the two-block linked call" in header
    assert "level 0 against a dictionary is mi355lz4_compress_dict_device" in header
    assert "levels 1..12: mi355lz4_compress_hcdict_device" in header, "the level-0 dictionary call does not point here"
    assert "profiles/hcdict_rate.json" in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7j" in design and "k_encode_hc_dict" in design and "k_hcdict_build" in design
    assert "compress_hcdict" in open(os.path.join(ROOT, "README.md")).read()


def test_haskell_shim_imports_match_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_haskell_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    for name in SYMBOLS:
        assert name in r.stdout, name + " was not among the imports that were checked"


def test_null_and_argument_checks_need_no_device(slz4):
    """each returns E_ARG in front of the first HIP call, and mi355lz4_last_error() names the call"""
    L = slz4.lib
    sz = C.c_size_t(7)
    out = C.c_void_p(7)
    assert L.mi355lz4_hcdict_create(None, C.byref(out)) == E_ARG and not out.value
    assert b"hcdict_create" in L.mi355lz4_last_error()
    assert L.mi355lz4_hcdict_create(None, None) == E_ARG
    L.mi355lz4_hcdict_destroy(None)
    assert L.mi355lz4_hcdict_load(None, None, None, 0) == E_ARG
    assert b"hcdict_load" in L.mi355lz4_last_error()
    assert L.mi355lz4_hcdict_size(None) == E_ARG
    assert b"hcdict_size" in L.mi355lz4_last_error()
    assert L.mi355lz4_compress_hcdict_device(None, None, None, None, None, 0, 0, 0, 8, None, 0, None) == E_ARG
    assert b"compress_hcdict_device" in L.mi355lz4_last_error()
    assert L.mi355lz4_compress_hcdict(None, None, None, None, 0, 8, None, 0, C.byref(sz), None, None) == E_ARG
    assert sz.value == 0 and b"compress_hcdict" in L.mi355lz4_last_error()
    assert L.mi355lz4_compress_hcdict(None, None, None, None, 0, 8, None, 0, None, None, None) == E_ARG


def test_sanitizer_builds_list_the_stubs():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    san = [ln for ln in mk.splitlines() if ln.startswith("SAN_SRCS")][0]
    assert "tests/native/san_stubs_hcdict.cpp" in san, "make asan / make tsan would not link"
    assert re.search(r"^asan-hcdict:", mk, re.M)


def test_argument_checks_under_sanitizers():
    """the host code of the calls from a program of its own (tests/native/hcdict_args_main.cpp), ASan + UBSan, no device"""
    if shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("g++ or the HIP host headers are not available")
    r = subprocess.run(["make", "-C", ROOT, "asan-hcdict"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "hcdict_args_main ok" in r.stdout
    for bad in ("ERROR: AddressSanitizer", "runtime error:"):
        assert bad not in r.stdout + r.stderr
