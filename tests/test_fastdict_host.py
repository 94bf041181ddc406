"""The level-0 calls against a prepared dictionary without a GPU (mi355lz4_compress_fastdict_device, mi355lz4_compress_fastdict,
mi355lz4_debug_hcdict_fast_image): the surface -- symbols, header, bindings, the C++ and Haskell mirrors -- and the argument checks
that need no device, from Python and from a program of its own under ASan + UBSan."""
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
SYMBOLS = ["mi355lz4_compress_fastdict_device", "mi355lz4_compress_fastdict"]
HOOK = "mi355lz4_debug_hcdict_fast_image"


def test_symbols_declared_listed_and_exported(slz4):
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in include/mi355lz4.h"
        assert name in slz4.DECLARED_SYMBOLS, name
        assert getattr(slz4.lib, name).argtypes is not None, name + " has no sig() declaration"
    # the diagnostic hook is exported and has a signature, and stays out of the public header like mi355lz4_debug_hcdict_image
    assert getattr(slz4.lib, HOOK).argtypes is not None
    assert HOOK not in header and "mi355lz4_debug_hcdict_image" not in header


def test_mirrors_are_present(slz4):
    for m in ("compress_fastdict_device", "compress_fastdict"):
        assert hasattr(slz4.Engine, m)
    assert hasattr(slz4.HcDict, "fast_image") and slz4.HcDict.FAST_IMAGE_BYTES == 10240 + 16
    assert slz4.HcDict.IMAGE_BYTES == 221248, "the hash-chain image keeps its size"
    kh = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "kernels.h")).read()
    assert re.search(r"#define\s+FASTDICT_TABLE_BYTES\s+10240\b", kh)
    hpp = open(os.path.join(ROOT, "include", "streamly_lz4.hpp")).read()
    assert re.search(r"\bcompressWithDictFast\s*\(", hpp)
    cpp = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "host_stream.cpp")).read()
    assert "Engine::compressWithDictFast" in cpp and "mi355lz4_compress_fastdict(" in cpp
    shim = open(os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")).read()
    for name in SYMBOLS:
        assert '"mi355lz4.h %s"' % name in shim, name + " is not imported by the Haskell shim"
    assert "compressChunksWithDictFast" in shim


def test_header_states_the_contract():
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    top = header.split("engine lifecycle")[0]
    for name in ("_compress_fastdict_device", "_compress_fastdict:"):
        assert name in top, name + " is missing from the 'what a call may write' block"
    assert "second block of the two-block linked call [D[-keep:], B_i]" in header
    assert "MI355LZ4_FASTDICT_WAVES" in header
    assert "profiles/fastdict_rate.json" in header
    # the sentences the older dictionary calls are found by
    assert "level 0 against a dictionary is mi355lz4_compress_dict_device" in header
    assert "levels 1..12: mi355lz4_compress_hcdict_device" in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7l" in design and "k_encode_fastdict" in design and "k_hcdict_build_fast" in design
    assert "compress_fastdict" in open(os.path.join(ROOT, "README.md")).read()
    assert "compress_fastdict" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_haskell_shim_imports_match_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_haskell_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    for name in SYMBOLS:
        assert name in r.stdout, name + " was not among the imports that were checked"


def test_null_and_argument_checks_need_no_device(slz4):
    """each returns E_ARG in front of the first HIP call, and mi355lz4_last_error() names the call"""
    L = slz4.lib
    sz = C.c_size_t(7)
    assert L.mi355lz4_compress_fastdict_device(None, None, None, None, None, 0, 0, 0, 1, 8, None, 0, None) == E_ARG
    assert b"compress_fastdict_device" in L.mi355lz4_last_error()
    assert L.mi355lz4_compress_fastdict(None, None, None, None, 0, 1, 8, None, 0, C.byref(sz), None, None) == E_ARG
    assert sz.value == 0 and b"compress_fastdict" in L.mi355lz4_last_error()
    assert L.mi355lz4_compress_fastdict(None, None, None, None, 0, 1, 8, None, 0, None, None, None) == E_ARG
    assert L.mi355lz4_debug_hcdict_fast_image(None, None) == E_ARG
    assert b"debug_hcdict_fast_image" in L.mi355lz4_last_error()


def test_sanitizer_builds_list_the_stubs():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    for var in ("SAN_SRCS", "DICT_SAN_SRCS", "HCDICT_SAN_SRCS", "PAGES_SAN_SRCS", "FASTDICT_SAN_SRCS"):
        line = [ln for ln in mk.splitlines() if ln.startswith(var + " ")][0]
        assert "tests/native/san_stubs_fastdict.cpp" in line, "%s: hcdict_load's new launcher would not link" % var
    assert re.search(r"^asan-fastdict:", mk, re.M)
    stubs = open(os.path.join(ROOT, "tests", "native", "san_stubs_fastdict.cpp")).read()
    for fn in ("launch_hcdict_build_fast", "encode_fastdict_grid", "launch_encode_fastdict"):
        assert fn in stubs


def test_argument_checks_under_sanitizers():
    """the host code of the calls from a program of its own (tests/native/fastdict_args_main.cpp), ASan + UBSan, no device"""
    if shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("g++ or the HIP host headers are not available")
    r = subprocess.run(["make", "-C", ROOT, "asan-fastdict"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "fastdict_args_main ok" in r.stdout
    for bad in ("ERROR: AddressSanitizer", "runtime error:"):
        assert bad not in r.stdout + r.stderr
