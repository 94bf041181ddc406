"""The dictionary-set calls without a GPU (mi355lz4_dictset_create / _destroy / _count, mi355lz4_compress_fastdict_multi_device,
mi355lz4_compress_fastdict_multi, mi355lz4_decompress_dict_multi_device, mi355lz4_decompress_dict_multi and the hook
mi355lz4_debug_dictset_last): the surface -- symbols, header, bindings, the C++ and Haskell mirrors -- and the argument checks that
need no device, from Python and from a program of its own under ASan + UBSan."""
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
SYMBOLS = ["mi355lz4_dictset_create", "mi355lz4_dictset_destroy", "mi355lz4_dictset_count",
           "mi355lz4_compress_fastdict_multi_device", "mi355lz4_compress_fastdict_multi",
           "mi355lz4_decompress_dict_multi_device", "mi355lz4_decompress_dict_multi"]
HOOK = "mi355lz4_debug_dictset_last"


def test_symbols_declared_listed_and_exported(slz4):
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in include/mi355lz4.h"
        assert name in slz4.DECLARED_SYMBOLS, name
        assert getattr(slz4.lib, name).argtypes is not None, name + " has no sig() declaration"
    assert re.search(r"typedef\s+struct\s+mi355lz4_dictset\s+mi355lz4_dictset\s*;", header)
    assert re.search(r"#define\s+MI355LZ4_BLK_E_DICT\s+\(-0x7F000006\)", header)
    # the diagnostic hook is exported and has a signature, and stays out of the public header like the other mi355lz4_debug_* hooks
    assert getattr(slz4.lib, HOOK).argtypes is not None
    assert HOOK not in header and HOOK not in slz4.DECLARED_SYMBOLS


def test_mirrors_are_present(slz4):
    for m in ("compress_fastdict_multi_device", "compress_fastdict_multi", "decompress_dict_multi_device", "decompress_dict_multi"):
        assert hasattr(slz4.Engine, m), m
    assert hasattr(slz4, "DictSet") and hasattr(slz4.DictSet, "last") and slz4.DictSet.BLK_E_DICT == -0x7F000006
    kh = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "kernels.h")).read()
    assert re.search(r"#define\s+BLK_E_DICT\s+\(-0x7F000006\)", kh) and re.search(r"#define\s+DICTSET_MAX\s+65536\b", kh)
    hpp = open(os.path.join(ROOT, "include", "streamly_lz4.hpp")).read()
    assert re.search(r"\bclass\s+DictSet\b", hpp)
    assert re.search(r"\bcompressWithDictsFast\s*\(", hpp) and re.search(r"\bdecompressWithDicts\s*\(", hpp)
    cpp = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "host_stream.cpp")).read()
    assert "Engine::compressWithDictsFast" in cpp and "mi355lz4_compress_fastdict_multi(" in cpp
    assert "Engine::decompressWithDicts" in cpp and "mi355lz4_decompress_dict_multi(" in cpp
    assert "DictSet::DictSet" in cpp and "mi355lz4_dictset_create(" in cpp
    shim = open(os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")).read()
    for name in SYMBOLS:
        assert '"mi355lz4.h %s"' % name in shim, name + " is not imported by the Haskell shim"
    for name in ("newDictSet", "compressChunksWithDictsFast", "decompressChunksWithDicts"):
        assert re.search(r"^%s\s*$|^%s\s*::" % (name, name), shim, re.M), name


def test_header_states_the_contract():
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    top = header.split("engine lifecycle")[0]
    for name in ("_dictset_create", "_compress_fastdict_multi_device", "_decompress_dict_multi_device", "_compress_fastdict_multi and",
                 "MI355LZ4_BLK_E_DICT"):
        assert name in top, name + " is missing from the 'what a call may write' block"
    assert "destroying a member before the set is the caller's" in header
    assert "BORROWED" in header and "grid + G - 1" in header
    assert "profiles/dictset_rate.json" in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7o" in design and "k_encode_fastdict_multi" in design and "k_decode_dict_multi" in design
    assert "compress_fastdict_multi" in open(os.path.join(ROOT, "README.md")).read()
    assert "compress_fastdict_multi" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_haskell_shim_imports_match_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_haskell_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    for name in SYMBOLS:
        assert name in r.stdout, name + " was not among the imports that were checked"


def test_null_and_argument_checks_need_no_device(slz4):
    """each returns E_ARG in front of the first HIP call, and mi355lz4_last_error() names the call"""
    L = slz4.lib
    out = C.c_void_p(5)
    assert L.mi355lz4_dictset_create(None, None, 1, C.byref(out)) == E_ARG and not out.value
    assert b"dictset_create" in L.mi355lz4_last_error()
    assert L.mi355lz4_dictset_create(None, None, 1, None) == E_ARG
    assert L.mi355lz4_dictset_count(None) == E_ARG and b"dictset_count" in L.mi355lz4_last_error()
    L.mi355lz4_dictset_destroy(None)
    assert L.mi355lz4_debug_dictset_last(None, None) == E_ARG and b"debug_dictset_last" in L.mi355lz4_last_error()
    assert L.mi355lz4_compress_fastdict_multi_device(None, None, None, None, None, None, 0, 0, 0, 1, 8, None, 0, None) == E_ARG
    assert b"compress_fastdict_multi_device" in L.mi355lz4_last_error()
    sz = C.c_size_t(7)
    assert L.mi355lz4_compress_fastdict_multi(None, None, None, None, None, 0, 1, 8, None, 0, C.byref(sz), None, None) == E_ARG
    assert sz.value == 0 and b"compress_fastdict_multi" in L.mi355lz4_last_error()
    assert L.mi355lz4_compress_fastdict_multi(None, None, None, None, None, 0, 1, 8, None, 0, None, None, None) == E_ARG
    assert L.mi355lz4_decompress_dict_multi_device(None, None, 0, None, 0, 8, 0, None, None, None, None, None, None) == E_ARG
    assert b"decompress_dict_multi_device" in L.mi355lz4_last_error()
    sz, got = C.c_size_t(7), C.c_int(7)
    assert L.mi355lz4_decompress_dict_multi(None, None, 0, 8, 0, None, None, None, 0, C.byref(sz), None, 0, C.byref(got)) == E_ARG
    assert sz.value == 0 and got.value == 0 and b"decompress_dict_multi" in L.mi355lz4_last_error()


def test_sanitizer_builds_list_the_stubs():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    lists = [ln for ln in mk.splitlines() if re.match(r"^[A-Z]*_?SAN_SRCS :=", ln)]
    assert len(lists) >= 8, "the Makefile's *_SAN_SRCS lists: the two host programs and one per family of calls"
    for ln in lists:
        assert "tests/native/san_stubs_dictset.cpp" in ln, "%s: the new launchers would not link" % ln.split()[0]
    assert re.search(r"^asan-dictset:", mk, re.M)
    stubs = open(os.path.join(ROOT, "tests", "native", "san_stubs_dictset.cpp")).read()
    for fn in ("launch_dictset_group", "launch_encode_fastdict_multi", "launch_decode_dict_multi"):
        assert fn in stubs


def test_argument_checks_under_sanitizers():
    """the host code of the calls from a program of its own (tests/native/dictset_args_main.cpp), ASan + UBSan, no device"""
    if shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("g++ or the HIP host headers are not available")
    r = subprocess.run(["make", "-C", ROOT, "asan-dictset"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "dictset_args_main ok" in r.stdout
    for bad in ("ERROR: AddressSanitizer", "runtime error:"):
        assert bad not in r.stdout + r.stderr
