"""The fast linked streams without a GPU (mi355lz4_fstreams_create / _destroy / _count / _reset / _set_dict,
mi355lz4_compress_streams_fast_device, mi355lz4_compress_streams_fast and the hook mi355lz4_debug_fstreams_peek): the surface --
symbols, header, bindings, the C++ and Haskell mirrors -- and the argument checks that need no device, from Python and from a
program of its own under ASan + UBSan.  (A set cannot be had without a device: the checks that need one run from Python in
tests/test_fstreams_gpu.py and, on a set that is a plain struct, in tests/native/fstreams_args_main.cpp.)"""
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
SYMBOLS = ["mi355lz4_fstreams_create", "mi355lz4_fstreams_destroy", "mi355lz4_fstreams_count", "mi355lz4_fstreams_reset",
           "mi355lz4_fstreams_set_dict", "mi355lz4_compress_streams_fast_device", "mi355lz4_compress_streams_fast"]
HOOK = "mi355lz4_debug_fstreams_peek"
_i32p = C.POINTER(C.c_int32)


def test_symbols_declared_listed_and_exported(slz4):
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in include/mi355lz4.h"
        assert name in slz4.DECLARED_SYMBOLS, name
        assert getattr(slz4.lib, name).argtypes is not None, name + " has no sig() declaration"
    assert re.search(r"typedef\s+struct\s+mi355lz4_fstreams\s+mi355lz4_fstreams\s*;", header)
    # the diagnostic hook is exported and has a signature, and stays out of the public header like the other mi355lz4_debug_* hooks
    assert getattr(slz4.lib, HOOK).argtypes is not None
    assert HOOK not in header and HOOK not in slz4.DECLARED_SYMBOLS


def test_mirrors_are_present(slz4):
    for m in ("compress_streams_fast_device", "compress_streams_fast"):
        assert hasattr(slz4.Engine, m), m
    assert hasattr(slz4, "FastCompressStreams") and "FastCompressStreams" in slz4.__all__
    for m in ("reset", "set_dict", "peek", "close"):
        assert hasattr(slz4.FastCompressStreams, m), m
    kh = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "kernels.h")).read()
    assert re.search(r"#define\s+FSTREAM_SLOT_BYTES\s+DSTREAM_SLOT_BYTES\b", kh) and re.search(r"\bstruct\s+FStreamsArgs\b", kh)
    hpp = open(os.path.join(ROOT, "include", "streamly_lz4.hpp")).read()
    assert re.search(r"\bclass\s+FastCompressStreams\b", hpp) and re.search(r"\bsetDict\s*\(", hpp)
    assert re.search(r"\bcompressStreamsFast\s*\(", hpp)
    cpp = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "host_stream.cpp")).read()
    assert "Engine::compressStreamsFast" in cpp and "mi355lz4_compress_streams_fast(" in cpp
    assert "FastCompressStreams::FastCompressStreams" in cpp and "mi355lz4_fstreams_create(" in cpp
    assert "FastCompressStreams::setDict" in cpp and "mi355lz4_fstreams_set_dict(" in cpp
    shim = open(os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")).read()
    for name in SYMBOLS:
        assert '"mi355lz4.h %s"' % name in shim, name + " is not imported by the Haskell shim"
    for name in ("newFastStreams", "compressChunksManyFast"):
        assert re.search(r"^%s\s*$|^%s\s*::" % (name, name), shim, re.M), name


def test_one_checker_for_both_compress_sets():
    api = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "api.cpp")).read()
    m = re.search(r"static int compress_streams_check\(const mi355lz4_ctx \*c, const SlotSet \*s, int nSlots,", api)
    assert m, "the checker the two sets share takes the slot count"
    assert len(re.findall(r"return compress_streams_check\(", api)) == 2
    assert "StreamTableRing" in open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "engine.hpp")).read()
    assert api.count("stream_table_upload(c, fs->table") == 1


def test_header_states_the_contract():
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    top = header.split("engine lifecycle")[0]
    for name in ("_compress_streams_fast_device", "_fstreams_reset / _fstreams_set_dict", "_compress_streams_fast is", "engine scratch"):
        assert name in top, name + " is missing from the 'what a call may write' block"
    for words in ("second block", "[D, B_k]", "max(|D|, maxBlockLen)", "do not depend on how it is cut into calls",
                  "zero-length array resets a stream's", "LZ4_decompress_safe_continue", "reads no device memory on the host",
                  "An empty stream leaves its slot untouched", "The slot owns its copy", "only level 0 accepted",
                  "block checksums apply", "profiles/fstreams_rate.json"):
        assert words in header, words
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7p" in design and "k_encode_fstreams" in design and "k_fstreams_plan" in design and "k_fstreams_save" in design
    assert "fast linked streams" in open(os.path.join(ROOT, "README.md")).read()


def test_resource_record():
    rec = open(os.path.join(ROOT, "profiles", "fstreams_kernel_resources.txt")).read()

    def row(name):
        m = re.search(r"^%s\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) lds\s+(\d+) scratch\s+(\d+)$" % re.escape(name), rec, re.M)
        assert m, name
        return [int(x) for x in m.groups()]
    for pair in ("ILb0EEv", "ILb1EEv"):
        new, old = row("_Z17k_encode_fstreams%s12FStreamsArgs" % pair), row("_Z17k_encode_fastdict%s12FastDictArgs" % pair)
        # 4 waves a SIMD (512 VGPRs / 128), 16 waves' tables in a CU's LDS, and no more scratch
        assert new[0] <= 128 and new[4] == old[4] == 10240 and new[5] <= old[5], (pair, new, old)


def test_haskell_shim_imports_match_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_haskell_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    for name in SYMBOLS:
        assert name in r.stdout, name + " was not among the imports that were checked"


def test_null_and_argument_checks_need_no_device(slz4):
    """each returns E_ARG in front of the first HIP call, and mi355lz4_last_error() names the call"""
    L = slz4.lib
    out = C.c_void_p(5)
    assert L.mi355lz4_fstreams_create(None, 4, C.byref(out)) == E_ARG and not out.value
    assert b"fstreams_create" in L.mi355lz4_last_error()
    assert L.mi355lz4_fstreams_create(None, 4, None) == E_ARG
    assert L.mi355lz4_fstreams_count(None) == E_ARG and b"fstreams_count" in L.mi355lz4_last_error()
    L.mi355lz4_fstreams_destroy(None)
    assert L.mi355lz4_fstreams_reset(None, None, None, 0) == E_ARG and b"fstreams_reset" in L.mi355lz4_last_error()
    assert L.mi355lz4_fstreams_set_dict(None, None, 0, None, 0) == E_ARG and b"fstreams_set_dict" in L.mi355lz4_last_error()
    cnt = C.c_int(7)
    assert L.mi355lz4_debug_fstreams_peek(None, 0, None, C.byref(cnt)) == E_ARG and cnt.value == 7
    assert b"debug_fstreams_peek" in L.mi355lz4_last_error()
    sf = (C.c_int32 * 2)(0, 1)
    sl = (C.c_int32 * 1)(0)
    assert L.mi355lz4_compress_streams_fast_device(None, None, None, None, None, 0, 16, 1, sf, sl, 1, 1, 8, None, 64, None) == E_ARG
    assert b"compress_streams_fast_device" in L.mi355lz4_last_error()
    sz = C.c_size_t(7)
    assert L.mi355lz4_compress_streams_fast(None, None, None, None, 1, sf, sl, 1, 1, 8, None, 0, C.byref(sz), None, None) == E_ARG
    assert sz.value == 0 and b"compress_streams_fast" in L.mi355lz4_last_error()
    assert L.mi355lz4_compress_streams_fast(None, None, None, None, 1, sf, sl, 1, 1, 8, None, 0, None, None, None) == E_ARG


def test_sanitizer_builds_list_the_stubs():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    lists = [ln for ln in mk.splitlines() if re.match(r"^[A-Z]*_?SAN_SRCS :=", ln)]
    assert len(lists) >= 9, "the Makefile's *_SAN_SRCS lists: the two host programs and one per family of calls"
    for ln in lists:
        assert "tests/native/san_stubs_fstreams.cpp" in ln, "%s: the new launcher would not link" % ln.split()[0]
    assert re.search(r"^asan-fstreams:", mk, re.M) and re.search(r"^asan:.*\basan-fstreams\b", mk, re.M)
    assert "launch_fstreams" in open(os.path.join(ROOT, "tests", "native", "san_stubs_fstreams.cpp")).read()


def test_argument_checks_under_sanitizers():
    """the host code of the calls from a program of its own (tests/native/fstreams_args_main.cpp), ASan + UBSan, no device"""
    if shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("g++ or the HIP host headers are not available")
    r = subprocess.run(["make", "-C", ROOT, "asan-fstreams"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "fstreams_args_main ok" in r.stdout
    for bad in ("ERROR: AddressSanitizer", "runtime error:"):
        assert bad not in r.stdout + r.stderr
