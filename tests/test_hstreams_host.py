"""The level of a set of fast linked streams without a GPU (mi355lz4_fstreams_set_level / _get_level): the surface --
symbols, header, bindings, the C++ and Haskell mirrors -- the attribute's own checks from Python, the argument checks of the two
compress forms at a set level from a program of its own under ASan + UBSan (tests/native/hstreams_args_main.cpp), and the record
of the new kernel's resources next to the kernels it must leave as they were."""
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
SYMBOLS = ["mi355lz4_fstreams_set_level", "mi355lz4_fstreams_get_level"]
CSRC = os.path.join(ROOT, "streamly-lz4_amd", "csrc")


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_symbols_declared_listed_and_exported(slz4):
    header = read("include", "mi355lz4.h")
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in include/mi355lz4.h"
        assert name in slz4.DECLARED_SYMBOLS, name
        assert getattr(slz4.lib, name).argtypes is not None, name + " has no sig() declaration"
    assert re.search(r"int\s+mi355lz4_fstreams_set_level\s*\(\s*mi355lz4_fstreams\s*\*\s*fs\s*,\s*int\s+level\s*\)", header)
    assert re.search(r"int\s+mi355lz4_fstreams_get_level\s*\(\s*const\s+mi355lz4_fstreams\s*\*\s*fs\s*\)", header)
    # a property of the set, not a new device call: the header has no further `int mi355lz4_*_device(` for it
    assert not re.search(r"mi355lz4_\w*(hstreams|streams_hc|streams_fast_hc)\w*_device\s*\(", header)


def test_mirrors_are_present(slz4):
    assert isinstance(slz4.FastCompressStreams.level, property) and hasattr(slz4.FastCompressStreams, "set_level")
    hpp = read("include", "streamly_lz4.hpp")
    cls = hpp.split("class FastCompressStreams {")[1].split("};")[0]
    assert re.search(r"\bvoid\s+setLevel\s*\(\s*int\s+level\s*\)", cls) and re.search(r"\bint\s+level\s*\(\s*\)\s*const", cls)
    cpp = read("streamly-lz4_amd", "csrc", "host_stream.cpp")
    assert "FastCompressStreams::setLevel" in cpp and "mi355lz4_fstreams_set_level(" in cpp
    assert "FastCompressStreams::level" in cpp and "mi355lz4_fstreams_get_level(" in cpp
    shim = read("haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")
    for name in SYMBOLS:
        assert '"mi355lz4.h %s"' % name in shim, name + " is not imported by the Haskell shim"
    assert re.search(r"^setFastStreamsLevel\s*::", shim, re.M) and re.search(r"^\s+, setFastStreamsLevel\s*$", shim, re.M)


def test_haskell_shim_imports_match_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_haskell_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    for name in SYMBOLS:
        assert name in r.stdout, name + " was not among the imports that were checked"


def test_the_set_carries_the_level_and_one_enqueue_branches_on_it():
    eng = read("streamly-lz4_amd", "csrc", "engine.hpp")
    assert re.search(r"struct\s+mi355lz4_fstreams\s*:\s*SlotSet\s*\{[^}]*\bint\s+level\s*=\s*0\s*;", eng)
    api = read("streamly-lz4_amd", "csrc", "api.cpp")
    assert api.count("stream_table_upload(c, fs->table") == 1 and len(re.findall(r"return compress_streams_check\(", api)) == 2
    body = api.split("int mi355lz4_detail::fstreams_enqueue(")[1].split("\nextern \"C\"")[0]
    assert body.index("stream_table_upload(c, fs->table") < body.index("fs->level") < body.index("launch_fstreams_hc(")
    assert "launch_fstreams(x, grid, c->stream)" in body and 'env_int("MI355LZ4_HSTREAMS_GROUPS", 0)' in body
    # the engine's level is refused as before, whatever the set says
    assert "%s: compression level %d; %s streams are level 0's encoder" in api
    kh = read("streamly-lz4_amd", "csrc", "kernels.h")
    assert re.search(r"void\s+launch_fstreams_hc\s*\(\s*const\s+FStreamsArgs\s*&\s*\w*\s*,\s*int\s+grid\s*,\s*int\s+level\s*,\s*hipStream_t", kh)


def test_the_kernel_is_where_the_map_says():
    fam = read("streamly-lz4_amd", "csrc", "kernels.hip")
    assert "k_encode_hc_fstreams" in fam and "kernels_hstreams.hip" in fam
    unit = read("streamly-lz4_amd", "csrc", "kernels_hstreams.hip")
    assert re.search(r"__launch_bounds__\(HC_THREADS\)\s+void\s+k_encode_hc_fstreams\s*\(\s*FStreamsArgs\s+x\s*,\s*int\s+depth\s*\)", unit)
    assert "__shared__ HcLds L;" in unit and "encode_block_hc<false>(L, src, n, dictLen, slot + a.headerKind, depth)" in unit
    assert "wg_copy_pieces(blockAt - dictLen" in unit and unit.index("__syncthreads();") < unit.index("wg_copy_pieces(blockAt - dictLen")
    inc = read("streamly-lz4_amd", "csrc", "kernels", "encode.inc")
    launcher = inc.split("void launch_fstreams_hc(")[1].split("\n}\n")[0]
    assert launcher.index("k_fstreams_plan") < launcher.index("launch_encode_hc_fstreams(") < launcher.index("k_fstreams_save")
    assert "$(CSRC)/kernels_hstreams.hip" in read("Makefile")


def test_header_states_the_contract():
    header = read("include", "mi355lz4.h")
    for words in ("mi355lz4_fstreams_set_level", "a property of the set", "speaks of the ENGINE's level", "0 (the default after _create)",
                  "needs no device and", "enqueues nothing", "a call already enqueued keeps the level", "leaves the level as it was",
                  "accel is ignored", "10..12 search as 9", "the engine at level L", "second block of the contiguous two-block call [D, B_k]",
                  "max(|D|, maxBlockLen)", "neither on how it is cut into calls nor on where its blocks lie",
                  "The level may change between calls of one stream", "group seams included", "MI355LZ4_HSTREAMS_GROUPS"):
        assert words in header, words
    # the sentences of the level-0 contract are as they were
    for words in ("only level 0 accepted", "do not depend on how it is cut into calls", "zero-length array resets a stream's",
                  "LZ4_decompress_safe_continue", "reads no device memory on the host", "An empty stream leaves its slot untouched",
                  "block checksums apply", "profiles/fstreams_rate.json"):
        assert words in header, words
    design = read("DESIGN.md")
    assert "## 7q." in design and "k_encode_hc_fstreams" in design and "mi355lz4_fstreams_set_level" in design
    assert "fstreams_set_level" in read("README.md") and "fstreams_set_level" in read("INTEGRATION.md")
    rates = os.path.exists(os.path.join(ROOT, "profiles", "hstreams_rate.json"))
    for doc in (read("README.md"), design):
        assert ("profiles/hstreams_rate.json" in doc) and (rates or "unmeasured until" in doc)


def test_the_attribute_needs_no_device(slz4):
    L = slz4.lib
    assert L.mi355lz4_fstreams_set_level(None, 3) == E_ARG and b"fstreams_set_level" in L.mi355lz4_last_error()
    assert L.mi355lz4_fstreams_get_level(None) == E_ARG and b"fstreams_get_level" in L.mi355lz4_last_error()


def test_sanitizer_builds_list_the_stub():
    mk = read("Makefile")
    lists = [ln for ln in mk.splitlines() if re.match(r"^[A-Z]*_?SAN_SRCS :=", ln)]
    assert len(lists) >= 10, "the Makefile's *_SAN_SRCS lists: the two host programs and one per family of calls"
    for ln in lists:
        assert "tests/native/san_stubs_hstreams.cpp" in ln, "%s: the new launcher would not link" % ln.split()[0]
    assert re.search(r"^asan-hstreams:", mk, re.M) and re.search(r"^asan:.*\basan-hstreams\b", mk, re.M)
    stub = read("tests", "native", "san_stubs_hstreams.cpp")
    assert "launch_fstreams_hc" in stub and "encode_hc_fstreams_grid" in stub
    main = read("tests", "native", "hstreams_args_main.cpp")
    assert re.search(r"^int main\(\)", main, re.M) and "LD_PRELOAD" not in main + mk


def test_argument_checks_under_sanitizers():
    """the host code of the calls from a program of its own (tests/native/hstreams_args_main.cpp), ASan + UBSan, no device"""
    if shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("g++ or the HIP host headers are not available")
    r = subprocess.run(["make", "-C", ROOT, "asan-hstreams"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "hstreams_args_main ok" in r.stdout
    for bad in ("ERROR: AddressSanitizer", "runtime error:"):
        assert bad not in r.stdout + r.stderr


def test_resource_record():
    rec = read("profiles", "hstreams_kernel_resources.txt")

    def row(name, tag=""):
        m = re.search(r"^%s%s\s+vgpr\s+(\d+) sgpr\s+(\d+) vspill\s+(\d+) sspill\s+(\d+) lds\s+(\d+) scratch\s+(\d+)$"
                      % (tag, re.escape(name)), rec, re.M)
        assert m, tag + name
        return [int(x) for x in m.groups()]
    new = row("_Z20k_encode_hc_fstreams12FStreamsArgsi")
    hc = row("_Z11k_encode_hc10EncodeArgsi", "change  ")
    # 16 waves of one workgroup on a CU's four SIMDs (512 VGPRs / 4), k_encode_hc's LDS -- all of a CU's -- no vector spills, no scratch
    assert new[0] <= 128 and new[2] == 0 and new[4] == hc[4] <= 160 * 1024 and new[5] == 0, new
    for name in ("_Z11k_encode_hc10EncodeArgsi", "_Z16k_encode_hc_dict10HcDictArgsi",
                 "_Z17k_encode_fstreamsILb0EEv12FStreamsArgs", "_Z17k_encode_fstreamsILb1EEv12FStreamsArgs"):
        assert row(name, "change  ") == row(name, "parent  "), name + ": the change moved a kernel it does not edit"
