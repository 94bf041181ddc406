"""The frame writer, the part that needs no GPU: the model the GPU tests compare with (tests/cframes_model.py) rebuilds every
golden liblz4 frame from its own payloads and options byte for byte; mi355lz4_cframes_bound is the formula and covers every
golden frame; the new face is in the header, the library's exports, the Python binding's symbol list and the C++ and Haskell
mirrors; none of its device-pointer calls carries a _device suffix, so the list tests/stream_order.py draws from the header is
what it was; and the argument checks run from a program of their own under ASan + UBSan (make asan-cframes)."""
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import cframes_model as CM  # noqa: E402
import frames_cases as FC  # noqa: E402
import frames_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["mi355lz4_cframes_bound", "mi355lz4_cframes_create", "mi355lz4_cframes_destroy", "mi355lz4_cframes_reserve",
       "mi355lz4_cframes_compress", "mi355lz4_compress_frames"]

# the *_device declarations of the header as the parent commit had them: tests/stream_order.py demands a late-input case for each
DEVICE_CALLS = [
    "mi355lz4_compact_device", "mi355lz4_compress_batch_device", "mi355lz4_compress_dict_device", "mi355lz4_compress_fastdict_device",
    "mi355lz4_compress_fastdict_multi_device", "mi355lz4_compress_hcdict_device", "mi355lz4_compress_pages_device",
    "mi355lz4_compress_pages_fast_device", "mi355lz4_compress_pages_fastdict_device", "mi355lz4_compress_streams_device",
    "mi355lz4_compress_streams_fast_device", "mi355lz4_decoded_size_device", "mi355lz4_decompress_batch_device",
    "mi355lz4_decompress_dict_device", "mi355lz4_decompress_dict_multi_device", "mi355lz4_decompress_dstreams_device",
    "mi355lz4_decompress_partial_device", "mi355lz4_decompress_streams_device", "mi355lz4_generate_device", "mi355lz4_index_device",
    "mi355lz4_interleave_device", "mi355lz4_xxh32_device",
]


def _options(frame):
    """(block size id, flags of the writer) of a parsed liblz4 frame"""
    f = frame
    flags = (0 if f.flg & 0x20 else CM.LINKED) | (CM.BLOCK_CHECKSUM if f.flg & 0x10 else 0) | (CM.CONTENT_SIZE if f.flg & 8 else 0) | \
        (CM.CONTENT_CHECKSUM if f.flg & 4 else 0)
    return (f.bmax.bit_length() - 1 - 8) // 2, flags


def test_model_xxh32_is_the_published_one():
    assert CM.xxh32(b"") == 0x02CC5D05
    assert CM.xxh32(b"a") == 0x550D7456
    assert CM.xxh32(b"Nobody inspects the spammish repetition") == 0xE2293B2F
    assert CM.xxh32(b"a", 1) != CM.xxh32(b"a")
    for n in (3, 4, 15, 16, 17, 31, 32, 33, 255, 4099):
        data = FC.content("random", n, n)
        assert CM.xxh32(data) == M.xxh32(data), n


def test_model_rebuilds_every_golden_frame():
    """a liblz4 frame, taken apart by the decode side's walk and rebuilt from its own payloads and options, is the same bytes"""
    seen_flags, stored, short_middle = set(), 0, 0
    for ident, frame, data in FC.golden():
        frames, err = M.walk(frame)
        assert err is None and len(frames) == 1, ident
        f = frames[0]
        bsid, flags = _options(f)
        blocks, payloads, at = [], [], 0
        for (_p, is_stored, payload, _ck) in f.blocks:
            n = len(payload) if is_stored else M.block_size(payload, f.bmax)
            assert n is not None, ident
            blocks.append(data[at: at + n])
            payloads.append(None if is_stored else payload)
            # liblz4 follows the rule the model states: never a compressed block that is not smaller than its bytes
            assert is_stored or len(payload) < n, ident
            at += n
        assert at == len(data), ident
        cut = CM.cut(data, bsid)
        given = None if [len(b) for b in blocks] == [len(b) for b in cut] else blocks
        short_middle += given is not None
        assert CM.frame(data, bsid, flags, payloads, blocks=given) == frame, ident
        assert len(frame) <= CM.bound(len(data), bsid, flags) or given is not None, ident
        seen_flags.add(flags)
        stored += sum(1 for b in f.blocks if b[1])
    assert seen_flags == set(range(16)) and stored >= 8 and short_middle >= 2


def test_bound_is_the_formula_and_covers_the_golden_frames(slz4):
    import streamly_lz4_amd as S
    for bsid in (4, 5, 6, 7):
        bmax = 1 << (8 + 2 * bsid)
        for flags in range(16):
            for n in (0, 1, 12, 13, bmax - 1, bmax, bmax + 1, 3 * bmax, 3 * bmax + 5, (1 << 40) + 3):
                nb = (n + bmax - 1) // bmax
                want = (15 if flags & 4 else 7) + nb * (8 if flags & 2 else 4) + n + 4 + (4 if flags & 8 else 0)
                assert S.cframes_bound(n, bsid, flags) == want == CM.bound(n, bsid, flags), (bsid, flags, n)
    assert S.cframes_bound(100, 3, 0) == 0 and S.cframes_bound(100, 8, 0) == 0 and S.cframes_bound(100, 4, 16) == 0
    for ident, frame, data in FC.golden():
        f = M.walk(frame)[0][0]
        bsid, flags = _options(f)
        # a frame written with flushes has more blocks than the writer's cut: each costs its word (and its checksum)
        extra = len(f.blocks) - len(CM.cut(data, bsid))
        assert extra >= 0, ident
        assert S.cframes_bound(len(data), bsid, flags) + extra * (8 if flags & 2 else 4) >= len(frame), ident


def test_symbols_everywhere(slz4):
    text = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert not name.endswith("_device")
    assert "typedef struct mi355lz4_cframes mi355lz4_cframes;" in code
    for name, value in (("LINKED", 1), ("BLOCK_CHECKSUM", 2), ("CONTENT_SIZE", 4), ("CONTENT_CHECKSUM", 8)):
        m = re.search(r"#define MI355LZ4_CFRAMES_%s\s+(\d+)u" % name, code)
        assert m and int(m.group(1)) == value == getattr(CM, name), name
    for name, value in (("CAPACITY", CM.E_CAPACITY), ("INPUT", CM.E_INPUT)):
        m = re.search(r"#define MI355LZ4_FRW_E_%s\s+\((-0x[0-9A-Fa-f]+)\)" % name, code)
        assert m and int(m.group(1), 16) == value, name
    codes = [int(v, 16) for v in re.findall(r"#define MI355LZ4_(?:BLK_E|FRM_E|FRW_E|E)_\w+\s+\((-(?:0x)?[0-9A-Fa-f]+)\)", code)]
    assert len(codes) == len(set(codes))
    # the library exports them, the binding declares them
    import streamly_lz4_amd as S
    for name in NEW:
        assert name in S.DECLARED_SYMBOLS and hasattr(S.lib, name), name
    assert (S.FRW_E_CAPACITY, S.FRW_E_INPUT) == (CM.E_CAPACITY, CM.E_INPUT)
    assert (S.CFRAMES_LINKED, S.CFRAMES_BLOCK_CHECKSUM, S.CFRAMES_CONTENT_SIZE, S.CFRAMES_CONTENT_CHECKSUM) == (1, 2, 4, 8)
    assert hasattr(S, "FrameWriter") and hasattr(S.FrameWriter, "reserve") and hasattr(S.FrameWriter, "compress")
    assert hasattr(S.Engine, "compress_frames")
    # the C++ mirror
    hpp = open(os.path.join(ROOT, "include", "streamly_lz4.hpp")).read()
    assert re.search(r"class FrameWriter\b", hpp) and re.search(r"\bcompressFrames\s*\(", hpp)
    impl = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "host_stream.cpp")).read()
    for name in ("mi355lz4_cframes_create", "mi355lz4_cframes_destroy", "mi355lz4_cframes_reserve", "mi355lz4_cframes_compress",
                 "mi355lz4_compress_frames"):
        assert name in impl, name
    # the Haskell mirror
    hs = open(os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")).read()
    for name in NEW:
        assert '"mi355lz4.h %s"' % name in hs, name
    assert re.search(r"^newFrameWriter ::", hs, re.M) and re.search(r"^compressFramesMany ::", hs, re.M)


def test_haskell_ffi_check_still_passes():
    import shutil
    if shutil.which("gcc") is None:
        pytest.skip("gcc is not available")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_haskell_ffi.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "mi355lz4_cframes_compress" in r.stdout and "mi355lz4_compress_frames" in r.stdout


def test_stream_order_device_symbols_are_unchanged():
    """no call of the new face is one tests/stream_order.py demands a late-input case for (that file is not edited)"""
    import stream_order as SO
    assert SO.header_device_symbols() == sorted(DEVICE_CALLS)
    assert not any("frames" in name for name in SO.header_device_symbols())


def test_kernels_are_a_translation_unit_of_their_own():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    m = re.search(r"^SRCS :=(.*)$", mk, re.M)
    assert m and "$(CSRC)/kernels_cframes.hip" in m.group(1) and "$(CSRC)/cframes.cpp" in m.group(1)
    unit = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "kernels.hip")).read()
    assert "cframes" not in re.sub(r"//[^\n]*", "", unit)                   # nothing of it is included into kernels.hip
    src = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "kernels_cframes.hip")).read()
    for k in ("k_cframes_count", "k_cframes_plan", "k_cframes_sizes", "k_cframes_layout", "k_cframes_pack", "k_cframes_head"):
        assert re.search(r"__global__[^\n]*\bvoid %s\(" % k, src), k
    assert "encode_" not in re.sub(r"//[^\n]*", "", src)                    # the new kernels call no encoder


def test_sanitizer_build_is_wired():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    m = re.search(r"^CFRAMES_SAN_SRCS :=(.*)$", mk, re.M)
    assert m and "$(CSRC)/cframes.cpp" in m.group(1) and "tests/native/san_stubs_cframes.cpp" in m.group(1) \
        and "tests/native/cframes_args_main.cpp" in m.group(1)
    assert re.search(r"^asan-cframes:", mk, re.M)
    assert re.search(r"^asan:.*\basan-cframes\b", mk, re.M)
    stubs = open(os.path.join(ROOT, "tests", "native", "san_stubs_cframes.cpp")).read()
    for fn in ("launch_cframes_plan", "launch_cframes_finish", "launch_cframes_gather"):
        assert fn in stubs
    main = open(os.path.join(ROOT, "tests", "native", "cframes_args_main.cpp")).read()
    assert "int main()" in main and "LD_PRELOAD" not in mk.split("CFRAMES_SAN_SRCS")[1].split("asan:")[0]


def test_argument_checks_under_sanitizers():
    """the host code of the calls from a program of its own (tests/native/cframes_args_main.cpp), ASan + UBSan, no device"""
    import shutil
    if shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("g++ or the HIP host headers are not available")
    r = subprocess.run(["make", "-C", ROOT, "asan-cframes"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "cframes_args_main: every argument check holds" in r.stdout
    for bad in ("ERROR: AddressSanitizer", "runtime error:"):
        assert bad not in r.stdout + r.stderr
