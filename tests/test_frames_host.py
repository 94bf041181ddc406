"""Batches of standard LZ4 frames, the part that needs no GPU: the model the GPU tests compare with (tests/frames_model.py) is
held to the golden contents, to the named code of every corruption and, where the system liblz4 loads, to LZ4F_decompress; the
new face is in the header, in the Python binding's symbol list and in the Haskell shim's check, and none of its device-pointer
calls carries a _device suffix (tests/stream_order.py lists those)."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import frames_cases as FC  # noqa: E402
import frames_model as M  # noqa: E402
import lz4f  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = lz4f.load()

NEW = ["mi355lz4_frames_create", "mi355lz4_frames_destroy", "mi355lz4_frames_load", "mi355lz4_frames_inputs", "mi355lz4_frames_blocks",
       "mi355lz4_frames_total", "mi355lz4_frames_sizes", "mi355lz4_frames_get_sizes", "mi355lz4_frames_decode",
       "mi355lz4_decompress_frames"]


def test_xxh32_known_values():
    assert M.xxh32(b"") == 0x02CC5D05
    assert M.xxh32(b"a") == 0x550D7456
    assert M.xxh32(b"Nobody inspects the spammish repetition") == 0xE2293B2F


def test_golden_covers_the_options():
    ids = [g[0] for g in FC.golden()]
    assert len(ids) == len(set(ids)) == len(FC.golden_specs())
    for n in (0, 1, 12, 13, 65535, 65536, 65537, 3 * 65536 + 5):
        for tag in ("-L", "-I", "B", "C", "S", "-l0-", "-l9-", "-frame", "-pieces"):
            assert any(i.startswith("text%d-" % n) and tag in i[len("text%d" % n):] for i in ids), (n, tag)
    assert any(i.startswith("random70000") for i in ids) and any("-b7-L" in i for i in ids) and any("-b7-I" in i for i in ids)
    assert os.path.getsize(FC.GOLDEN) <= max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f))
                                             for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f != "frames_vectors.json")


def test_model_reads_every_golden_frame(oracle):
    stored = 0
    for ident, frame, data in FC.golden():
        size, result, out = M.model(frame, oracle)
        assert (size, result) == (len(data), len(data)) and out == data, ident
        stored += sum(1 for f in M.walk(frame)[0] for b in f.blocks if b[1])
    assert stored >= 8                                  # the random contents came out as stored blocks


def test_model_on_hand_built_frames(oracle):
    for name, frame, data in FC.valid_cases(oracle):
        size, result, out = M.model(frame, oracle)
        assert (size, result, out) == (len(data), len(data), data), name
        if L is not None:
            assert lz4f.decompress(L, frame, len(data) + 16) == data, name


def test_the_dropped_clause_is_the_only_difference():
    """The block that is one long match from the window, ending 5 bytes before its end: the decoded-size rule of the engine's
    own blocks refuses it (rule 4's last clause), a frame's rule gives its size."""
    import lz4_synth as Z
    import size_model
    blk = Z.write_block([(b"", 350, 300)], last_literals=b"5last")
    assert size_model.model_size(blk, 65536) == size_model.UNKNOWN
    assert M.block_size(blk, 65536) == 305


def test_model_names_every_corruption(oracle):
    seen = set()
    for name, frame, code in FC.corrupt_cases(oracle):
        size, result, out = M.model(frame, oracle)
        assert result < 0 and out is None, name
        if code is not None:
            assert result == code, (name, M.NAMES.get(result), M.NAMES[code])
        # what is known at load is reported at load; BLOCK from decoding and CONTENT_CHECKSUM only by the decode
        assert size == result or (size >= 0 and result in (M.E_BLOCK, M.E_CONTENT_CHECKSUM)), name
        seen.add(result)
    assert seen == set(M.NAMES)


def test_skip_flags_in_the_model(oracle):
    for name, frame, code in FC.corrupt_cases(oracle):
        size, result, _ = M.model(frame, oracle, M.SKIP_CONTENT_CHECKSUM | M.SKIP_BLOCK_CHECKSUM)
        if name in ("block-checksum-flipped", "content-checksum-flipped", "data-byte-flipped-stored"):
            assert result >= 0, name
        elif code is not None and code not in (M.E_BLOCK_CHECKSUM, M.E_CONTENT_CHECKSUM):
            assert result == code, name
    # the fields must still be there
    assert M.model(dict((n, f) for n, f, _ in FC.corrupt_cases(oracle))["cut-in-content-checksum"], oracle, 3)[1] == M.E_TRUNCATED


def test_symbols_everywhere():
    text = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert not name.endswith("_device")
    assert "typedef struct mi355lz4_frames mi355lz4_frames;" in code
    for k, name in enumerate(("MAGIC", "HEADER", "HEADER_CHECKSUM", "TRUNCATED", "BLOCK_SIZE", "BLOCK_CHECKSUM", "BLOCK", "CONTENT_SIZE",
                              "CONTENT_CHECKSUM"), 1):
        m = re.search(r"#define MI355LZ4_FRM_E_%s\s+\((-0x[0-9A-Fa-f]+)\)" % name, code)
        assert m and int(m.group(1), 16) == -0x7F000100 - k == getattr(M, "E_" + name)
    codes = [int(v, 16) for v in re.findall(r"#define MI355LZ4_(?:BLK_E|FRM_E|E)_\w+\s+\((-(?:0x)?[0-9A-Fa-f]+)\)", code)]
    assert len(codes) == len(set(codes))
    # no function of the new face is one of the calls tests/stream_order.py demands a late-input case for
    device_calls = re.findall(r"int\s+(mi355lz4_\w*_device)\s*\(", code)
    assert device_calls and not any("frames" in d for d in device_calls)


def test_python_binding_declares_them():
    import streamly_lz4_amd as S
    for name in NEW:
        assert name in S.DECLARED_SYMBOLS and hasattr(S.lib, name), name
    assert (S.FRM_E_MAGIC, S.FRM_E_CONTENT_CHECKSUM) == (M.E_MAGIC, M.E_CONTENT_CHECKSUM)
    assert hasattr(S, "Frames") and hasattr(S.Engine, "decompress_frames")


def test_sanitizer_build_is_wired():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    m = re.search(r"^FRAMES_SAN_SRCS :=(.*)$", mk, re.M)
    assert m and "$(CSRC)/frames.cpp" in m.group(1) and "tests/native/san_stubs_frames.cpp" in m.group(1) \
        and "tests/native/frames_args_main.cpp" in m.group(1)
    assert re.search(r"^asan-frames:", mk, re.M)
    stubs = open(os.path.join(ROOT, "tests", "native", "san_stubs_frames.cpp")).read()
    for fn in ("launch_frames_scan", "launch_frames_load", "launch_frames_place", "launch_frames_decode"):
        assert fn in stubs
    assert "int main()" in open(os.path.join(ROOT, "tests", "native", "frames_args_main.cpp")).read()


def test_argument_checks_under_sanitizers():
    """the host code of the calls from a program of its own (tests/native/frames_args_main.cpp), ASan + UBSan, no device"""
    import shutil
    import subprocess
    if shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("g++ or the HIP host headers are not available")
    r = subprocess.run(["make", "-C", ROOT, "asan-frames"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "frames_args_main: every argument check holds" in r.stdout
    for bad in ("ERROR: AddressSanitizer", "runtime error:"):
        assert bad not in r.stdout + r.stderr
