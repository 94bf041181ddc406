"""The decode streams' surface without a GPU: the symbols are declared, listed and exported, the argument checks that need no
device return MI355LZ4_E_ARG, the Haskell shim's imports match the header, and the tests' stream writer is frame_compress's."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dstreams_model as M  # noqa: E402

E_ARG = -3
SYMBOLS = ["mi355lz4_dstreams_create", "mi355lz4_dstreams_destroy", "mi355lz4_dstreams_count", "mi355lz4_dstreams_reset",
           "mi355lz4_dstreams_set_dict", "mi355lz4_decompress_dstreams_device", "mi355lz4_decompress_dstreams"]
_i32p = C.POINTER(C.c_int32)


def test_symbols_declared_listed_and_exported(slz4):
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in include/mi355lz4.h"
        assert name in slz4.DECLARED_SYMBOLS, name
        assert getattr(slz4.lib, name).argtypes is not None, name + " has no sig() declaration"
    assert "typedef struct mi355lz4_dstreams mi355lz4_dstreams;" in header
    for cls in ("DecompressStreams",):
        assert cls in slz4.__all__ and hasattr(slz4, cls)
    for m in ("decompress_dstreams_device", "decompress_dstreams"):
        assert hasattr(slz4.Engine, m)
    for m in ("reset", "set_dict", "close", "__len__"):
        assert hasattr(slz4.DecompressStreams, m)


def test_header_states_size_limit_and_confinement():
    header = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    kernels_h = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "kernels.h")).read()
    assert "65600 bytes" in header and "DSTREAM_SLOT_BYTES (DSTREAM_COUNT_OFF + 64)" in kernels_h
    assert "One wavefront walks one stream" in header and "_decompress_dstreams_device" in header.split("engine lifecycle")[0]
    assert "unmeasured until scripts/dstreams_rate.py has written" in header


def test_null_and_table_checks_need_no_device(slz4):
    L = slz4.lib
    one = (C.c_int32 * 2)(0, 0)
    sz, nb = C.c_size_t(7), C.c_int(7)
    out = C.c_void_p()
    assert L.mi355lz4_dstreams_create(None, 4, C.byref(out)) == E_ARG and not out.value
    assert L.mi355lz4_dstreams_count(None) == E_ARG
    assert L.mi355lz4_dstreams_reset(None, None, None, 0) == E_ARG
    assert L.mi355lz4_dstreams_set_dict(None, None, 0, None, 0) == E_ARG
    L.mi355lz4_dstreams_destroy(None)
    assert L.mi355lz4_decompress_dstreams_device(None, None, None, 0, None, 0, 8, 0, one, one, 1, None, None, None, None) == E_ARG
    assert b"decompress_dstreams_device" in L.mi355lz4_last_error()
    assert L.mi355lz4_decompress_dstreams(None, None, None, 0, 8, 0, one, one, 1, None, 0, C.byref(sz), None, 0, C.byref(nb)) == E_ARG
    assert sz.value == 0 and nb.value == 0
    assert b"decompress_dstreams" in L.mi355lz4_last_error()


def test_haskell_shim_imports_match_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_haskell_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    shim = open(os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")).read()
    for name in SYMBOLS:
        assert '"%s"' % name in shim or name in shim, name + " is not imported by the Haskell shim"
    assert "decompressChunksMany" in shim


def test_stream_writer_is_frame_compress(oracle):
    """linked_stream's call sequence for ragged arrays writes what Oracle.frame_compress(linked=True) writes"""
    buf = M.data(oracle, "text", 5 * 4096 + 100)
    arrays = M.cut(buf, [4096] * 5 + [100])
    assert M.linked_stream(oracle, arrays, ragged=True) == M.linked_stream(oracle, arrays)
    st = [M.good_block(c, len(a), 8) for c, a in zip(M.linked_stream(oracle, arrays), arrays)]
    M.assert_dependent(oracle, st)
    codes, outs, prev = M.model(oracle, st)
    assert codes == [len(a) for a in arrays] and outs == arrays and prev == arrays[-1]


def test_model_inputs_hold_on_the_cpu(oracle):
    """what every GPU test asserts first: the streams decode under the model and every block after a first one needs its dictionary"""
    for kind in (8, 4):
        streams, arrays = M.cut_streams(oracle, kind)
        for st, a in zip(streams, arrays):
            M.assert_dependent(oracle, st)
            assert M.model(oracle, st)[1] == a
    st, arrays = M.failing_stream(oracle, 8)
    codes = M.model(oracle, st)[0]
    assert codes[:2] == [4096, 4096] and -0x7F000000 < codes[2] < 0 and codes[3:] == [0, M.BLK_E_COMPLEN, 4096]
