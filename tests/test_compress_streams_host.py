"""The many-streams compress API without a GPU: the symbols are declared, exported and bound, the Haskell imports agree with the
header, and the argument checks that need no device answer MI355LZ4_E_ARG."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

E_ARG = -3
PUBLIC = ["mi355lz4_cstreams_create", "mi355lz4_cstreams_destroy", "mi355lz4_cstreams_count", "mi355lz4_cstreams_reset",
          "mi355lz4_compress_streams_device", "mi355lz4_compress_streams"]
HOOK = "mi355lz4_debug_cstream_state"


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", "mi355lz4.h")).read()


def test_declared_in_the_header(header):
    for name in PUBLIC:
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert "typedef struct mi355lz4_cstreams mi355lz4_cstreams;" in header
    assert HOOK not in header                                   # a diagnostic hook, like mi355lz4_debug_exact_state
    assert "80 KiB a slot" in header


def test_exported_and_bound(slz4):
    for name in PUBLIC + [HOOK]:
        assert getattr(slz4.lib, name).argtypes is not None, name
    for name in PUBLIC:
        assert name in slz4.DECLARED_SYMBOLS
    assert {"reset", "close", "state"} <= set(dir(slz4.CompressStreams))
    assert hasattr(slz4.Engine, "compress_streams_device") and hasattr(slz4.Engine, "compress_streams")
    assert "CompressStreams" in slz4.__all__


def test_haskell_imports_agree():
    shim = open(os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")).read()
    for name in PUBLIC:
        assert '"mi355lz4.h %s"' % name in shim, name
    assert "compressChunksMany" in shim
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_haskell_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in PUBLIC:
        assert name in r.stdout


def test_cxx_mirror_declares_it():
    hpp = open(os.path.join(ROOT, "include", "streamly_lz4.hpp")).read()
    assert "class CompressStreams" in hpp and "compressStreams" in hpp


def test_null_arguments(slz4):
    L = slz4.lib
    h = C.c_void_p()
    assert L.mi355lz4_cstreams_create(None, 4, C.byref(h)) == E_ARG and not h
    assert L.mi355lz4_cstreams_create(None, 4, None) == E_ARG
    assert L.mi355lz4_cstreams_count(None) == E_ARG
    assert L.mi355lz4_cstreams_reset(None, None, None, 0) == E_ARG
    L.mi355lz4_cstreams_destroy(None)
    sf = (C.c_int32 * 2)(0, 1)
    sl = (C.c_int32 * 1)(0)
    assert L.mi355lz4_compress_streams_device(None, None, None, None, None, 0, 16, 1, sf, sl, 1, 1, 8, None, 64, None) == E_ARG
    n = C.c_size_t(5)
    assert L.mi355lz4_compress_streams(None, None, None, None, 1, sf, sl, 1, 1, 8, None, 0, C.byref(n), None, None) == E_ARG
    assert n.value == 0
    assert L.mi355lz4_debug_cstream_state(None, 0, None, None) == E_ARG
    assert b"null" in L.mi355lz4_last_error() or b"bad" in L.mi355lz4_last_error()
