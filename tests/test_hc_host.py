"""Compression levels (mi355lz4_set_compression_level / _get_compression_level) -- what runs without a GPU: the new
symbols in the header, the Python binding and the library; the argument checks that need no engine; the Haskell shim's
import of the setter against the header."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import check_haskell_ffi as ffi  # noqa: E402
import streamly_lz4_amd as S  # noqa: E402

E_ARG = -3
NEW = ["mi355lz4_set_compression_level", "mi355lz4_get_compression_level"]
SHIM = os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")


def test_new_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    for name in NEW:
        assert name in S.DECLARED_SYMBOLS
        assert name + "(" in hdr
        getattr(S.lib, name)
    assert "int mi355lz4_set_compression_level(mi355lz4_ctx *ctx, int level);" in hdr
    assert "int mi355lz4_get_compression_level(const mi355lz4_ctx *ctx);" in hdr


def test_null_ctx_and_bad_levels_are_rejected():
    for level in (-100, -1, 0, 1, 9, 12, 13, 1000):
        assert S.lib.mi355lz4_set_compression_level(None, level) == E_ARG
    assert S.lib.mi355lz4_get_compression_level(None) == E_ARG
    assert "null ctx" in S.lib.mi355lz4_last_error().decode()


def test_python_mirrors_exist():
    assert callable(getattr(S.Engine, "set_compression_level"))
    assert isinstance(S.Engine.__dict__["compression_level"], property)
    assert callable(getattr(S.MultiEngine, "set_compression_level"))


def test_haskell_shim_binds_the_setter():
    rc, msg = ffi.check(SHIM, os.path.join(ROOT, "include"))
    assert rc == 0, msg
    names = [c for _h, c, *_ in ffi.parse_imports(open(SHIM).read())]
    assert "mi355lz4_set_compression_level" in names
    assert "setCompressionLevel ::" in open(SHIM).read()
