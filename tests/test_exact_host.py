"""Reference-exact compression (mi355lz4_set_compress_exact) -- what runs without a GPU: the new symbols in the header,
the Python binding and the library; the null-ctx checks; the Python and C++ mirrors; the Haskell shim's imports of the
setter and the reset against the header."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import check_haskell_ffi as ffi  # noqa: E402
import streamly_lz4_amd as S  # noqa: E402

E_ARG = -3
NEW = ["mi355lz4_set_compress_exact", "mi355lz4_get_compress_exact", "mi355lz4_compress_exact_reset"]
SHIM = os.path.join(ROOT, "haskell-shim", "Streamly", "Internal", "LZ4", "GPU.hs")


def test_new_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    for name in NEW:
        assert name in S.DECLARED_SYMBOLS
        assert name + "(" in hdr
        getattr(S.lib, name)
    assert "int mi355lz4_set_compress_exact(mi355lz4_ctx *ctx, int on);" in hdr
    assert "int mi355lz4_get_compress_exact(const mi355lz4_ctx *ctx);" in hdr
    assert "int mi355lz4_compress_exact_reset(mi355lz4_ctx *ctx);" in hdr
    getattr(S.lib, "mi355lz4_debug_exact_state")      # diagnostics: exported, not in the header
    assert "mi355lz4_debug_exact_state" not in hdr


def test_null_ctx_is_rejected():
    for on in (0, 1):
        assert S.lib.mi355lz4_set_compress_exact(None, on) == E_ARG
    assert S.lib.mi355lz4_get_compress_exact(None) == E_ARG
    assert S.lib.mi355lz4_compress_exact_reset(None) == E_ARG
    assert "null ctx" in S.lib.mi355lz4_last_error().decode()


def test_python_and_cpp_mirrors_exist():
    assert callable(getattr(S.Engine, "set_compress_exact"))
    assert callable(getattr(S.Engine, "reset_compress_stream"))
    assert isinstance(S.Engine.__dict__["compress_exact"], property)
    hpp = open(os.path.join(ROOT, "include", "streamly_lz4.hpp")).read()
    for decl in ("void setCompressExact(bool on);", "bool compressExact() const;", "void resetCompressStream();"):
        assert decl in hpp
    src = open(os.path.join(ROOT, "streamly-lz4_amd", "csrc", "host_stream.cpp")).read()
    assert "void Engine::setCompressExact(bool on)" in src and "void Engine::resetCompressStream()" in src
    # compressChunks starts a new stream when it starts
    assert "if (eng_.compressExact()) eng_.resetCompressStream();" in src


def test_haskell_shim_binds_the_setter_and_reset():
    rc, msg = ffi.check(SHIM, os.path.join(ROOT, "include"))
    assert rc == 0, msg
    names = [c for _h, c, *_ in ffi.parse_imports(open(SHIM).read())]
    assert "mi355lz4_set_compress_exact" in names
    assert "mi355lz4_compress_exact_reset" in names
    assert "mi355lz4_get_compress_exact" in names
    text = open(SHIM).read()
    assert "setCompressExact ::" in text and "resetCompressStream ::" in text
    # compressChunksGPU starts a new exact stream, as the C++ and Python compressChunks do
    assert "    . startExactStream eng\n" in text


def test_canonical_table_equality_is_sufficient():
    """The speculation's premise, on the oracle: wherever a run-in from a zeroed table reaches the true table up to the
    canonicalisation (entries below currentOffset - 65536 read 0), the next block's bytes are the true stream's."""
    import exact_runin_sim as sim
    for kind in ("text", "pysrc", "lzsynth"):
        res = sim.run(kind, 40, 65536, [1, 3, 8], 16)
        for r in res.values():
            assert r["bytes_equal_where_tables_equal"] in (None, 1.0)
        assert res["8"]["tables_equal"] > 0
    assert sim.run("text", 24, 65536, [1, 2], 8)["1"]["tables_equal"] == 0.0     # R = 1 on text fails: the repair path
