"""Block checksums (mi355lz4_set_block_checksum, Config.hs setBlockChecksum) -- what runs without a GPU: the new symbols,
the slot stride with a trailer, and the host walk of header chains whose blocks carry a 4-byte xxh32 trailer."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import streamly_lz4_amd as S  # noqa: E402

E_ARG, E_STREAM = -3, -6
NEW = ["mi355lz4_set_block_checksum", "mi355lz4_slot_stride_ex", "mi355lz4_index_host_ex", "mi355lz4_xxh32_device"]


def _chain(blocks, hk, ck):
    """A framed stream built in Python: [compLen][uncompLen (hk 8)][data][xxh32(data) when ck]."""
    out = b""
    for data, ulen in blocks:
        out += struct.pack("<i", len(data)) + (struct.pack("<i", ulen) if hk == 8 else b"") + data
        if ck:
            out += struct.pack("<I", S.xxh32(data))
    return out


def test_new_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    for name in NEW:
        assert name in S.DECLARED_SYMBOLS
        assert name + "(" in hdr
        getattr(S.lib, name)
    assert "MI355LZ4_BLK_E_CHECKSUM (-0x7F000004)" in hdr


def test_new_calls_without_an_engine_fail_cleanly():
    assert S.lib.mi355lz4_set_block_checksum(None, 1) == E_ARG
    assert S.lib.mi355lz4_xxh32_device(None, None, None, None, 1, 0, None) == E_ARG
    if S.device_count() == 0:
        h = C.c_void_p()
        assert S.lib.mi355lz4_create(C.byref(h), 0) == -1          # MI355LZ4_E_NO_DEVICE: no CPU path


@pytest.mark.parametrize("n", [0, 1, 15, 16, 65536, 4 << 20])
@pytest.mark.parametrize("hk", [4, 8])
def test_slot_stride_ex(n, hk):
    assert S.slot_stride_ex(n, hk, False) == S.slot_stride(n, hk)
    b = S.compress_bound(n) + hk + 4
    assert S.slot_stride_ex(n, hk, True) == (b + 15) & ~15
    assert S.slot_stride_ex(n, hk, True) % 16 == 0


@pytest.mark.parametrize("hk", [4, 8])
def test_index_host_ex_walks_trailers(hk):
    rng = np.random.default_rng(7)
    blocks = [(rng.integers(0, 256, size=int(L), dtype=np.uint8).tobytes(), int(L) * 3)
              for L in (1, 5, 16, 300, 4096, 2)]
    fixed = 65536
    framed = _chain(blocks, hk, True)
    boff, ulen = S.index_host(framed, hk, fixed, block_checksum=True)
    want, pos = [], 0
    for data, _ in blocks:
        want.append(pos)
        pos += hk + len(data) + 4
    assert boff == want and pos == len(framed)
    assert ulen == ([u for _, u in blocks] if hk == 8 else [fixed] * len(blocks))
    # the same chain without trailers walks as before, with both functions
    plain = _chain(blocks, hk, False)
    assert S.index_host(plain, hk, fixed, block_checksum=False)[0] == [o - 4 * i for i, o in enumerate(want)]
    # read as a chain without trailers, the trailered stream is malformed
    with pytest.raises(S.LZ4Error):
        S.index_host(framed, hk, fixed, block_checksum=False)


@pytest.mark.parametrize("cut", [1, 2, 3, 4])
@pytest.mark.parametrize("hk", [4, 8])
def test_index_host_ex_short_last_trailer(hk, cut):
    blocks = [(b"abcdefgh" * 5, 40), (b"0123456789", 10)]
    framed = _chain(blocks, hk, True)[:-cut]
    src = np.frombuffer(framed, dtype=np.uint8)
    boff = np.zeros(8, dtype=np.uint64)
    ulen = np.zeros(8, dtype=np.int32)
    nb = C.c_int()
    rc = S.lib.mi355lz4_index_host_ex(src.ctypes.data_as(C.POINTER(C.c_uint8)), src.size, hk, 0, 1,
                                      boff.ctypes.data_as(C.POINTER(C.c_uint64)), ulen.ctypes.data_as(C.POINTER(C.c_int32)),
                                      8, C.byref(nb))
    assert rc == E_STREAM
    assert b"incomplete block 1" in S.lib.mi355lz4_last_error()
    # the unchanged function reads the cut stream without trailers: a different chain, also malformed here or not --
    # but never one that ends in the middle of block 1's trailer
    rc0 = S.lib.mi355lz4_index_host(src.ctypes.data_as(C.POINTER(C.c_uint8)), src.size, hk, 0,
                                    boff.ctypes.data_as(C.POINTER(C.c_uint64)), ulen.ctypes.data_as(C.POINTER(C.c_int32)),
                                    8, C.byref(nb))
    assert rc0 in (0, E_STREAM)


# ---- the C++ mirror's resizeChunks with setBlockChecksum True (host only) ---------------------------------------
def _rechunk(stream, size):
    return [stream[i:i + size] for i in range(0, len(stream), size)]


@pytest.mark.parametrize("size", [1, 512, 32 << 10, 256 << 10])
@pytest.mark.parametrize("bs", [S.BlockSize.BlockHasSize, S.BlockSize.BlockMax64KB])
def test_resize_chunks_with_trailers(bs, size):
    rng = np.random.default_rng(size)
    hk = 8 if bs == S.BlockSize.BlockHasSize else 4
    # blocks of every size class, the last ones small, so that headers and trailers straddle the rechunked arrays
    lens = [1, 3, 4, 5, 17, 511, 513, 40000, 70000, 131071, 2, 9]
    blocks = [(rng.integers(0, 256, size=L, dtype=np.uint8).tobytes(), L * 2) for L in lens]
    want = [_chain([b], hk, True) for b in blocks]
    stream = b"".join(want)
    cfg = S.setBlockChecksum(True, S.BlockConfig(bs))
    assert cfg.blockChecksum and S.setBlockMaxSize(bs, cfg).blockChecksum
    got = S.resizeChunks(cfg, S.defaultFrameConfig, _rechunk(stream, size))
    assert got == want
    # without the switch the trailer is read as the next block's header: not the same blocks, or a malformed stream
    try:
        assert S.resizeChunks(S.BlockConfig(bs), S.defaultFrameConfig, _rechunk(stream, size)) != want
    except S.LZ4Error:
        pass


def test_resize_chunks_incomplete_trailer():
    cfg = S.setBlockChecksum(True, S.BlockConfig(S.BlockSize.BlockMax64KB))
    stream = _chain([(b"x" * 100, 0)], 4, True)
    with pytest.raises(S.LZ4Error, match="Incomplete block"):
        S.resizeChunks(cfg, S.defaultFrameConfig, _rechunk(stream[:-1], 7))
