"""Many reference-exact compress streams in one call (mi355lz4_cstreams, mi355lz4_compress_streams_device / _streams).
Every stream of a call continues its own slot of device-resident state; its blocks must be the bytes of ONE oracle compress
stream (orc_cstream_init once, orc_compress_fast_continue per array, each array its own allocation) -- whatever else shares
the call, however the stream is cut into calls, and through the 2 GiB renormalisation."""
import ctypes as C
import glob
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from conftest import DECODERS  # noqa: E402
from oracle.oracle import Oracle, build as oracle_build  # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG = -3
_u8p = C.POINTER(C.c_uint8)
ORC_CURRENT_OFFSET = 16384          # oracle/lz4_oracle.h, orc_cstream: uint32 table[4096]; uint32 currentOffset; ptr dict; uint32 dictSize
ORC_DICT_SIZE = 16400


class OracleStream:
    """orc_cstream over separately allocated arrays: the reference's compressChunksD call sequence."""

    def __init__(self):
        self.lib = C.CDLL(oracle_build(), mode=os.RTLD_LOCAL)
        self.lib.orc_compress_fast_continue.restype = C.c_int
        self.lib.orc_compress_fast_continue.argtypes = [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int]
        self.lib.orc_compress_bound.restype = C.c_int
        self.lib.orc_compress_bound.argtypes = [C.c_int]
        self.lib.orc_debug_renorms.restype = C.c_long
        self.reset()

    def reset(self):
        self.st = C.create_string_buffer(16384 + 256)
        self.lib.orc_cstream_init(self.st)
        self.keep = []

    def compress(self, arrays, accel=1):
        if accel < 0:
            accel = 0
        out = []
        for a in arrays:
            src = np.zeros(len(a) + 64, dtype=np.uint8)  # its own allocation, readable slack behind it
            src[: len(a)] = np.frombuffer(bytes(a), dtype=np.uint8)
            cap = self.lib.orc_compress_bound(len(a))
            dst = np.zeros(cap + 64, dtype=np.uint8)
            r = self.lib.orc_compress_fast_continue(self.st, src.ctypes.data_as(_u8p), dst.ctypes.data_as(_u8p), len(a),
                                                    cap, int(accel))
            assert r > 0
            out.append(dst[:r].tobytes())
            self.keep = self.keep[-1:] + [src]      # the previous array stays alive: it is the dictionary
        return out

    def scalars(self):
        return (struct.unpack_from("<I", self.st, ORC_CURRENT_OFFSET)[0], struct.unpack_from("<I", self.st, ORC_DICT_SIZE)[0])

    def poke_current_offset(self, v):
        struct.pack_into("<I", self.st, ORC_CURRENT_OFFSET, v)


def frame_block(comp, array, kind, checksum=False):
    """The engine's framing of one block: | compLen | uncompLen (kind 8) | data | xxh32 (checksums) |."""
    import streamly_lz4_amd as S
    out = bytearray(len(comp).to_bytes(4, "little"))
    if kind == 8:
        out += len(array).to_bytes(4, "little")
    out += comp
    if checksum:
        out += int(S.lib.slz4_xxh32(np.frombuffer(comp, dtype=np.uint8).ctypes.data_as(_u8p), len(comp), 0)).to_bytes(4, "little")
    return bytes(out)


def framed_by(ostream, arrays, accel=1, kind=8, checksum=False):
    return [frame_block(c, a, kind, checksum) for c, a in zip(ostream.compress(arrays, accel), arrays)]


_ORC = None


def orc():
    global _ORC
    if _ORC is None:
        _ORC = Oracle()
    return _ORC


_DATA = {}


def data(kind, nbytes, first=0):
    key = (kind, nbytes, first)
    if key not in _DATA:
        if kind == "pysrc":
            buf = bytearray()
            for f in sorted(glob.glob(os.path.join(os.path.dirname(os.__file__), "*.py"))):
                buf += open(f, "rb").read()
                if len(buf) >= nbytes + first:
                    break
            while len(buf) < nbytes + first:
                buf = buf + buf
            _DATA[key] = bytes(buf[first:first + nbytes])
        else:
            _DATA[key] = orc().gen("text", 1, nbytes, first_block=first).tobytes()
    return _DATA[key]


# 9 streams, ragged: an empty one, a one-block one, one whose first array is 0 bytes, a 1 MiB block, last arrays shorter
# than 64 KiB, longer than 64 KiB and of 0 bytes
STREAM_LENS = [
    [],
    [65536],
    [0, 13, 65537],
    [1, 3, 4, 5, 12, 4095],
    [200000, 65535, 0, 12],
    [1 << 20, 4095],
    [65536, 65536, 200000],
    [4095, 0],
    [5, 65537, 13, 1, 65535, 4],
]


def cut(raw, lens):
    out, p = [], 0
    for n in lens:
        out.append(raw[p:p + n])
        p += n
    return out


_STREAMS = None


def ragged_streams():
    """text for the odd streams, Python sources for the even ones; computed once, never changed"""
    global _STREAMS
    if _STREAMS is None:
        _STREAMS = [cut(data("text" if s % 2 else "pysrc", sum(lens) + 16, first=3 + s), lens) for s, lens in enumerate(STREAM_LENS)]
    return _STREAMS


_EXPECT = {}


def expect(accel=1, kind=8, checksum=False):
    """the oracle's framed blocks of ragged_streams(), one oracle stream per stream"""
    key = (max(1, min(accel, 65537)), kind, checksum)
    if key not in _EXPECT:
        _EXPECT[key] = [framed_by(OracleStream(), st, accel, kind, checksum) for st in ragged_streams()]
    return _EXPECT[key]


def run_device(eng, cs, streams, slots=None, accel=1, kind=8, gap=37, bad=None, scribble=True):
    """One compress_streams_device call, the arrays separated by `gap` bytes.  bad = {block index: length} overrides srcLen.
    Returns (per stream, the framed bytes of its blocks; framedLen of all blocks)."""
    import torch
    import streamly_lz4_amd as S
    blocks = [b for st in streams for b in st]
    n = len(blocks)
    sf = np.cumsum([0] + [len(st) for st in streams]).astype(np.int32)
    slots = list(range(len(streams))) if slots is None else slots
    offs, p = [], 0
    for a in blocks:
        offs.append(p)
        p += len(a) + gap
    buf = np.zeros(p + 16, dtype=np.uint8)
    for o, a in zip(offs, blocks):
        buf[o:o + len(a)] = np.frombuffer(bytes(a), dtype=np.uint8)
    mx = max([len(a) for a in blocks] + [0])
    lens = [len(a) for a in blocks]
    for k, v in (bad or {}).items():
        lens[k] = v
    stride = S.slot_stride_ex(mx, kind, eng._block_checksum)
    src = torch.from_numpy(buf).cuda()
    off = torch.tensor(offs + [0], dtype=torch.int64).cuda()
    ln = torch.tensor(lens + [0], dtype=torch.int32).cuda()
    out = torch.zeros(max(n, 1) * stride, dtype=torch.uint8).cuda()
    flen = torch.full((max(n, 1),), -7, dtype=torch.int32).cuda()
    eng.compress_streams_device(cs, src, n, mx, sf, slots, out, stride, flen, accel=accel, header_kind=kind, src_off=off,
                                src_len=ln, block_stride=0)
    torch.cuda.synchronize()
    if scribble:                                     # the call has run: its source is the caller's again
        src.fill_(0xA5)
        torch.cuda.synchronize()
    sl = out.cpu().numpy()
    fl = flen.cpu().tolist()[:n]
    per = [[sl[i * stride:i * stride + fl[i]].tobytes() for i in range(sf[s], sf[s + 1])] for s in range(len(streams))]
    return per, fl


def run_host(eng, cs, streams, slots=None, accel=1, kind=8):
    framed, fl = eng.compress_streams(streams, cs, slots=slots, accel=accel, header_kind=kind)
    assert sum(fl) == len(framed)
    per, p, k = [], 0, 0
    for st in streams:
        row = []
        for _ in st:
            row.append(framed[p:p + fl[k]])
            p += fl[k]
            k += 1
        per.append(row)
    return per, fl


@pytest.fixture
def eng():
    import streamly_lz4_amd as S
    e = S.Engine(0)
    yield e
    e.close()


@pytest.fixture
def cs9(eng):
    import streamly_lz4_amd as S
    cs = S.CompressStreams(eng, len(STREAM_LENS))
    yield cs
    cs.close()


# ---- 1. byte equality -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [4, 8])
@pytest.mark.parametrize("checksum", [False, True])
def test_header_kinds_and_checksums(eng, cs9, kind, checksum):
    eng.set_block_checksum(checksum)
    want = expect(1, kind, checksum)
    got, fl = run_device(eng, cs9, ragged_streams(), kind=kind)
    assert got == want
    assert fl == [len(b) for st in want for b in st]
    cs9.reset()
    got, _ = run_host(eng, cs9, ragged_streams(), kind=kind)
    assert got == want


@pytest.mark.parametrize("accel", [-3, 1, 9, 10 ** 6])
def test_accel(eng, cs9, accel):
    want = expect(accel)
    if accel == 9:
        assert want != expect(1)
    assert run_device(eng, cs9, ragged_streams(), accel=accel)[0] == want
    cs9.reset()
    assert run_host(eng, cs9, ragged_streams(), accel=accel)[0] == want


def test_state_after_a_call(eng, cs9):
    """currentOffset, dictSize, saved bytes: the sum of the lengths, the last array's length, its last min(n, 64 KiB)"""
    assert len(cs9) == len(STREAM_LENS)
    run_device(eng, cs9, ragged_streams())
    for s, lens in enumerate(STREAM_LENS):
        assert cs9.state(s) == ((sum(lens), lens[-1], min(lens[-1], 65536)) if lens else (0, 0, 0)), s


# ---- 2. continuation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_call", [1, 2])
@pytest.mark.parametrize("host", [False, True])
def test_calls_continue_the_slots(eng, cs9, per_call, host):
    """the streams fed per_call blocks at a time, in changing order, some calls naming only some of the slots, every call's
    source scribbled over once it has run"""
    streams = ragged_streams()
    want = expect(1)
    got = [[] for _ in streams]
    pos = [0] * len(streams)
    rnd = 0
    while any(pos[s] < len(st) for s, st in enumerate(streams)):
        order = [s for s in range(len(streams)) if pos[s] < len(streams[s]) or s % 4 == 0]     # (finished ones come along empty)
        if rnd % 3 == 1 and len(order) > 3:
            order = [s for s in order if s % 3 != 0]                                              # a subset of the slots
        order = order[::-1] if rnd % 2 else order[rnd % len(order):] + order[:rnd % len(order)]
        part = [streams[s][pos[s]:pos[s] + per_call] for s in order]
        before = {s: cs9.state(s) for s in range(len(streams)) if s not in order or not part[order.index(s)]}
        per, _ = (run_host if host else run_device)(eng, cs9, part, slots=order)
        for s, blocks, fed in zip(order, per, part):
            got[s] += blocks
            pos[s] += len(fed)
        for s, st in before.items():
            assert cs9.state(s) == st, (rnd, s)
        rnd += 1
    assert got == want


# ---- 3. isolation and reset -------------------------------------------------------------------------------------------
def test_isolation_and_reset(eng):
    import streamly_lz4_amd as S
    x = cut(data("text", 300000, first=40), [65536, 4095, 200000, 13])
    y = cut(data("pysrc", 200000, first=1000), [12, 65537, 65536])
    cs = S.CompressStreams(eng, 5)
    try:
        ox, oy = OracleStream(), OracleStream()
        per, _ = run_device(eng, cs, [x[:2], y[:2], x[:2]], slots=[0, 2, 4])
        assert per[0] == per[2] == framed_by(ox, x[:2])
        assert per[1] == framed_by(oy, y[:2])
        assert cs.state(1) == cs.state(3) == (0, 0, 0)
        cs.reset([2])
        assert cs.state(2) == (0, 0, 0) and cs.state(0) == (65536 + 4095, 4095, 4095)
        per, _ = run_device(eng, cs, [x[2:], y[2:], x[2:]], slots=[4, 2, 0])
        assert per[0] == per[2] == framed_by(ox, x[2:])                 # slots 0 and 4 continue
        assert per[1] == framed_by(OracleStream(), y[2:])                # slot 2 starts again
        assert per[1] != framed_by(oy, y[2:])
        assert cs.state(1) == cs.state(3) == (0, 0, 0)
        cs.reset()
        assert [cs.state(k) for k in range(5)] == [(0, 0, 0)] * 5
        assert run_host(eng, cs, [x], slots=[3])[0] == [framed_by(OracleStream(), x)]
    finally:
        cs.close()


# ---- 4. one stream: the in-kernel scalars against the host's ------------------------------------------------------------
def test_single_stream_equals_the_engines_exact_stream(eng):
    import torch
    import streamly_lz4_amd as S
    arrays = [b for st in ragged_streams() for b in st if len(b) < (1 << 20)]
    cs = S.CompressStreams(eng, 1)
    other = S.Engine(0)
    try:
        other.set_compress_exact(True)
        got = []
        for lo, hi in ((0, 5), (5, 6), (6, len(arrays))):
            got += run_device(eng, cs, [arrays[lo:hi]])[0][0]
        framed, fl = other.compress_batch(arrays)
        assert b"".join(got) == framed and [len(g) for g in got] == fl
        torch.cuda.synchronize()
    finally:
        other.close()
        cs.close()


# ---- 5. the 2 GiB renorm ------------------------------------------------------------------------------------------------
def test_renorm(eng):
    import streamly_lz4_amd as S
    start = 2 ** 31 - 3 * 65536 - 100
    arrays = cut(orc().gen("text", 8, 65536, first_block=3).tobytes(), [65536] * 8)
    o, o2 = OracleStream(), OracleStream()
    o.poke_current_offset(start)
    cs = S.CompressStreams(eng, 2)
    try:
        assert cs.state(0, set_current_offset=start) == (0, 0, 0)
        assert cs.state(0) == (start, 0, 0)
        oracle_all = []
        for lo, hi in ((0, 3), (3, 8)):
            r0 = o.lib.orc_debug_renorms()
            want = framed_by(o, arrays[lo:hi])
            renorms = o.lib.orc_debug_renorms() - r0
            assert renorms == (1 if lo == 3 else 0)                      # the oracle renorms exactly once, at block 3
            want2 = framed_by(o2, arrays[lo:hi])
            oracle_all += want
            per, _ = run_device(eng, cs, [arrays[lo:hi], arrays[lo:hi]])
            assert per[0] == want
            assert per[1] == want2
            assert cs.state(0)[:2] == o.scalars()                        # a missing renorm changes no byte here: the scalars catch it
            assert cs.state(1)[:2] == o2.scalars()
        assert o.scalars() == (393216, 65536) and o2.scalars() == (8 * 65536, 65536)
        raw = b"".join(arrays)
        assert orc().frame_decompress(b"".join(oracle_all), len(raw), 8, 65536, True) == raw
    finally:
        cs.close()


# ---- 6. a bad length ----------------------------------------------------------------------------------------------------
def test_bad_length_stops_its_stream_only(eng, cs9):
    streams = ragged_streams()
    want = expect(1)
    victim = 8                                                         # six blocks
    first = sum(len(st) for st in streams[:victim])
    mx = max(len(b) for st in streams for b in st)
    per, fl = run_device(eng, cs9, streams, bad={first + 2: mx + 1})
    for s in range(len(streams)):
        if s != victim:
            assert per[s] == want[s], s
    assert per[victim][:2] == want[victim][:2]
    assert fl[first + 2:first + 6] == [0, 0, 0, 0]
    two = STREAM_LENS[victim][:2]
    assert cs9.state(victim) == (sum(two), two[1], min(two[1], 65536))
    # the slot is as after block 2: the stream goes on from there
    per, _ = run_device(eng, cs9, [streams[victim][2:]], slots=[victim])
    assert per[0] == want[victim][2:]
    # a negative length, at a stream's first block
    cs9.reset()
    per, fl = run_device(eng, cs9, streams, bad={first: -1})
    assert fl[first:first + 6] == [0] * 6 and cs9.state(victim) == (0, 0, 0)
    assert [per[s] for s in range(victim)] == want[:victim]


# ---- 7. argument checks, the engine's own exact stream ---------------------------------------------------------------------
def test_argument_checks(eng):
    import torch
    import streamly_lz4_amd as S
    cs = S.CompressStreams(eng, 3)
    a = data("text", 4096, first=77)
    try:
        run_device(eng, cs, [[a]], slots=[1])
        st = [cs.state(k) for k in range(3)]
        src = torch.from_numpy(np.frombuffer(a * 3, dtype=np.uint8).copy()).cuda()
        stride = S.slot_stride_ex(4096, 8, False)
        out = torch.zeros(3 * stride, dtype=torch.uint8).cuda()
        flen = torch.full((3,), -7, dtype=torch.int32).cuda()

        def call(sf, sl, n=3):
            return S.lib.mi355lz4_compress_streams_device(
                eng.ctx, cs._h, C.c_void_p(src.data_ptr()), None, None, 4096, 4096, n,
                np.array(sf, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32)),
                np.array(sl, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32)), len(sl), 1, 8,
                C.c_void_p(out.data_ptr()), stride, C.c_void_p(flen.data_ptr()))

        eng._follow_torch()
        assert call([0, 1, 3], [2, 2]) == E_ARG                          # a duplicate slot
        assert call([0, 1, 3], [0, 3]) == E_ARG                          # a slot out of range
        assert call([0, 1, 3], [0, -1]) == E_ARG
        assert call([0, 2, 1, 3], [0, 1, 2]) == E_ARG                    # descending
        assert call([1, 2, 3], [0, 1]) == E_ARG                          # does not start at block 0
        assert call([0, 1, 2], [0, 1]) == E_ARG                          # does not end at nBlocks
        eng.set_compression_level(3)
        assert call([0, 1, 3], [0, 1]) == E_ARG                          # a non-zero compression level
        with pytest.raises(S.LZ4Error, match="compression level"):
            eng.compress_streams([[a]], cs)
        eng.set_compression_level(0)
        with pytest.raises(S.LZ4Error, match="twice"):
            eng.compress_streams([[a], [a]], cs, slots=[1, 1])
        torch.cuda.synchronize()
        assert int(out.count_nonzero()) == 0 and flen.cpu().tolist() == [-7] * 3     # nothing written
        assert [cs.state(k) for k in range(3)] == st
        assert call([0, 1, 3], [0, 2]) == 0
        torch.cuda.synchronize()
        assert min(flen.cpu().tolist()) > 8
    finally:
        eng.set_compression_level(0)
        cs.close()


def test_engines_own_exact_stream_is_untouched(eng):
    import streamly_lz4_amd as S
    mine = cut(data("pysrc", 150000, first=500), [65536, 13, 60000])
    theirs = cut(data("text", 150000, first=60), [4095, 65537, 5])
    cs = S.CompressStreams(eng, 1)
    try:
        eng.set_compress_exact(True)
        om, ot = OracleStream(), OracleStream()
        got_m, got_t = b"", []
        for i in range(3):
            got_m += eng.compress_batch([mine[i]])[0]
            got_t += (run_device if i % 2 else run_host)(eng, cs, [[theirs[i]]])[0][0]
        assert got_m == b"".join(framed_by(om, mine))
        assert got_t == framed_by(ot, theirs)
    finally:
        eng.set_compress_exact(False)
        cs.close()


# ---- 8. decoding -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder", DECODERS)
def test_output_decodes(eng, cs9, decoder):
    import streamly_lz4_amd as S
    streams = ragged_streams()
    framed, fl = eng.compress_streams(streams, cs9)
    sf = np.cumsum([0] + [len(st) for st in streams]).tolist()
    dec = S.Engine(0)
    try:
        dec.set_decoder(decoder)
        out, lens = dec.decompress_streams(framed, sf)
    finally:
        dec.close()
    assert lens == [len(b) for st in streams for b in st]
    assert out == b"".join(b for st in streams for b in st)
    p = 0
    for s, st in enumerate(streams):
        n = sum(fl[sf[s]:sf[s + 1]])
        raw = b"".join(st)
        if st:
            assert orc().frame_decompress(framed[p:p + n], len(raw), 8, 0, True) == raw, s
        p += n


# ---- 9. more streams than the chip has wave slots ---------------------------------------------------------------------------
def test_3000_streams(eng):
    import torch
    import streamly_lz4_amd as S
    n, bl = 3000, 4096
    raw = orc().gen("text", n, bl, first_block=100).tobytes()
    o = OracleStream()
    want = []
    for i in range(n):
        o.reset()
        want.append(framed_by(o, [raw[i * bl:(i + 1) * bl]])[0])
    cs = S.CompressStreams(eng, n)
    try:
        stride = S.slot_stride_ex(bl, 8, False)
        src = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()
        out = torch.zeros(n * stride, dtype=torch.uint8).cuda()
        flen = torch.zeros(n, dtype=torch.int32).cuda()
        slots = np.random.default_rng(5).permutation(n).tolist()
        eng.compress_streams_device(cs, src, n, bl, list(range(n + 1)), slots, out, stride, flen)
        torch.cuda.synchronize()
        sl, fl = out.cpu().numpy(), flen.cpu().tolist()
        assert fl == [len(w) for w in want]
        assert all(sl[i * stride:i * stride + fl[i]].tobytes() == want[i] for i in range(n))
        assert cs.state(slots[0]) == (bl, bl, bl) and cs.state(slots[-1]) == (bl, bl, bl)
    finally:
        cs.close()
