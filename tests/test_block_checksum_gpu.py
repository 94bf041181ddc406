"""Block checksums on the GPU (mi355lz4_set_block_checksum / mi355lz4_xxh32_device; Config.hs setBlockChecksum): the xxh32
kernel against the host xxh32, the compress side's trailers, round trips through the decode paths, corruption, and interop
with liblz4's frame blocks (B.Checksum)."""
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from conftest import DECODERS  # noqa: E402

pytestmark = pytest.mark.gpu

E_BLOCK, E_CAPACITY = -5, -4
BLK_E_COMPLEN, BLK_E_CHECKSUM = -0x7F000001, -0x7F000004
LINKED_VARIANTS = {
    "default": {},
    "runs": {"MI355LZ4_LINKED_RUNS": "64"},
    "pointers": {"MI355LZ4_LINKED_PTR": "1"},
    "replay": {"MI355LZ4_LINKED_PTR": "0"},
    "runin": {"MI355LZ4_LINKED_RUNIN": "1"},
}


@pytest.fixture
def ck_engine(slz4):
    eng = slz4.Engine(0)
    yield eng
    eng.close()


def _gen(eng, kind, bl, n):
    import torch
    src = torch.empty(n * bl, dtype=torch.uint8, device="cuda:0")
    eng.generate(kind, src, bl, n)
    eng.synchronize()
    return src


def _le32(b, at):
    return struct.unpack_from("<i", b, at)[0]


def _blocks_of(framed, hk, ck):
    """[(offset, compLen)] of a dense framed stream."""
    out, pos = [], 0
    while pos < len(framed):
        cl = _le32(framed, pos)
        out.append((pos, cl))
        pos += hk + cl + (4 if ck else 0)
    assert pos == len(framed)
    return out


# ---- 1. the kernel against the host xxh32 ---------------------------------------------------------------------
def test_xxh32_device_matches_host(ck_engine, slz4):
    import torch
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, size=(4 << 20) + (1 << 20), dtype=np.uint8)
    dbuf = torch.from_numpy(buf).cuda()
    host = buf.tobytes()

    def check(offs, lens, seed):
        n = len(offs)
        off = torch.tensor(offs, dtype=torch.int64, device="cuda:0")
        ln = torch.tensor(lens, dtype=torch.int32, device="cuda:0")
        out = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        ck_engine.xxh32_device(dbuf, off, ln, n, seed, out)
        ck_engine.synchronize()
        got = out.cpu().numpy().view(np.uint32).tolist()
        want = [slz4.xxh32(host[o:o + L], seed) for o, L in zip(offs, lens)]
        assert got == want, "seed %d: first mismatch at %d" % (seed, next(i for i in range(n) if got[i] != want[i]))

    for seed in (0, 1):
        # every length 0..64, every byte alignment
        offs = [int(7 * L + (L % 16)) for L in range(65)]
        check(offs, list(range(65)), seed)
        # 4 MiB (+ bound) at an odd offset, alone: the one-range shape
        check([3], [(4 << 20) + (4 << 20) // 255 + 16], seed)
        # 3 big ranges, 160 mid-size, 65 536 small random ones
        check([1, 1 << 20, 2 << 20], [1_400_001, 1_399_999, 1_000_003], seed)
        lens = rng.integers(0, 70_000, size=160).tolist()
        check(rng.integers(0, len(buf) - 70_000, size=160).tolist(), lens, seed)
    lens = rng.integers(0, 200, size=65536).tolist()
    check(rng.integers(0, len(buf) - 200, size=65536).tolist(), lens, 0)


# ---- 2. compress with the switch on ---------------------------------------------------------------------------
def _dev_compress(eng, slz4, src, bl, n, hk, ck, linked, segs, stride=None):
    import torch
    eng.set_block_checksum(ck)
    eng.set_linked_compress(linked)
    eng.set_segments(segs)
    stride = stride or slz4.slot_stride_ex(bl, hk, ck)
    slots = torch.zeros(n * stride, dtype=torch.uint8, device="cuda:0")
    flen = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    eng.compress_batch_device(src, n, bl, slots, stride, flen, header_kind=hk)
    eng.synchronize()
    return slots.cpu().numpy().tobytes(), stride, flen.cpu().numpy().tolist()


@pytest.mark.parametrize("bl,n", [(65536, 8), (1 << 20, 4), (4 << 20, 3)])
@pytest.mark.parametrize("mode", ["independent", "independent-noseg", "linked"])
def test_compress_trailers(ck_engine, slz4, bl, n, mode):
    hk = 8
    src = _gen(ck_engine, "text", bl, n)
    linked, segs = mode == "linked", (0 if mode == "independent-noseg" else -1)
    off_b, s0, f0 = _dev_compress(ck_engine, slz4, src, bl, n, hk, False, linked, segs)
    on_b, s1, f1 = _dev_compress(ck_engine, slz4, src, bl, n, hk, True, linked, segs)
    for i in range(n):
        assert f1[i] == f0[i] + 4
        a, b = off_b[i * s0:i * s0 + f0[i]], on_b[i * s1:i * s1 + f1[i]]
        assert b[:-4] == a, "block %d: data differs from the switch-off output" % i
        assert struct.unpack("<I", b[-4:])[0] == slz4.xxh32(b[hk:-4]), "block %d: trailer" % i
    # a slot stride with room for the data but not for the trailer is refused
    with pytest.raises(slz4.LZ4Error, match=r"\(-4\)"):
        _dev_compress(ck_engine, slz4, src, bl, n, hk, True, linked, segs, stride=slz4.compress_bound(bl) + hk + 3)
    ck_engine.set_segments(-1)
    ck_engine.set_linked_compress(False)


# ---- 3. round trips -------------------------------------------------------------------------------------------
def _host_stream(eng, slz4, kind, bl, n, hk, linked):
    src = _gen(eng, kind, bl, n)
    raw = src.cpu().numpy().tobytes()
    eng.set_block_checksum(True)
    eng.set_linked_compress(linked)
    framed, flen = eng.compress_batch([raw[i * bl:(i + 1) * bl] for i in range(n)], header_kind=hk)
    eng.set_linked_compress(False)
    assert sum(flen) == len(framed)
    for (o, cl), f in zip(_blocks_of(framed, hk, True), flen):
        assert f == hk + cl + 4
        assert struct.unpack_from("<I", framed, o + hk + cl)[0] == slz4.xxh32(framed[o + hk:o + hk + cl])
    return raw, framed


@pytest.mark.parametrize("decoder", DECODERS)
@pytest.mark.parametrize("hk", [4, 8])
def test_round_trip_decoders(ck_engine, slz4, decoder, hk):
    bl, n = 65536, 24
    raw, framed = _host_stream(ck_engine, slz4, "lzsynth", bl, n, hk, False)
    ck_engine.set_decoder(decoder)
    out, blen = ck_engine.decompress_batch(framed, header_kind=hk, fixed_uncomp=bl)
    ck_engine.set_decoder(0)
    assert blen == [bl] * n and out == raw


def _dev_decode(eng, framed, blocks, hk, bl, linked):
    import torch
    n = len(blocks)
    fr = torch.from_numpy(np.frombuffer(framed, dtype=np.uint8).copy()).cuda()
    boff = torch.tensor([o for o, _ in blocks], dtype=torch.int64, device="cuda:0")
    ooff = torch.arange(n + 1, dtype=torch.int64, device="cuda:0") * bl
    out = torch.zeros(n * bl, dtype=torch.uint8, device="cuda:0")
    res = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    rc = 0
    try:
        eng.decompress_batch_device(fr, len(framed), boff, n, out, ooff, res, header_kind=hk, fixed_uncomp=bl, linked=linked)
    except Exception as e:                      # a failed block may be reported by the call itself; nothing else may
        assert "(-5)" in str(e), str(e)
        rc = -5
    eng.synchronize()
    return rc, out.cpu().numpy().tobytes(), res.cpu().numpy().tolist()


@pytest.mark.parametrize("variant", sorted(LINKED_VARIANTS) + ["async", "big"])
def test_round_trip_linked_paths(ck_engine, slz4, monkeypatch, variant):
    hk = 4
    bl, n = ((1 << 20), 4) if variant == "big" else (65536, 48)
    raw, framed = _host_stream(ck_engine, slz4, "text", bl, n, hk, True)
    for k, v in LINKED_VARIANTS.get(variant, {}).items():
        monkeypatch.setenv(k, v)
    if variant == "async":
        ck_engine.set_linked_async(bl)
    blocks = _blocks_of(framed, hk, True)
    _, out, res = _dev_decode(ck_engine, framed, blocks, hk, bl, True)
    assert res == [bl] * n and out == raw
    # the path verifies: one flipped byte in block k's data
    k = n // 2
    o, cl = blocks[k]
    bad = bytearray(framed)
    bad[o + hk + cl // 2] ^= 0x04
    _, out_b, res_b = _dev_decode(ck_engine, bytes(bad), blocks, hk, bl, True)
    ck_engine.set_linked_async(0)
    assert res_b[k] == BLK_E_CHECKSUM and res_b[:k] == [bl] * k and out_b[:k * bl] == raw[:k * bl]
    # and through the host-buffer call, linked
    out2, blen = ck_engine.decompress_batch(framed, header_kind=hk, fixed_uncomp=bl, linked=True)
    assert blen == [bl] * n and out2 == raw


def test_round_trip_streams_and_begin_end(ck_engine, slz4):
    import torch
    hk, bl, n = 8, 65536, 12
    raw, framed = _host_stream(ck_engine, slz4, "text", bl, n, hk, True)
    out, blen = ck_engine.decompress_streams(framed, [0, n], header_kind=hk)
    assert blen == [bl] * n and out == raw
    blocks = _blocks_of(framed, hk, True)
    fr = torch.from_numpy(np.frombuffer(framed, dtype=np.uint8).copy()).cuda()
    boff = torch.tensor([o for o, _ in blocks], dtype=torch.int64, device="cuda:0")
    ooff = torch.arange(n + 1, dtype=torch.int64, device="cuda:0") * bl
    dout = torch.zeros(n * bl, dtype=torch.uint8, device="cuda:0")
    res = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    sf = torch.tensor([0, n], dtype=torch.int32, device="cuda:0")
    ck_engine.decompress_streams_device(fr, len(framed), boff, n, sf, 1, dout, ooff, res, header_kind=hk)
    ck_engine.synchronize()
    assert res.cpu().tolist() == [bl] * n and dout.cpu().numpy().tobytes() == raw
    dout.zero_()
    res.zero_()
    ck_engine.decompress_linked_begin(fr, len(framed), boff, n, dout, ooff, res, 0, header_kind=hk)
    ck_engine.decompress_linked_end()
    ck_engine.synchronize()
    assert res.cpu().tolist() == [bl] * n and dout.cpu().numpy().tobytes() == raw
    # each of the three verifies: block k's data corrupted
    k = 5
    o, cl = blocks[k]
    fr[o + hk + cl // 2] ^= 0x10
    _, blen = ck_engine.decompress_streams(bytes(fr.cpu().numpy().tobytes()), [0, n], header_kind=hk, raise_on_block_error=False)
    assert blen[k] == BLK_E_CHECKSUM and blen[:k] == [bl] * k
    res.zero_()
    ck_engine.decompress_streams_device(fr, len(framed), boff, n, sf, 1, dout, ooff, res, header_kind=hk)
    ck_engine.synchronize()
    assert res.cpu().tolist()[k] == BLK_E_CHECKSUM and res.cpu().tolist()[:k] == [bl] * k
    res.zero_()
    ck_engine.decompress_linked_begin(fr, len(framed), boff, n, dout, ooff, res, 0, header_kind=hk)
    ck_engine.decompress_linked_end()
    ck_engine.synchronize()
    assert res.cpu().tolist()[k] == BLK_E_CHECKSUM and res.cpu().tolist()[:k] == [bl] * k


@pytest.mark.parametrize("engines", [1, 2, 3])
def test_round_trip_multi_handle(slz4, engines):
    m = slz4.MultiEngine([0] * engines)
    try:
        rng = np.random.default_rng(engines)
        blocks = [bytes(rng.integers(0, 4, size=65536, dtype=np.uint8)) for _ in range(10)]
        m.set_block_checksum(True)
        framed, flen = m.compress_batch(blocks, header_kind=8)
        for (o, cl), f in zip(_blocks_of(framed, 8, True), flen):
            assert f == 8 + cl + 4
        out, blen = m.decompress_batch(framed, header_kind=8)
        assert out == b"".join(blocks) and blen == [65536] * 10
        k = 7
        o, cl = _blocks_of(framed, 8, True)[k]
        bad = bytearray(framed)
        bad[o + 8 + cl - 1] ^= 0x80
        _, blen = m.decompress_batch(bytes(bad), header_kind=8, raise_on_block_error=False)
        assert blen[k] == BLK_E_CHECKSUM and [b for i, b in enumerate(blen) if i != k] == [65536] * 9
        if engines > 1:
            import ctypes as C
            slz4.lib.mi355lz4_multi_engine.restype = C.c_void_p
            slz4.lib.mi355lz4_set_block_checksum(C.c_void_p(slz4.lib.mi355lz4_multi_engine(m._h, 1)), 0)
            with pytest.raises(slz4.LZ4Error, match=r"\(-3\)"):
                m.decompress_batch(framed, header_kind=8)
    finally:
        m.close()


# ---- 4. corruption --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["data", "trailer"])
def test_corrupt_independent(ck_engine, slz4, where):
    hk, bl, n, k = 8, 65536, 16, 5
    raw, framed = _host_stream(ck_engine, slz4, "lzsynth", bl, n, hk, False)
    blocks = _blocks_of(framed, hk, True)
    o, cl = blocks[k]
    bad = bytearray(framed)
    bad[o + hk + (cl // 2 if where == "data" else cl + 1)] ^= 0x20
    out, blen = ck_engine.decompress_batch(bytes(bad), header_kind=hk, raise_on_block_error=False)
    assert blen[k] == BLK_E_CHECKSUM
    assert [b for i, b in enumerate(blen) if i != k] == [bl] * (n - 1)
    with pytest.raises(slz4.LZ4Error, match=r"\(-5\)"):
        ck_engine.decompress_batch(bytes(bad), header_kind=hk)
    _, dout, res = _dev_decode(ck_engine, bytes(bad), blocks, hk, bl, False)
    assert res[k] == BLK_E_CHECKSUM
    for i in range(n):
        if i != k:
            assert res[i] == bl and dout[i * bl:(i + 1) * bl] == raw[i * bl:(i + 1) * bl]


def test_corrupt_linked_is_a_rejected_block(ck_engine, slz4):
    hk, bl, n, k = 8, 65536, 16, 6
    raw, framed = _host_stream(ck_engine, slz4, "text", bl, n, hk, True)
    blocks = _blocks_of(framed, hk, True)
    o, cl = blocks[k]
    bad = bytearray(framed)
    bad[o + hk + cl // 3] ^= 0x01
    _, out_ck, res_ck = _dev_decode(ck_engine, bytes(bad), blocks, hk, bl, True)
    rej = bytearray(framed)
    rej[o:o + 4] = struct.pack("<i", 0)                 # the same block rejected by its header instead
    _, out_rj, res_rj = _dev_decode(ck_engine, bytes(rej), blocks, hk, bl, True)
    assert res_ck[k] == BLK_E_CHECKSUM and res_rj[k] == BLK_E_COMPLEN
    for i in range(n):
        if i != k:
            assert res_ck[i] == res_rj[i], "block %d" % i
            if res_ck[i] > 0:
                assert out_ck[i * bl:i * bl + res_ck[i]] == out_rj[i * bl:i * bl + res_rj[i]], "block %d" % i
    assert res_ck[:k] == [bl] * k


def test_trailer_past_the_buffer_is_truncated(ck_engine, slz4):
    hk, bl, n = 8, 65536, 4
    raw, framed = _host_stream(ck_engine, slz4, "lzsynth", bl, n, hk, False)
    blocks = _blocks_of(framed, hk, True)
    _, _, res = _dev_decode(ck_engine, framed[:-2], blocks, hk, bl, False)
    assert res[:-1] == [bl] * (n - 1) and res[-1] == -0x7F000002


# ---- 5. interop with liblz4 -----------------------------------------------------------------------------------
def _lz4f():
    import lz4f
    L = lz4f.load()
    if L is None:
        pytest.skip("liblz4 not available")
    return lz4f, L


def test_liblz4_frame_blocks_decode(ck_engine, slz4):
    import ctypes as C
    lz4f, L = _lz4f()
    bl, n = 65536, 20
    raw = _gen(ck_engine, "text", bl, n).cpu().numpy().tobytes()
    prefs = lz4f.Preferences()
    prefs.frameInfo.blockSizeID = 4                         # 64 KiB
    prefs.frameInfo.blockMode = 1                           # independent
    prefs.frameInfo.blockChecksumFlag = 1
    cap = L.LZ4F_compressFrameBound(len(raw), C.byref(prefs))
    dst = C.create_string_buffer(cap)
    w = L.LZ4F_compressFrame(dst, cap, raw, len(raw), C.byref(prefs))
    assert not L.LZ4F_isError(w)
    frame = dst.raw[:w]
    assert frame[:4] == b"\x04\x22\x4d\x18" and frame[4] & 0x10
    body = frame[7:-4]                                      # magic + FLG + BD + HC, end mark
    assert all(cl > 0 for _, cl in _blocks_of(body, 4, True)), "a stored block: use compressible data"
    ck_engine.set_block_checksum(True)
    out, blen = ck_engine.decompress_batch(body, header_kind=4, fixed_uncomp=bl)
    assert out == raw and blen == [bl] * n
    bad = bytearray(body)
    bad[100] ^= 0x40
    _, blen = ck_engine.decompress_batch(bytes(bad), header_kind=4, fixed_uncomp=bl, raise_on_block_error=False)
    assert blen[0] == BLK_E_CHECKSUM and blen[1:] == [bl] * (n - 1)


def test_engine_blocks_are_a_liblz4_frame(ck_engine, slz4):
    import ctypes as C
    _, L = _lz4f()
    bl, n = 65536, 20
    raw = _gen(ck_engine, "text", bl, n).cpu().numpy().tobytes()
    ck_engine.set_block_checksum(True)
    body, _ = ck_engine.compress_batch([raw[i * bl:(i + 1) * bl] for i in range(n)], header_kind=4)
    assert all(cl < bl for _, cl in _blocks_of(body, 4, True))
    desc = bytes([0x70, 0x40])                              # version 01, independent blocks, block checksums; 64 KiB
    frame = b"\x04\x22\x4d\x18" + desc + bytes([(slz4.xxh32(desc) >> 8) & 0xFF]) + body + b"\x00\x00\x00\x00"
    dctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(C.byref(dctx), 100))
    try:
        out = C.create_string_buffer(len(raw) + 16)
        osz, isz = C.c_size_t(len(raw) + 16), C.c_size_t(len(frame))
        r = L.LZ4F_decompress(dctx, out, C.byref(osz), frame, C.byref(isz), None)
        assert not L.LZ4F_isError(r), L.LZ4F_getErrorName(r)
        assert r == 0 and isz.value == len(frame) and out.raw[:osz.value] == raw
    finally:
        L.LZ4F_freeDecompressionContext(dctx)


# ---- 6. the C++ mirror (compressChunks / decompressChunks with setBlockChecksum True) ------------------------------
def _mirror_stream(eng, slz4, n=12):
    bl = 65536
    raw = _gen(eng, "text", bl, n).cpu().numpy().tobytes()
    cfg = slz4.setBlockChecksum(True, slz4.BlockConfig(slz4.BlockSize.BlockMax64KB))
    arrays = slz4.compressChunks(cfg, 1, [raw[i * bl:(i + 1) * bl] for i in range(n)], eng)
    return cfg, raw, arrays, bl


def test_mirror_round_trip(ck_engine, slz4):
    cfg, raw, arrays, bl = _mirror_stream(ck_engine, slz4)
    for a in arrays:
        cl = _le32(a, 0)
        assert len(a) == 4 + cl + 4 and struct.unpack("<I", a[-4:])[0] == slz4.xxh32(a[4:-4])
    stream = b"".join(arrays)
    assert b"".join(slz4.decompressChunksRaw(cfg, arrays, ck_engine)) == raw
    for size in (1000, 65536, 1 << 20):
        chunks = [stream[i:i + size] for i in range(0, len(stream), size)]
        assert b"".join(slz4.decompressChunks(cfg, chunks, ck_engine)) == raw
        got, err = slz4.decompressChunksStream(cfg, chunks, ck_engine)
        assert err is None and b"".join(got) == raw
    # the engine's own switch is the caller's: the mirror sets it from its config per call and puts it back
    plain = slz4.compressChunks(slz4.BlockConfig(slz4.BlockSize.BlockMax64KB), 1, [raw[:bl]], ck_engine)[0]
    assert len(plain) == 4 + _le32(plain, 0)
    ck_engine.set_block_checksum(True)
    plain = slz4.compressChunks(slz4.BlockConfig(slz4.BlockSize.BlockMax64KB), 1, [raw[:bl]], ck_engine)[0]
    assert len(plain) == 4 + _le32(plain, 0)
    out, blen = ck_engine.decompress_batch(stream, header_kind=4, fixed_uncomp=bl)     # still on for the engine's calls
    assert out == raw


@pytest.mark.parametrize("batch", [4096, 3])
def test_mirror_error_in_stream_order(ck_engine, slz4, batch):
    cfg, raw, arrays, bl = _mirror_stream(ck_engine, slz4)
    k = 7
    bad = [bytearray(a) for a in arrays]
    bad[k][4 + 100] ^= 0x01
    stream = b"".join(bytes(a) for a in bad)
    ck_engine.set_batch_blocks(batch)
    with pytest.raises(slz4.LZ4Error, match="checksum.*block %d" % k):
        slz4.decompressChunks(cfg, [stream], ck_engine)
    got, err = slz4.decompressChunksStream(cfg, [stream[i:i + 5000] for i in range(0, len(stream), 5000)], ck_engine)
    assert err is not None and "checksum" in str(err) and "block %d" % k in str(err)
    assert [bytes(g) for g in got] == [raw[i * bl:(i + 1) * bl] for i in range(k)]
    ck_engine.set_batch_blocks(4096)
