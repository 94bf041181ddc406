"""Level 0 against a prepared dictionary by the wave encoder: mi355lz4_compress_fastdict_device / mi355lz4_compress_fastdict and the
table image mi355lz4_hcdict_load builds for them.

The contract needs no CPU codec: with keep = min(len, 65536), block i is what the engine writes for it as the SECOND block of the
linked two-block call [D[-keep:], B_i] through mi355lz4_compress_batch_device at level 0 with the same accel and
max(keep, maxBlockLen) as its maxBlockLen; with keep == 0 the block of the one-block linked call.  One linked call over all the
pairs of a dictionary length, laid into one buffer with gaps between the pairs, gives every oracle block.  On top of that: every
block is a valid LZ4 block (tests/lz4_check.py) that mi355lz4_decompress_dict_device and the CPU oracle decode with the dictionary;
hand-built seam cases; a wave's second and later blocks; the object only read; confinement; arguments; checksums; the host form."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dict_cases as DC  # noqa: E402
import guarded as G  # noqa: E402
import lz4_check  # noqa: E402
from dstreams_model import xxh32  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG, E_CAPACITY = -3, -4
APART = 7                     # sources lie 7 bytes apart: every alignment occurs
FILL = 0xA5
KNOB = "MI355LZ4_FASTDICT_WAVES"
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bytes_t(b):
    """bytes on the device (one byte at least, so that the tensor has a pointer)"""
    return _t(np.frombuffer(bytes(b) + b"\x00", dtype=np.uint8).copy())


def rnd(seed, n):
    return np.random.RandomState(seed).randint(0, 256, size=n).astype(np.uint8).tobytes()


def spaced(datas, apart=APART, lead=3, order=None):
    """the datas in one buffer, `apart` bytes between them, laid down in `order` (a permutation; default: as given): (buffer, offsets)"""
    off, pos = [0] * len(datas), lead
    for i in (range(len(datas)) if order is None else order):
        off[i] = pos
        pos += len(datas[i]) + apart
    buf = np.full(pos + 64, FILL, dtype=np.uint8)
    for o, d in zip(off, datas):
        buf[o:o + len(d)] = np.frombuffer(bytes(d), dtype=np.uint8)
    return buf, off


@pytest.fixture(scope="module")
def setup():
    import streamly_lz4_amd as S
    os.environ.pop(KNOB, None)
    eng = S.Engine(0)
    hd = S.HcDict(eng)
    yield S, eng, hd
    os.environ.pop(KNOB, None)
    eng.set_compression_level(0)
    eng.set_block_checksum(False)
    eng.set_linked_compress(False)
    hd.close()
    eng.close()


def load(eng, hd, dictionary):
    d = _bytes_t(dictionary)
    hd.load(d, len(dictionary))
    eng.synchronize()
    assert len(hd) == min(len(dictionary), 65536)


def fd_call(S, eng, hd, blocks, accel=1, kind=8, checksum=False, lens=None, maxlen=None, order=None, waves=None):
    """one compress_fastdict_device call over `blocks`, APART bytes apart: (framedLen[], [slot bytes up to framedLen], all slots)"""
    import torch
    n = len(blocks)
    mx = max([len(b) for b in blocks] + [1]) if maxlen is None else maxlen
    buf, off = spaced(blocks, order=order)
    stride = S.slot_stride_ex(mx, kind, checksum)
    slots = torch.full((max(n, 1) * stride,), FILL, dtype=torch.uint8, device=DEV)
    flen = torch.full((max(n, 1),), -77, dtype=torch.int32, device=DEV)
    eng.set_compression_level(0)
    eng.set_block_checksum(checksum)
    if waves is not None:
        os.environ[KNOB] = str(waves)
    try:
        eng.compress_fastdict_device(hd, _t(buf), n, mx, slots, stride, flen, accel=accel, header_kind=kind,
                                     src_off=_t(np.array(off + [0], dtype=np.int64)),
                                     src_len=_t(np.array([len(b) for b in blocks] if lens is None else lens, dtype=np.int32)), block_stride=0)
        eng.synchronize()
    finally:
        eng.set_block_checksum(False)
        os.environ.pop(KNOB, None)
    fl, hb = flen.cpu().tolist()[:n], slots.cpu().numpy()
    return fl, [hb[i * stride:i * stride + max(fl[i], 0)].tobytes() for i in range(n)], hb.reshape(max(n, 1), stride)


def payloads(S, eng, hd, blocks, accel=1, maxlen=None, **kw):
    fl, got, _ = fd_call(S, eng, hd, blocks, accel, maxlen=maxlen, **kw)
    for f, g, b in zip(fl, got, blocks):
        assert f == len(g) and int.from_bytes(g[:4], "little") == f - 8 and int.from_bytes(g[4:8], "little") == len(b)
    return [g[8:] for g in got]


def linked_oracle(S, eng, dictionary, blocks, accel=1, maxlen=None):
    """The contract's right-hand side for every block at once: all pairs [D[-keep:], B] in one buffer with gaps between the pairs
    (a pair's first block then has nothing directly in front of it), ONE linked compress_batch_device call at level 0 with
    max(keep, maxlen) as its maxBlockLen; the payload of every pair's second block.  keep == 0: the one-block pairs [B]."""
    import torch
    kept = bytes(dictionary[-65536:]) if dictionary else b""
    mx = max([len(b) for b in blocks] + [1]) if maxlen is None else maxlen
    parts, offs, second, pos = [], [], [], 5
    for b in blocks:
        if kept:
            parts.append(kept)
            offs.append(pos)
            pos += len(kept)
        second.append(len(offs))
        parts.append(bytes(b))
        offs.append(pos)
        pos += len(b) + APART + 4             # the gap: the next pair is not linked to this one
    lens = [len(x) for x in parts]
    data = np.full(pos + 64, FILL, dtype=np.uint8)
    for o, x in zip(offs, parts):
        data[o:o + len(x)] = np.frombuffer(x, dtype=np.uint8)
    n, big = len(offs), max(len(kept), mx)
    stride = S.slot_stride_ex(big, 8, False)
    slots = torch.full((n * stride,), FILL, dtype=torch.uint8, device=DEV)
    flen = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    eng.set_compression_level(0)
    eng.set_linked_compress(True)
    try:
        eng.compress_batch_device(_t(data), n, big, slots, stride, flen, accel=accel, header_kind=8, src_off=_t(np.array(offs, dtype=np.int64)),
                                  src_len=_t(np.array(lens, dtype=np.int32)), block_stride=0)
        eng.synchronize()
    finally:
        eng.set_linked_compress(False)
    fl, hb = flen.cpu().tolist(), slots.cpu().numpy()
    return [hb[i * stride + 8:i * stride + fl[i]].tobytes() for i in second]


def sequences(block):
    """[(output position of the literals, literal count, offset, match length)] of a valid block; the last entry has offset 0"""
    out, i, pos = [], 0, 0
    while i < len(block):
        tok = block[i]
        i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = block[i]
                i += 1
                lit += b
                if b != 255:
                    break
        i += lit
        if i >= len(block):
            out.append((pos, lit, 0, 0))
            break
        off = block[i] | (block[i + 1] << 8)
        i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = block[i]
                i += 1
                ml += b
                if b != 255:
                    break
        out.append((pos, lit, off, ml + 4))
        pos += lit + ml + 4
    return out


def decode_on_device(eng, framed_blocks, sizes, dict_t, dict_len, kind):
    """the framed blocks (header, payload, trailer as the compress call wrote them) through decompress_dict_device, capacities exact:
    (results, [decoded bytes])"""
    import torch
    framed, boff = bytearray(), []
    for g in framed_blocks:
        boff.append(len(framed))
        framed += g
    ooff = np.cumsum([0] + [s + APART for s in sizes])[:-1].astype(np.int64)
    out = torch.full((int(ooff[-1]) + sizes[-1] + 64,), FILL, dtype=torch.uint8, device=DEV)
    res = torch.full((len(sizes),), -77, dtype=torch.int32, device=DEV)
    eng.decompress_dict_device(_bytes_t(framed), len(framed), _t(np.array(boff, dtype=np.int64)), len(sizes), dict_t, dict_len, out,
                               _t(ooff), res, header_kind=kind, fixed_uncomp=max(sizes) if kind == 4 else 0,
                               out_cap=_t(np.array(sizes, dtype=np.int32)) if kind == 4 else None)
    eng.synchronize()
    hb = out.cpu().numpy()
    return res.cpu().tolist(), [hb[o:o + s].tobytes() for o, s in zip(ooff, sizes)]


def validate(S, eng, oracle, D, blocks, framed, kind=8, checksum=False):
    """every block passes the strict validator with the dictionary and decodes to its input on the CPU and on the device"""
    keep = min(len(D), 65536)
    trailer = 4 if checksum else 0
    for g, b in zip(framed, blocks):
        comp = g[kind:len(g) - trailer]
        lz4_check.check_block(comp, len(b), dict_len=keep)
        assert oracle.decompress_block(comp, len(b), D[-65536:] if D else None) == (len(b), b), (len(D), len(b))
    eng.set_block_checksum(checksum)
    try:
        r, outs = decode_on_device(eng, framed, [len(b) for b in blocks], _bytes_t(D), len(D), kind)
    finally:
        eng.set_block_checksum(False)
    assert r == [len(b) for b in blocks] and outs == [bytes(b) for b in blocks], (len(D), r)


# ---- 1. and 3. the grid: byte equality with the linked oracle, both kernel forms, both headers; validity ------------------------------
SMALL = [bl for bl in DC.BLOCK_LENS if bl <= 65536]


@pytest.mark.parametrize("dl", DC.DICT_LENS)
def test_grid_is_the_linked_call_s_second_block(setup, oracle, dl):
    """one load and, per accel, header kind and kernel form, one ragged call with every block length, sources 7 bytes apart"""
    S, eng, hd = setup
    D = DC.dictionary(dl)
    load(eng, hd, D)
    for lens_, mx in ((SMALL, 65536), (list(DC.BLOCK_LENS), 100000)):          # k_encode<true, true>'s form / k_encode<true, false>'s
        blocks = [DC.block(bl) for bl in lens_]
        for accel in DC.ACCELS:
            want = linked_oracle(S, eng, D, blocks, accel, maxlen=mx)
            for kind in (8, 4):
                fl, got, _ = fd_call(S, eng, hd, blocks, accel, kind, maxlen=mx)
                for i, b in enumerate(blocks):
                    comp = got[i][kind:]
                    assert fl[i] == kind + len(comp) and int.from_bytes(got[i][:4], "little") == len(comp), (dl, len(b), accel, kind)
                    if kind == 8:
                        assert int.from_bytes(got[i][4:8], "little") == len(b)
                    assert comp == want[i], "dictionary %d, block %d, accel %d, header %d, maxBlockLen %d" % (dl, len(b), accel, kind, mx)
                    if len(b) < 13:                                             # literals only; an empty block is the zero token
                        assert comp == (bytes([len(b) << 4]) + b if b else b"\x00")
                if accel == 1 or kind == 8:
                    validate(S, eng, oracle, D, blocks, got, kind)


# ---- 2. the seam, hand-built ------------------------------------------------------------------------------------------------------------
def seam_case(S, eng, hd, oracle, D, blocks, accel=1):
    load(eng, hd, D)
    fl, got, _ = fd_call(S, eng, hd, blocks, accel)
    comps = [g[8:] for g in got]
    assert comps == linked_oracle(S, eng, D, blocks, accel)
    validate(S, eng, oracle, D, blocks, got)
    return comps


def test_seam_block_continues_a_match_that_starts_in_the_dictionary(setup, oracle):
    """the block is the dictionary's bytes from some offset on: its first match lies in the dictionary and runs for (nearly) the
    whole copied stretch"""
    S, eng, hd = setup
    D = rnd(2, 3000)
    for at in (1000, 1001, 2047, 2990 - 500):
        B = D[at:at + 500] + rnd(3, 40)
        comp = seam_case(S, eng, hd, oracle, D, [B])[0]
        matches = [s for s in sequences(comp) if s[2]]
        assert matches and matches[0][2] == len(D) - at, (at, matches[:2])
        assert lz4_check.check_block(comp, len(B), dict_len=len(D))[3] >= 1, "a match reaches into the dictionary"
    # ... and from ENC_SEED_STEP-odd and seam positions: the dictionary's last bytes go on in the block
    X = rnd(4, 20)
    D2, B2 = rnd(5, 1000) + X, X + X + X + rnd(6, 20)
    seam_case(S, eng, hd, oracle, D2, [B2])


def test_seam_block_equals_the_first_kept_bytes(setup, oracle):
    """offsets near 65535: the block repeats the first bytes the dictionary kept"""
    S, eng, hd = setup
    D = rnd(21, 70000)
    kept = D[-65536:]
    blocks = [kept[:300] + rnd(22, 30), kept[1:200] + rnd(23, 30), rnd(24, 1023) + kept[1024:1064] + rnd(25, 61)]
    comps = seam_case(S, eng, hd, oracle, D, blocks)
    for comp, b in zip(comps, blocks):
        assert lz4_check.check_block(comp, len(b), dict_len=65536)[1] <= 65535


@pytest.mark.parametrize("keep", [1000, 1001, 128 + 2, 128 + 3, 131, 65536, 65535])
def test_seam_positions_share_a_bucket_with_older_ones(setup, oracle, keep):
    """the dictionary's last 12 bytes are one repeated byte: the seam positions and older positions of the same seed step hash
    alike (same bucket, same tag), for an odd and an even keep and where the seam falls on a step's edge.  Blocks that begin with
    that byte's run go on from the seam; one begins with other bytes"""
    S, eng, hd = setup
    D = rnd(31 + keep, keep - 12) + b"\x77" * 12
    blocks = [b"\x77" * 40 + rnd(32, 30), b"\x77" * 3 + rnd(33, 60), b"\x77" * 5 + D[5:60], rnd(34, 64), b"\x77" * 13]
    for accel in (1, 7):
        seam_case(S, eng, hd, oracle, D, blocks, accel)


@pytest.mark.parametrize("keep", [1, 4, 5, 6, 127, 128, 129, 130, 131, 132])
def test_seam_short_dictionaries_and_step_edges(setup, oracle, keep):
    """keep of 1, 4, 5 and 6: no position, or only seam positions, are entered; around 128 a seed step's edge cuts the seam in two"""
    S, eng, hd = setup
    D = DC.dictionary(4096)[:keep]
    blocks = [D + D + rnd(41, 20), D[-3:] * 8 + rnd(42, 30), DC.block(1000), D[-1:] * 30, DC.block(13)]
    seam_case(S, eng, hd, oracle, D, blocks)
    img = hd.fast_image()
    assert int.from_bytes(img[10240:10244], "little") == keep
    seam0 = int.from_bytes(img[10244:10248], "little")
    first_seam = (max(keep - 4, 0) + 1) // 2 * 2          # the first entered (even) position whose five bytes pass the dictionary's end
    assert seam0 == first_seam // 128 * 128, "the image ends in front of the step that holds the first seam position"
    if keep <= 4 or seam0 == 0:
        assert img[:10240] == bytes(10240), "no step without a seam position: the image is the empty table"


# ---- 4. a wave's second block ----------------------------------------------------------------------------------------------------------
def test_a_wave_s_later_blocks_start_clean(setup, oracle):
    """two waves in all take 40 blocks of 65536, 13, 4096, 0, 12, 1000 bytes in turn: every block is its oracle block and what the
    default grid gives it -- nothing of the image, the seam or the window leaks from one block into the next"""
    S, eng, hd = setup
    D = DC.dictionary(65536)
    load(eng, hd, D)
    sizes = [(65536, 13, 4096, 0, 12, 1000)[i % 6] for i in range(40)]
    blocks = [DC.text(610000 + i, n) for i, n in enumerate(sizes)]
    want = linked_oracle(S, eng, D, blocks, maxlen=65536)
    two = payloads(S, eng, hd, blocks, maxlen=65536, waves=-2)
    dflt = payloads(S, eng, hd, blocks, maxlen=65536)
    one = payloads(S, eng, hd, blocks, maxlen=65536, waves=-1)
    for i in range(40):
        assert two[i] == want[i], "block %d (%d bytes) of two waves' call" % (i, sizes[i])
        assert dflt[i] == want[i] and one[i] == want[i], i


# ---- 5. the object is only read, and building is repeatable ----------------------------------------------------------------------------
def test_object_is_only_read_and_the_build_repeats(setup):
    S, eng, hd = setup
    D1, D2 = DC.dictionary(70000), DC.dictionary(4095)
    blocks = [DC.block(bl) for bl in (64, 1000, 4096)]
    load(eng, hd, D1)
    fast, image = hd.fast_image(), hd.image()
    assert len(fast) == S.HcDict.FAST_IMAGE_BYTES and len(image) == S.HcDict.IMAGE_BYTES
    assert int.from_bytes(fast[10240:10244], "little") == 65536 and fast[:10240] != bytes(10240)
    first = payloads(S, eng, hd, blocks)
    eng.set_compression_level(9)
    try:
        import torch
        buf, off = spaced(blocks)
        stride = S.slot_stride_ex(4096, 8, False)
        slots = torch.zeros(3 * stride, dtype=torch.uint8, device=DEV)
        flen = torch.zeros(3, dtype=torch.int32, device=DEV)
        eng.compress_hcdict_device(hd, _t(buf), 3, 4096, slots, stride, flen, header_kind=8, src_off=_t(np.array(off, dtype=np.int64)),
                                   src_len=_t(np.array([len(b) for b in blocks], dtype=np.int32)), block_stride=0)
        eng.synchronize()
        hc_first = slots.cpu().numpy().tobytes()
        assert all(f > 8 for f in flen.cpu().tolist())
    finally:
        eng.set_compression_level(0)
    assert hd.fast_image() == fast and hd.image() == image, "a compress call wrote the prepared dictionary"
    load(eng, hd, D1)
    assert hd.fast_image() == fast and hd.image() == image, "loading the same dictionary again gave another image"
    assert payloads(S, eng, hd, blocks) == first
    load(eng, hd, D2)
    assert hd.fast_image() != fast
    second = payloads(S, eng, hd, blocks)
    assert second != first and second == linked_oracle(S, eng, D2, blocks)
    eng.set_compression_level(9)
    try:
        slots.zero_()
        eng.compress_hcdict_device(hd, _t(buf), 3, 4096, slots, stride, flen, header_kind=8, src_off=_t(np.array(off, dtype=np.int64)),
                                   src_len=_t(np.array([len(b) for b in blocks], dtype=np.int32)), block_stride=0)
        eng.synchronize()
        assert slots.cpu().numpy().tobytes() != hc_first
    finally:
        eng.set_compression_level(0)
    load(eng, hd, b"")
    assert hd.fast_image() == bytes(S.HcDict.FAST_IMAGE_BYTES)
    assert payloads(S, eng, hd, blocks) == linked_oracle(S, eng, b"", blocks)


# ---- 6. bad lengths and confinement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("checksum,extra,bad", [(False, 0, False), (True, 37, False), (False, 37, True), (True, 0, True)])
def test_call_is_confined(oracle, checksum, extra, bad):
    """srcLen of -1 and maxBlockLen + 1: framedLen 0 and an untouched slot, the neighbours right; nothing of a slot behind
    framedLen[i], nothing outside the slots, no input, neither image"""
    import torch
    import streamly_lz4_amd as S
    dl, mx = 70000, max(DC.BLOCK_LENS)
    D = DC.dictionary(dl)
    blocks = [DC.block(bl) for bl in DC.BLOCK_LENS]
    n = len(blocks)
    lens = [len(b) for b in blocks]
    dead = {2, 7} if bad else set()
    if bad:
        lens[2], lens[7] = -1, mx + 1
    need = S.slot_stride_ex(mx, 8, checksum)
    stride = need + extra
    lay_src = G.layout([len(b) for b in blocks])
    lay = G.layout([need] * n, stride=stride, first_residue=extra)
    eng = S.Engine(0)
    hd = S.HcDict(eng)
    try:
        want = linked_oracle(S, eng, D, blocks, maxlen=mx)
        eng.set_block_checksum(checksum)
        dlay = G.layout([dl], first_residue=5)
        dbuf = _t(G.pair(dlay, [D], seeds=(31, 32))[0])
        hd.load(dbuf[dlay.starts[0]:dlay.starts[0] + dl], dl)
        eng.synchronize()
        dcopy = dbuf.clone()
        image, fast = hd.image(), hd.fast_image()
        seed = 73
        buf = G.new_torch(lay.total, seed, DEV)
        flen = G.GuardedArray(n, torch.int32, seed + 50, DEV)
        src = _t(G.pair(lay_src, blocks)[0])
        off = _t(np.array(lay_src.starts, dtype=np.int64))
        ln = _t(np.array(lens, dtype=np.int32))
        copies = [t.clone() for t in (src, off, ln)]
        eng.compress_fastdict_device(hd, src, n, mx, buf[lay.starts[0]:], stride, flen.view, accel=1, header_kind=8, src_off=off,
                                     src_len=ln, block_stride=0)
        eng.synchronize()
        torch.cuda.synchronize()
        fl = flen.view.cpu().tolist()
        allowed = [(s, s + fl[i]) for i, (s, _) in enumerate(lay.ranges()) if i not in dead]
        G.assert_confined(buf, allowed, seed, "slots")
        flen.check(what="framedLen[]")
        for t, c in zip((src, off, ln), copies):
            assert torch.equal(t, c), "an input was written"
        assert torch.equal(dbuf, dcopy), "the dictionary tensor was written"
        assert hd.image() == image and hd.fast_image() == fast, "the prepared dictionary was written"
        hb = buf.cpu().numpy()
        trailer = 4 if checksum else 0
        for i, bl in enumerate(DC.BLOCK_LENS):
            if i in dead:
                assert fl[i] == 0
                continue
            comp = hb[lay.starts[i] + 8:lay.starts[i] + fl[i] - trailer].tobytes()
            assert int.from_bytes(hb[lay.starts[i]:lay.starts[i] + 4].tobytes(), "little") == len(comp)
            assert comp == want[i], bl
            lz4_check.check_block(comp, bl, dict_len=65536)
            assert oracle.decompress_block(comp, bl, D[-65536:]) == (bl, blocks[i]), bl
    finally:
        eng.set_block_checksum(False)
        hd.close()
        eng.close()


# ---- 7. arguments on a live engine --------------------------------------------------------------------------------------------------------
def test_arguments(setup):
    """every error of the device call on a live engine; nothing is enqueued: the outputs keep their pattern and the images their bytes"""
    import torch
    S, eng, hd = setup
    L, P = S.lib, S._dptr
    D = DC.dictionary(100)
    load(eng, hd, D)
    fast = hd.fast_image()
    blocks = [DC.block(bl) for bl in (64, 1000)]
    buf, off = spaced(blocks)
    src, so, sl = _t(buf), _t(np.array(off, dtype=np.int64)), _t(np.array([64, 1000], dtype=np.int32))
    stride = S.slot_stride_ex(1000, 8, False)
    slots = torch.full((2 * stride,), FILL, dtype=torch.uint8, device=DEV)
    flen = torch.full((2,), -77, dtype=torch.int32, device=DEV)

    def comp(ctx=eng.ctx, h=hd._h, src=src, nb=2, kind=8, mx=1000, slots=slots, stride=stride, flen=flen, accel=1):
        return L.mi355lz4_compress_fastdict_device(ctx, h, P(src), P(so), P(sl), 0, mx, nb, accel, kind, P(slots), stride, P(flen))

    try:
        for kw in (dict(ctx=None), dict(h=None), dict(nb=-1), dict(kind=5), dict(mx=-1), dict(mx=(4 << 20) + 1, stride=8 << 20),
                   dict(src=None), dict(slots=None), dict(flen=None)):
            assert comp(**kw) == E_ARG, kw
            assert b"compress_fastdict_device" in L.mi355lz4_last_error(), kw
        need = S.compress_bound(1000) + 8         # (slot_stride_ex rounds up: the bound itself is the limit)
        assert comp(stride=need - 1) == E_CAPACITY and b"compress_fastdict_device" in L.mi355lz4_last_error()
        eng.set_block_checksum(True)
        assert comp(stride=need + 3) == E_CAPACITY, "the trailer counts in the bound"
        eng.set_block_checksum(False)
        for level in (1, 9):
            eng.set_compression_level(level)
            assert comp() == E_ARG and b"compress_hcdict_device" in L.mi355lz4_last_error()
        eng.set_compression_level(0)
        if torch.cuda.device_count() > 1:       # an object created on another device
            far = S.Engine(1)
            hd2 = S.HcDict(far)
            try:
                assert comp(h=hd2._h) == E_ARG and b"device" in L.mi355lz4_last_error()
            finally:
                hd2.close()
                far.close()
        assert comp(nb=0, src=None, slots=None, flen=None) == 0
        eng.synchronize()
        assert (slots == FILL).all() and (flen == -77).all()
        assert hd.fast_image() == fast
        # accel is clamped like compress_batch_device's: 0 is 1, anything above 65537 is 65537
        for accel, same_as in ((0, 1), (-3, 1), (1 << 20, 65537)):
            assert comp(accel=accel) == 0
            eng.synchronize()
            fl, hb = flen.cpu().tolist(), slots.cpu().numpy()
            assert [hb[i * stride + 8:i * stride + fl[i]].tobytes() for i in range(2)] == payloads(S, eng, hd, blocks, same_as), accel
    finally:
        eng.set_block_checksum(False)
        eng.set_compression_level(0)


# ---- 8. placement ---------------------------------------------------------------------------------------------------------------------------
def test_blocks_may_lie_in_any_order(setup):
    """srcOff descending, and shuffled: every block's bytes are those of the ascending call"""
    S, eng, hd = setup
    load(eng, hd, DC.dictionary(65536))
    blocks = [DC.text(620000 + i, n) for i, n in enumerate((4096, 13, 0, 1000, 65536, 12, 300, 4096, 64, 2000))]
    want = payloads(S, eng, hd, blocks)
    n = len(blocks)
    assert payloads(S, eng, hd, blocks, order=list(range(n - 1, -1, -1))) == want
    assert payloads(S, eng, hd, blocks, order=[int(i) for i in np.random.RandomState(3).permutation(n)]) == want


# ---- 9. checksums -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [8, 4])
def test_block_checksums(setup, oracle, kind):
    """with block checksums on every trailer is the xxh32 of its block's data, and the decoder accepts it"""
    S, eng, hd = setup
    D = DC.dictionary(65536)
    load(eng, hd, D)
    blocks = [DC.block(bl) for bl in (0, 1, 12, 13, 64, 1000, 4096)]
    plain = [g[kind:] for g in fd_call(S, eng, hd, blocks, kind=kind)[1]]
    fl, got, _ = fd_call(S, eng, hd, blocks, kind=kind, checksum=True)
    for i, b in enumerate(blocks):
        comp, trailer = got[i][kind:-4], got[i][-4:]
        assert fl[i] == kind + len(comp) + 4 and comp == plain[i]
        assert int.from_bytes(got[i][:4], "little") == len(comp)
        assert int.from_bytes(trailer, "little") == xxh32(comp), len(b)
    validate(S, eng, oracle, D, blocks, got, kind, checksum=True)


# ---- 10. the host form --------------------------------------------------------------------------------------------------------------------------
def test_host_form(setup):
    """compress_fastdict: the device call's blocks, densely framed; a bad length is E_ARG and nothing is written"""
    S, eng, hd = setup
    load(eng, hd, DC.dictionary(65536))
    rs = np.random.RandomState(9)
    blocks = [DC.text(630000 + i, int(rs.randint(0, 3000))) for i in range(50)]
    for accel in (1, 7):
        want = payloads(S, eng, hd, blocks, accel)
        eng.set_compression_level(0)
        framed, flen = eng.compress_fastdict(blocks, hd, accel=accel)
        dense = b"".join(len(w).to_bytes(4, "little") + len(b).to_bytes(4, "little") + w for w, b in zip(want, blocks))
        assert flen == [8 + len(w) for w in want] and framed == dense
    out = np.full(4096, FILL, dtype=np.uint8)
    fl, st = np.full(2, -77, dtype=np.int32), np.full(2, -77, dtype=np.int32)
    src = np.frombuffer(blocks[0] + bytes(16), dtype=np.uint8)
    ptrs = (_u8p * 2)(src.ctypes.data_as(_u8p), src.ctypes.data_as(_u8p))
    for bad in (-1, (4 << 20) + 1):
        lens = np.array([8, bad], dtype=np.int32)
        got = C.c_size_t(99)
        rc = S.lib.mi355lz4_compress_fastdict(eng.ctx, hd._h, ptrs, lens.ctypes.data_as(_i32p), 2, 1, 8, out.ctypes.data_as(_u8p),
                                              out.size, C.byref(got), fl.ctypes.data_as(_i32p), st.ctypes.data_as(_i32p))
        assert rc == E_ARG and got.value == 0 and b"compress_fastdict" in S.lib.mi355lz4_last_error()
        assert (out == FILL).all() and (fl == -77).all() and (st == -77).all()


# ---- 11. ratio, as a condition ------------------------------------------------------------------------------------------------------------------
def test_ratio_beats_the_call_without_a_dictionary(setup, record):
    """256 text records of 4 KiB against a 64 KiB dictionary: smaller in all than compress_batch_device makes them; the size of
    compress_dict_device (the reference's parse with the same dictionary) is printed beside it"""
    import torch
    S, eng, hd = setup
    D = DC.dictionary(65536)
    load(eng, hd, D)
    n, cnt = 4096, 256
    blocks = [DC.text(700000 + i, n) for i in range(cnt)]
    fast = sum(len(p) for p in payloads(S, eng, hd, blocks))
    buf, off = spaced(blocks)
    stride = S.slot_stride_ex(n, 8, False)
    args = dict(accel=1, header_kind=8, src_off=_t(np.array(off, dtype=np.int64)), src_len=_t(np.array([n] * cnt, dtype=np.int32)), block_stride=0)
    slots = torch.zeros(cnt * stride, dtype=torch.uint8, device=DEV)
    flen = torch.zeros(cnt, dtype=torch.int32, device=DEV)
    eng.set_compression_level(0)
    eng.compress_batch_device(_t(buf), cnt, n, slots, stride, flen, **args)
    eng.synchronize()
    plain = int(flen.sum().item()) - 8 * cnt
    cs = S.CompressStreams(eng, 1)
    try:
        cs.load_dict(0, _bytes_t(D), len(D))
        eng.compress_dict_device(cs, 0, _t(buf), cnt, n, slots, stride, flen, **args)
        eng.synchronize()
        exact = int(flen.sum().item()) - 8 * cnt
    finally:
        cs.close()
    rec = {"records": cnt, "bytes": n * cnt, "fastdict": fast, "batch_no_dict": plain, "dict_level0": exact}
    print("fastdict ratio:", rec)
    record("fastdict_ratio", rec)
    assert fast < plain, rec
