"""High-compression levels against a shared dictionary on the GPU: mi355lz4_hcdict_load (the prepared tables of a dictionary) and
mi355lz4_compress_hcdict_device / mi355lz4_compress_hcdict (levels 1..12 with that dictionary in front of every block).

The contract needs no CPU HC codec: block i is what the engine writes for it as the SECOND block of the linked two-block call
[D[-65536:], B] through mi355lz4_compress_batch_device at the same level.  On top of that: every block is a valid LZ4 block
(tests/lz4_check.py) that mi355lz4_decompress_dict_device and the oracle decode with the dictionary, hand-built seam cases, the
table image restored between the blocks of a workgroup, and the ratio against level 0 and against liblz4's HC with a dictionary."""
import ctypes as C
import ctypes.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dict_cases as DC  # noqa: E402
import lz4_check  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG, E_CAPACITY = -3, -4
MAXLEN = max(DC.BLOCK_LENS)
APART = 7                     # sources lie 7 bytes apart: every alignment occurs
FILL = 0xA5
_i32p = C.POINTER(C.c_int32)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bytes_t(b):
    """bytes on the device (one byte at least, so that the tensor has a pointer)"""
    return _t(np.frombuffer(bytes(b) + b"\x00", dtype=np.uint8).copy())


def rnd(seed, n):
    return np.random.RandomState(seed).randint(0, 256, size=n).astype(np.uint8).tobytes()


def spaced(datas, apart=APART, lead=3):
    off, pos = [], lead
    for d in datas:
        off.append(pos)
        pos += len(d) + apart
    buf = np.full(pos + 64, FILL, dtype=np.uint8)
    for o, d in zip(off, datas):
        buf[o:o + len(d)] = np.frombuffer(bytes(d), dtype=np.uint8)
    return buf, off


@pytest.fixture(scope="module")
def setup():
    import streamly_lz4_amd as S
    eng = S.Engine(0)
    hd = S.HcDict(eng)
    yield S, eng, hd
    eng.set_compression_level(0)
    eng.set_block_checksum(False)
    hd.close()
    eng.close()


def load(eng, hd, dictionary):
    d = _bytes_t(dictionary)
    hd.load(d, len(dictionary))
    eng.synchronize()
    assert len(hd) == min(len(dictionary), 65536)


def hc_call(S, eng, hd, blocks, level, kind=8, checksum=False, lens=None, maxlen=None):
    """one compress_hcdict_device call over `blocks`, APART bytes apart: (framedLen[], [slot bytes up to framedLen], all slots)"""
    import torch
    n = len(blocks)
    mx = max([len(b) for b in blocks] + [1]) if maxlen is None else maxlen
    buf, off = spaced(blocks)
    stride = S.slot_stride_ex(mx, kind, checksum)
    slots = torch.full((max(n, 1) * stride,), FILL, dtype=torch.uint8, device=DEV)
    flen = torch.full((max(n, 1),), -77, dtype=torch.int32, device=DEV)
    eng.set_compression_level(level)
    eng.set_block_checksum(checksum)
    try:
        eng.compress_hcdict_device(hd, _t(buf), n, mx, slots, stride, flen, header_kind=kind, src_off=_t(np.array(off + [0], dtype=np.int64)),
                                   src_len=_t(np.array([len(b) for b in blocks] if lens is None else lens, dtype=np.int32)), block_stride=0)
        eng.synchronize()
    finally:
        eng.set_block_checksum(False)
    fl, hb = flen.cpu().tolist()[:n], slots.cpu().numpy()
    return fl, [hb[i * stride:i * stride + max(fl[i], 0)].tobytes() for i in range(n)], hb.reshape(max(n, 1), stride)


def payloads(S, eng, hd, blocks, level):
    fl, got, _ = hc_call(S, eng, hd, blocks, level)
    for f, g, b in zip(fl, got, blocks):
        assert f == len(g) and int.from_bytes(g[:4], "little") == f - 8 and int.from_bytes(g[4:8], "little") == len(b)
    return [g[8:] for g in got]


def batch_call(S, eng, data, offs, lens, level, linked):
    """compress_batch_device over the ranges of `data`: [block payloads] (headers of kind 8 stripped)"""
    import torch
    n, mx = len(lens), max(list(lens) + [1])
    stride = S.slot_stride_ex(mx, 8, False)
    slots = torch.full((n * stride,), FILL, dtype=torch.uint8, device=DEV)
    flen = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    eng.set_compression_level(level)
    eng.set_linked_compress(linked)
    try:
        eng.compress_batch_device(_bytes_t(data), n, mx, slots, stride, flen, header_kind=8, src_off=_t(np.array(offs, dtype=np.int64)),
                                  src_len=_t(np.array(lens, dtype=np.int32)), block_stride=0)
        eng.synchronize()
    finally:
        eng.set_linked_compress(False)
    fl, hb = flen.cpu().tolist(), slots.cpu().numpy()
    return [hb[i * stride + 8:i * stride + fl[i]].tobytes() for i in range(n)]


def linked_second_block(S, eng, dictionary, block, level):
    """block 1 of the linked call [D[-65536:], B] laid contiguously; with D empty, compress_batch_device's block at that level"""
    kept = dictionary[-65536:] if dictionary else b""
    if not kept:
        return batch_call(S, eng, block, [0], [len(block)], level, False)[0]
    return batch_call(S, eng, kept + block, [0, len(kept)], [len(kept), len(block)], level, True)[1]


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


# ---- 1. the grid ------------------------------------------------------------------------------------------------------------------
GRID_RUNS = [(1, 8, False), (1, 4, False), (3, 8, False), (3, 4, False), (9, 8, False), (9, 4, False), (9, 8, True), (9, 4, True)]


@pytest.mark.parametrize("dl", DC.DICT_LENS)
def test_grid(setup, oracle, dl):
    """one call carries every block length: each block is a valid LZ4 block for `keep` bytes of dictionary and decodes to its
    source through decompress_dict_device and through the oracle, at levels 1, 3 and 9, both header kinds, trailers off and on"""
    S, eng, hd = setup
    D = DC.dictionary(dl)
    keep = min(dl, 65536)
    load(eng, hd, D)
    dict_t = _bytes_t(D)
    blocks = [DC.block(bl) for bl in DC.BLOCK_LENS]
    sizes = list(DC.BLOCK_LENS)
    for level, kind, checksum in GRID_RUNS:
        fl, got, _ = hc_call(S, eng, hd, blocks, level, kind, checksum, maxlen=MAXLEN)
        trailer = 4 if checksum else 0
        for i, n in enumerate(sizes):
            comp = got[i][kind:len(got[i]) - trailer]
            assert fl[i] == kind + len(comp) + trailer and int.from_bytes(got[i][:4], "little") == len(comp), (dl, n, level, kind)
            if kind == 8:
                assert int.from_bytes(got[i][4:8], "little") == n
            lz4_check.check_block(comp, n, dict_len=keep)
            assert oracle.decompress_block(comp, n, D[-65536:]) == (n, blocks[i]), (dl, n, level, kind)
        eng.set_block_checksum(checksum)
        try:
            r, outs = decode_on_device(eng, got, sizes, dict_t, dl, kind)
        finally:
            eng.set_block_checksum(False)
        assert r == sizes and outs == blocks, (dl, level, kind, checksum, r)


def test_bad_length_is_framed_len_zero(setup):
    """a length outside 0..maxBlockLen: framedLen 0 for that block, its slot keeps its fill pattern, the others are unaffected"""
    S, eng, hd = setup
    load(eng, hd, DC.dictionary(4095))
    blocks = [DC.block(bl) for bl in DC.BLOCK_LENS]
    good = payloads(S, eng, hd, blocks, 3)
    lens = [len(b) for b in blocks]
    lens[3], lens[6] = -1, MAXLEN + 1
    fl, got, slots = hc_call(S, eng, hd, blocks, 3, lens=lens, maxlen=MAXLEN)
    for i in range(len(blocks)):
        if i in (3, 6):
            assert fl[i] == 0 and (slots[i] == FILL).all()
        else:
            assert got[i][8:] == good[i]


# ---- 2. byte identity with the linked path ------------------------------------------------------------------------------------------
ID_BLOCKS = (13, 64, 1000, 4096, 65536, 100000)


@pytest.mark.parametrize("level", [1, 9])
@pytest.mark.parametrize("dl", [0, 3, 4, 100, 4095, 65535, 65536, 70000])
def test_bytes_are_the_linked_call_s_second_block(setup, dl, level):
    S, eng, hd = setup
    D = DC.dictionary(dl)
    load(eng, hd, D)
    blocks = [DC.block(bl) for bl in ID_BLOCKS]
    got = payloads(S, eng, hd, blocks, level)
    for b, g in zip(blocks, got):
        assert g == linked_second_block(S, eng, D, b, level), (dl, len(b), level)


# ---- 3. the seam, hand-built from seeded random bytes: one possible candidate each ------------------------------------------------------
@pytest.mark.parametrize("level", [1, 9])
def test_seam_match_runs_from_the_dictionary_into_the_block(setup, oracle, level):
    """(a) D ends with 20 bytes X, B = X X X + 20 random bytes: the first match starts in the dictionary (offset 20 at output position
    0) and is 60 bytes long -- it runs over the dictionary's end into the block's own bytes"""
    S, eng, hd = setup
    X = rnd(1, 20)
    D, B = rnd(2, 1000) + X, X + X + X + rnd(3, 20)
    load(eng, hd, D)
    comp = payloads(S, eng, hd, [B], level)[0]
    assert lz4_check.check_block(comp, len(B), dict_len=len(D))[3] == 1, "one match reaches into the dictionary"
    assert sequences(comp)[0] == (0, 0, 20, 60)
    assert oracle.decompress_block(comp, len(B), D) == (len(B), B)
    assert comp == linked_second_block(S, eng, D, B, level)


@pytest.mark.parametrize("level", [1, 9])
def test_seam_positions_are_inserted(setup, oracle, level):
    """(b) D ends with the bytes ab; B = 30 bytes C + filler + ab + C + a tail.  The four bytes ab C0 C1 at the dictionary's
    second-last position lie across the seam, so that position is not in the prepared image: the match at the second ab -- 32
    bytes from the dictionary's second-last byte, offset = output position + 2 -- exists only if the kernel inserts it per block"""
    S, eng, hd = setup
    ab, Cc = rnd(11, 2), rnd(12, 30)
    D = rnd(13, 500) + ab
    B = Cc + rnd(14, 40) + ab + Cc + rnd(15, 20)
    load(eng, hd, D)
    comp = payloads(S, eng, hd, [B], level)[0]
    lz4_check.check_block(comp, len(B), dict_len=len(D))
    seqs = sequences(comp)
    assert (0, 70, 72, 32) in seqs, seqs
    assert oracle.decompress_block(comp, len(B), D) == (len(B), B)
    assert comp == linked_second_block(S, eng, D, B, level)


@pytest.mark.parametrize("level", [6, 9])      # (a chain holds every position of its hash BUCKET: 15 random ones here, beyond level 1's depth of 1)
def test_offset_65535_and_never_more(setup, oracle, level):
    """(c) a 65536-byte dictionary.  The chain ring holds 64 Ki positions, and a search in a round that has inserted up to rEnd looks
    no further back than rEnd - 65536 (encode_hc.hpp): offset 65535 can be found at a round's LAST position only.  So the bytes
    1024..1063 of D recur at the block's position 1023, the last of its first round of 1024: that match has offset 65535.  The
    layout with D's bytes 1..40 at position 0 is run too: at a round's first position the ring no longer holds window position 1,
    so that match is out of reach there.  In both blocks no offset is 0 or above 65535 (lz4_check), both decode, and both are the
    linked call's bytes."""
    S, eng, hd = setup
    D = rnd(21, 65536)
    B1 = rnd(22, 1023) + D[1024:1064] + rnd(23, 61)
    B2 = D[1:41] + rnd(24, 40)
    load(eng, hd, D)
    c1, c2 = payloads(S, eng, hd, [B1, B2], level)
    for comp, B in ((c1, B1), (c2, B2)):
        _, max_off, _, _ = lz4_check.check_block(comp, len(B), dict_len=65536)
        assert max_off <= 65535
        assert oracle.decompress_block(comp, len(B), D) == (len(B), B)
        assert comp == linked_second_block(S, eng, D, B, level)
    assert sequences(c1)[0] == (0, 1023, 65535, 40), sequences(c1)


def test_only_the_last_64k_of_a_long_dictionary_count(setup):
    """(d) a 200000-byte dictionary gives the bytes its last 65536 give"""
    S, eng, hd = setup
    D = DC.dictionary(200000)
    blocks = [DC.block(bl) for bl in (64, 1000, 4096, 65536)]
    load(eng, hd, D)
    whole, image = payloads(S, eng, hd, blocks, 9), hd.image()
    load(eng, hd, D[-65536:])
    assert payloads(S, eng, hd, blocks, 9) == whole and hd.image() == image
    assert any(lz4_check.check_block(c, len(b), dict_len=65536)[3] > 0 for c, b in zip(whole, blocks))


# ---- 4. the table image is restored between the blocks of a workgroup -----------------------------------------------------------------
def test_tables_are_restored_between_blocks(setup):
    """three blocks and more per workgroup: every block's bytes are those it gets in a call of its own, and the call repeats itself"""
    import torch
    S, eng, hd = setup
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * cus + 1
    rs = np.random.RandomState(5)
    blocks = [DC.text(300000 + i, int(rs.randint(1000, 4097))) for i in range(n)]
    load(eng, hd, DC.dictionary(65536))
    fl, got, _ = hc_call(S, eng, hd, blocks, 3, maxlen=4096)
    fl2, got2, _ = hc_call(S, eng, hd, blocks, 3, maxlen=4096)
    assert (fl2, got2) == (fl, got), "the same call gave other bytes the second time"
    pick = sorted({0, 1, n - 1, n - 2, cus - 1, cus, cus + 1, 2 * cus - 1, 2 * cus, 2 * cus + 1, 3 * cus - 1} | set(range(7, n, max(n // 30, 1))))
    for i in pick:
        assert got[i][8:] == payloads(S, eng, hd, [blocks[i]], 3)[0], "block %d of %d differs from its bytes in a call of its own" % (i, n)


# ---- 5. sharing and lifetime ------------------------------------------------------------------------------------------------------------
def test_object_keeps_its_own_copy_and_is_never_written(setup):
    import torch
    S, eng, hd = setup
    blocks = [DC.block(bl) for bl in (64, 1000, 4096)]
    D1, D2 = DC.dictionary(70000), DC.dictionary(4095)
    d = _bytes_t(D1)
    hd.load(d, len(D1))
    eng.synchronize()
    image = hd.image()
    assert len(image) == S.HcDict.IMAGE_BYTES
    first = payloads(S, eng, hd, blocks, 6)
    d.fill_(0)
    torch.cuda.synchronize()
    del d
    torch.cuda.empty_cache()
    assert payloads(S, eng, hd, blocks, 6) == first, "the object did not keep its own copy of the dictionary"
    assert hd.image() == image, "a compress call wrote the prepared dictionary"
    other = S.Engine(0)                       # another engine on the device may use the object
    try:
        assert payloads(S, other, hd, blocks, 6) == first
    finally:
        other.close()
    load(eng, hd, D2)
    second = payloads(S, eng, hd, blocks, 6)
    assert second != first and second == [linked_second_block(S, eng, D2, b, 6) for b in blocks]
    load(eng, hd, b"")
    assert len(hd) == 0
    assert payloads(S, eng, hd, blocks, 6) == [linked_second_block(S, eng, b"", b, 6) for b in blocks]


# ---- 6. the host form ---------------------------------------------------------------------------------------------------------------------
def test_host_form(setup):
    """compress_hcdict: the device call's blocks, densely framed; a bad length is E_ARG and nothing is written"""
    S, eng, hd = setup
    load(eng, hd, DC.dictionary(65536))
    eng.set_batch_blocks(64)                  # (sizes the stream combinators' batches; this call's groups are cut by input bytes: the next test)
    try:
        rs = np.random.RandomState(9)
        blocks = [DC.text(400000 + i, int(rs.randint(0, 3000))) for i in range(200)]
        want = payloads(S, eng, hd, blocks, 3)
        eng.set_compression_level(3)
        framed, flen = eng.compress_hcdict(blocks, hd)
        dense = b"".join(len(w).to_bytes(4, "little") + len(b).to_bytes(4, "little") + w for w, b in zip(want, blocks))
        assert flen == [8 + len(w) for w in want] and framed == dense
        # a bad length: checked on the host, nothing enqueued, nothing written
        out = np.full(4096, FILL, dtype=np.uint8)
        fl, st = np.full(2, -77, dtype=np.int32), np.full(2, -77, dtype=np.int32)
        src = np.frombuffer(blocks[0] + bytes(16), dtype=np.uint8)
        ptrs = (C.POINTER(C.c_uint8) * 2)(src.ctypes.data_as(C.POINTER(C.c_uint8)), src.ctypes.data_as(C.POINTER(C.c_uint8)))
        for bad in (-1, (4 << 20) + 1):
            lens = np.array([8, bad], dtype=np.int32)
            got = C.c_size_t(99)
            rc = S.lib.mi355lz4_compress_hcdict(eng.ctx, hd._h, ptrs, lens.ctypes.data_as(_i32p), 2, 8, out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                out.size, C.byref(got), fl.ctypes.data_as(_i32p), st.ctypes.data_as(_i32p))
            assert rc == E_ARG and got.value == 0 and b"compress_hcdict" in S.lib.mi355lz4_last_error()
            assert (out == FILL).all() and (fl == -77).all() and (st == -77).all()
    finally:
        eng.set_batch_blocks(4096)


def test_host_form_of_more_than_one_group(setup):
    """The host pipeline cuts a call into groups of 64 MiB of input and runs consecutive groups on two compute streams, each with a
    staging scratch of its own: 17 records of 4 MiB (rotations of one text, level 1) are two groups; the blocks are the device call's"""
    S, eng, hd = setup
    load(eng, hd, DC.dictionary(65536))
    base = np.frombuffer(DC.text(450000, 4 << 20), dtype=np.uint8)
    blocks = [np.roll(base, 1000 * i + 1).tobytes() for i in range(17)]
    eng.set_compression_level(1)
    framed, flen = eng.compress_hcdict(blocks, hd)
    want = payloads(S, eng, hd, blocks[:1] + blocks[15:], 1)
    off = np.cumsum([0] + flen)
    for k, i in enumerate((0, 15, 16)):
        assert framed[off[i] + 8:off[i + 1]] == want[k], "block %d" % i
    assert len(framed) == off[-1]


# ---- 7. argument errors on a live engine ----------------------------------------------------------------------------------------------------
def test_arguments(setup):
    """every error of the device calls on a live engine; nothing is enqueued: the outputs keep their pattern and the image its bytes"""
    import torch
    S, eng, hd = setup
    L, P = S.lib, S._dptr
    D = DC.dictionary(100)
    load(eng, hd, D)
    image = hd.image()
    d = _bytes_t(D)
    for args in ((None, hd._h, P(d), 100), (eng.ctx, None, P(d), 100), (eng.ctx, hd._h, P(d), -1), (eng.ctx, hd._h, None, 5)):
        assert L.mi355lz4_hcdict_load(*args) == E_ARG, args
        assert b"hcdict_load" in L.mi355lz4_last_error()
    assert len(hd) == 100
    blocks = [DC.block(bl) for bl in (64, 1000)]
    buf, off = spaced(blocks)
    src, so, sl = _t(buf), _t(np.array(off, dtype=np.int64)), _t(np.array([64, 1000], dtype=np.int32))
    stride = S.slot_stride_ex(1000, 8, False)
    slots = torch.full((2 * stride,), FILL, dtype=torch.uint8, device=DEV)
    flen = torch.full((2,), -77, dtype=torch.int32, device=DEV)

    def comp(ctx=eng.ctx, h=hd._h, src=src, nb=2, kind=8, mx=1000, slots=slots, stride=stride, flen=flen):
        return L.mi355lz4_compress_hcdict_device(ctx, h, P(src), P(so), P(sl), 0, mx, nb, kind, P(slots), stride, P(flen))

    eng.set_compression_level(9)
    try:
        for kw in (dict(ctx=None), dict(h=None), dict(nb=-1), dict(kind=5), dict(mx=-1), dict(mx=(4 << 20) + 1, stride=8 << 20),
                   dict(src=None), dict(slots=None), dict(flen=None)):
            assert comp(**kw) == E_ARG, kw
            assert b"compress_hcdict_device" in L.mi355lz4_last_error(), kw
        need = S.compress_bound(1000) + 8         # (slot_stride_ex rounds up: the bound itself is the limit)
        assert comp(stride=need - 1) == E_CAPACITY and b"compress_hcdict_device" in L.mi355lz4_last_error()
        eng.set_block_checksum(True)
        assert comp(stride=need + 3) == E_CAPACITY, "the trailer counts in the bound"
        eng.set_block_checksum(False)
        eng.set_compression_level(0)
        assert comp() == E_ARG and b"mi355lz4_compress_dict_device" in L.mi355lz4_last_error()
        if torch.cuda.device_count() > 1:       # an object created on another device
            far = S.Engine(1)
            hd2 = S.HcDict(far)
            try:
                eng.set_compression_level(9)
                assert comp(h=hd2._h) == E_ARG and b"device" in L.mi355lz4_last_error()
                assert L.mi355lz4_hcdict_load(eng.ctx, hd2._h, P(d), 100) == E_ARG
            finally:
                hd2.close()
                far.close()
        eng.set_compression_level(9)
        assert comp(nb=0, src=None, slots=None, flen=None) == 0
        eng.synchronize()
        assert (slots == FILL).all() and (flen == -77).all()
        assert hd.image() == image
        assert comp() == 0
        eng.synchronize()
        fl = flen.cpu().tolist()
        hb = slots.cpu().numpy()
        assert [hb[i * stride + 8:i * stride + fl[i]].tobytes() for i in range(2)] == payloads(S, eng, hd, blocks, 9)
    finally:
        eng.set_block_checksum(False)
        eng.set_compression_level(0)


# ---- 8. ratio ---------------------------------------------------------------------------------------------------------------------------------
def _liblz4_hc_dict():
    for name in ("liblz4.so.1", ctypes.util.find_library("lz4")):
        if not name:
            continue
        try:
            L = C.CDLL(name)
        except OSError:
            continue
        if all(hasattr(L, f) for f in ("LZ4_createStreamHC", "LZ4_freeStreamHC", "LZ4_resetStreamHC_fast", "LZ4_loadDictHC", "LZ4_compress_HC_continue")):
            L.LZ4_createStreamHC.restype = C.c_void_p
            L.LZ4_freeStreamHC.argtypes = [C.c_void_p]
            L.LZ4_resetStreamHC_fast.argtypes = [C.c_void_p, C.c_int]
            L.LZ4_resetStreamHC_fast.restype = None
            L.LZ4_loadDictHC.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
            L.LZ4_compress_HC_continue.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int]
            return L
    return None


RATIO_RECORDS = ((1000, 256), (4096, 256), (65536, 16))


@pytest.mark.parametrize("dl", [65536, 4095])
def test_ratio(setup, record, dl):
    """level 9 with the dictionary against level 1, against level 0's dictionary batch (0.92: liblz4's HC9+dict / fast+dict on these
    inputs is 0.827..0.861, times the 1.03 this engine is allowed against liblz4's HC, is at most 0.887, plus slack) and, where
    liblz4 has LZ4_loadDictHC, against LZ4_resetStreamHC_fast(9) + LZ4_loadDictHC + LZ4_compress_HC_continue per record (1.03,
    tests/test_hc_compress_gpu.py::test_ratio's bound)"""
    import torch
    S, eng, hd = setup
    D = DC.dictionary(dl)
    load(eng, hd, D)
    groups = [[DC.text(700000 + i, n) for i in range(cnt)] for n, cnt in RATIO_RECORDS]
    rec, tot = {"dict": dl}, {1: 0, 9: 0, 0: 0}
    for (n, cnt), blocks in zip(RATIO_RECORDS, groups):
        for lv in (1, 9):
            size = sum(len(p) for p in payloads(S, eng, hd, blocks, lv))
            rec["hcdict_level%d_%d" % (lv, n)] = size
            tot[lv] += size
    # level 0: mi355lz4_compress_dict_device on the same records
    eng.set_compression_level(0)
    cs = S.CompressStreams(eng, 1)
    try:
        d = _bytes_t(D)
        cs.load_dict(0, d, dl)
        for (n, cnt), blocks in zip(RATIO_RECORDS, groups):
            buf, off = spaced(blocks)
            stride = S.slot_stride_ex(n, 8, False)
            slots = torch.zeros(cnt * stride, dtype=torch.uint8, device=DEV)
            flen = torch.zeros(cnt, dtype=torch.int32, device=DEV)
            eng.compress_dict_device(cs, 0, _t(buf), cnt, n, slots, stride, flen, accel=1, header_kind=8,
                                     src_off=_t(np.array(off, dtype=np.int64)), src_len=_t(np.array([n] * cnt, dtype=np.int32)), block_stride=0)
            eng.synchronize()
            size = int(flen.sum().item()) - 8 * cnt
            rec["dict_level0_%d" % n] = size
            tot[0] += size
    finally:
        cs.close()
    rec.update({"hcdict_level1": tot[1], "hcdict_level9": tot[9], "dict_level0": tot[0]})
    L = _liblz4_hc_dict()
    ref = None
    if L is not None:
        st = L.LZ4_createStreamHC()
        dst = C.create_string_buffer(65536 + 65536 // 255 + 16)
        ref = 0
        for blocks in groups:
            for b in blocks:
                L.LZ4_resetStreamHC_fast(st, 9)
                L.LZ4_loadDictHC(st, D, len(D))
                r = L.LZ4_compress_HC_continue(st, b, dst, len(b), len(dst))
                assert r > 0
                ref += r
        L.LZ4_freeStreamHC(st)
        rec["liblz4_hc9_dict"] = ref
    print("hcdict ratio:", rec)
    record("hcdict_ratio", rec)
    assert tot[9] <= tot[1], rec
    assert tot[9] <= 0.92 * tot[0], rec
    if ref is not None:
        assert tot[9] <= 1.03 * ref, rec
