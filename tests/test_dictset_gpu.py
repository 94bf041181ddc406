"""Dictionary sets: a batch in which every block names its dictionary -- mi355lz4_compress_fastdict_multi_device /
mi355lz4_compress_fastdict_multi and mi355lz4_decompress_dict_multi_device / mi355lz4_decompress_dict_multi.

The contract needs no CPU codec on the compress side: block i is what mi355lz4_compress_fastdict_device writes for it against the
member it names (which tests/test_fastdict_gpu.py holds to the linked call), and -1 is that call against an object that holds the
empty dictionary.  The single-dictionary call is made once per member, accel, header kind and checksum switch over all blocks, and
the result is shared and never changed.  The decode side is held to mi355lz4_decompress_dict_device per member and to the golden the
reference wrote (tests/golden/dict_vectors.json)."""
import ctypes as C
import hashlib
import json
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
E_ARG = -3
BLK_E_DICT = -0x7F000006
APART = 7                     # sources and outputs lie 7 bytes apart: every alignment occurs
FILL = 0xA5
KNOB = "MI355LZ4_FASTDICT_WAVES"
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)

DICT_LENS = (0, 3, 100, 4095, 65535, 65536, 70000)          # member k holds DC.dictionary(DICT_LENS[k]): other text per member
BLOCK_LENS = (0, 1, 12, 13, 64, 1000, 4096)
COPIES = 3                                                  # blocks per length, each with text of its own
NONE = -1


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bytes_t(b):
    """bytes on the device (one byte at least, so that the tensor has a pointer)"""
    return _t(np.frombuffer(bytes(b) + b"\x00", dtype=np.uint8).copy())


def sha(b):
    return hashlib.sha256(b).hexdigest()


def spaced(datas, lead=3):
    off, pos = [], lead
    for d in datas:
        off.append(pos)
        pos += len(d) + APART
    buf = np.full(pos + 64, FILL, dtype=np.uint8)
    for o, d in zip(off, datas):
        buf[o:o + len(d)] = np.frombuffer(bytes(d), dtype=np.uint8)
    return buf, off


BLOCKS = [DC.text(700000 + 10 * bl + c, bl) for bl in BLOCK_LENS for c in range(COPIES)]
NB = len(BLOCKS)


class World:
    """the engine, one loaded HcDict per dictionary length, one that holds the empty dictionary, and the set over the loaded ones"""

    def __init__(self, S):
        self.S = S
        self.eng = S.Engine(0)
        self.members = []
        for dl in DICT_LENS:
            hd = S.HcDict(self.eng)
            hd.load(_bytes_t(DC.dictionary(dl)), dl)
            self.members.append(hd)
        self.empty = S.HcDict(self.eng)                     # never loaded: what -1 stands for
        self.eng.synchronize()
        self.ds = S.DictSet(self.eng, self.members)
        self.kept = [DC.dictionary(dl)[-65536:] for dl in DICT_LENS]
        self._single = {}

    def member(self, k):
        return self.empty if k == NONE else self.members[k]

    def kept_of(self, k):
        return b"" if k == NONE else self.kept[k]

    def call(self, hd_or_ds, blocks, idx=None, accel=1, kind=8, checksum=False, lens=None, maxlen=None, waves=None):
        """one compress_fastdict_device (idx None) or compress_fastdict_multi_device call over `blocks`, APART bytes apart:
        (framedLen[], [slot bytes up to framedLen], all slots as rows)"""
        import torch
        S, eng = self.S, self.eng
        n = len(blocks)
        mx = max([len(b) for b in blocks] + [1]) if maxlen is None else maxlen
        buf, off = spaced(blocks)
        stride = S.slot_stride_ex(mx, kind, checksum)
        slots = torch.full((max(n, 1) * stride,), FILL, dtype=torch.uint8, device=DEV)
        flen = torch.full((max(n, 1),), -77, dtype=torch.int32, device=DEV)
        eng.set_compression_level(0)
        eng.set_block_checksum(checksum)
        os.environ.pop(KNOB, None)
        if waves is not None:
            os.environ[KNOB] = str(waves)
        kw = dict(accel=accel, header_kind=kind, src_off=_t(np.array(off + [0], dtype=np.int64)),
                  src_len=_t(np.array([len(b) for b in blocks] if lens is None else lens, dtype=np.int32)), block_stride=0)
        try:
            if idx is None:
                eng.compress_fastdict_device(hd_or_ds, _t(buf), n, mx, slots, stride, flen, **kw)
            else:
                eng.compress_fastdict_multi_device(hd_or_ds, _t(np.array(list(idx) + [0], dtype=np.int64).astype(np.int32)), _t(buf), n, mx,
                                                   slots, stride, flen, **kw)
            eng.synchronize()
        finally:
            eng.set_block_checksum(False)
            os.environ.pop(KNOB, None)
        fl, hb = flen.cpu().tolist()[:n], slots.cpu().numpy()
        return fl, [hb[i * stride:i * stride + max(fl[i], 0)].tobytes() for i in range(n)], hb.reshape(max(n, 1), stride)

    def single(self, k, accel, kind, checksum):
        """member k's framed blocks for all of BLOCKS by the single-dictionary call (maxBlockLen 4096): computed once"""
        key = (k, accel, kind, checksum)
        if key not in self._single:
            fl, got, _ = self.call(self.member(k), BLOCKS, None, accel, kind, checksum)
            assert all(f > kind for f in fl)
            self._single[key] = tuple(got)
        return self._single[key]

    def close(self):
        os.environ.pop(KNOB, None)
        self.ds.close()
        for hd in self.members + [self.empty]:
            hd.close()
        self.eng.close()


@pytest.fixture(scope="module")
def world():
    import streamly_lz4_amd as S
    w = World(S)
    yield w
    w.close()


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "dict_vectors.json")) as f:
        return json.load(f)


# ---- compress equals the single call ---------------------------------------------------------------------------------------------
NM = len(DICT_LENS)
ARRANGEMENTS = {
    "sorted": sorted((i * NM // NB) for i in range(NB)),
    "reversed": sorted(((i * NM // NB) for i in range(NB)), reverse=True),
    "round-robin": [i % NM for i in range(NB)],
    "random": np.random.RandomState(20261020).randint(0, NM, size=NB).tolist(),
    "all one member": [3] * NB,
    "every block another member": None,                     # (a set of NB entries, below)
    "some members unused": [(1, 4, 6)[i % 3] for i in range(NB)],
    "-1 mixed in": [(NONE if i % 4 == 1 else i % NM) for i in range(NB)],
    "the same object at two indices": None,                 # (a set that lists member 5 twice, below)
}


@pytest.mark.parametrize("name", list(ARRANGEMENTS))
def test_multi_is_the_single_call_per_member(world, name):
    """every arrangement with the grid at its default and at one, two and three waves (one wave across many members, range ends on
    and inside a group, nBlocks no multiple of the grid), accel 1 and 7, both headers, checksums on and off"""
    w = world
    ds, idx, member_of = w.ds, ARRANGEMENTS[name], list(range(NM))
    if name == "every block another member":
        member_of = [i % NM for i in range(NB)]
        ds = w.S.DictSet(w.eng, [w.members[k] for k in member_of])
        idx = list(range(NB))
    elif name == "the same object at two indices":
        member_of = [5, 2, 5, 6]
        ds = w.S.DictSet(w.eng, [w.members[k] for k in member_of])
        idx = [i % 4 for i in range(NB)]
    assert len(ds) == len(member_of)
    try:
        for accel in (1, 7):
            for kind in (8, 4):
                for checksum in (False, True):
                    want = [w.single(NONE if k == NONE else member_of[k], accel, kind, checksum)[i] for i, k in enumerate(idx)]
                    for waves in (None, -1, -2, -3):
                        fl, got, _ = w.call(ds, BLOCKS, idx, accel, kind, checksum, waves=waves)
                        assert fl == [len(x) for x in want], (name, accel, kind, checksum, waves)
                        assert got == want, (name, accel, kind, checksum, waves)
    finally:
        if ds is not w.ds:
            ds.close()


def test_every_block_is_valid_and_round_trips_with_its_member(world, oracle):
    """the multi call's blocks pass the strict validator against their member's kept bytes, decode on the CPU with them, and come
    back through decompress_dict_multi_device with the same indices"""
    w = world
    idx = ARRANGEMENTS["-1 mixed in"]
    for accel in (1, 7):
        fl, got, _ = w.call(w.ds, BLOCKS, idx, accel)
        for g, b, k in zip(got, BLOCKS, idx):
            kept = w.kept_of(k)
            assert int.from_bytes(g[:4], "little") == len(g) - 8 and int.from_bytes(g[4:8], "little") == len(b)
            lz4_check.check_block(g[8:], len(b), dict_len=len(kept))
            assert oracle.decompress_block(g[8:], len(b), kept if kept else None) == (len(b), b)
        r, outs, clean = decode_multi(w, w.ds, [(g[8:], len(b)) for g, b in zip(got, BLOCKS)], idx, 8)
        assert r == [len(b) for b in BLOCKS] and outs == BLOCKS and clean


def test_a_block_above_64k_takes_the_other_encoder_form(world):
    """maxBlockLen > 65536: one wave per window step; the same equality, the grid at its default and at one wave"""
    w = world
    blocks = [DC.text(710000, 100000), DC.text(710001, 1000), DC.text(710002, 4096), DC.text(710003, 13), DC.text(710004, 70000)]
    idx = [6, 2, NONE, 5, 4]
    want = []
    for b, k in zip(blocks, idx):
        fl, got, _ = w.call(w.member(k), [b], None, maxlen=100000)
        want.append(got[0])
    for waves in (None, -1, -2):
        fl, got, _ = w.call(w.ds, blocks, idx, maxlen=100000, waves=waves)
        assert got == want, waves
    for g, b, k in zip(want, blocks, idx):
        lz4_check.check_block(g[8:], len(b), dict_len=len(w.kept_of(k)))


def test_restaging_leaves_nothing_of_the_member_before(world, oracle):
    """One wave walks, in this order: no dictionary (-1 sorts first), a 65536-byte member, a 100-byte member, a member that holds the
    empty dictionary, a 3-byte member, the 65536-byte member again and a second 65536-byte member with other content.  Every block
    repeats text of the member BEFORE its own, so a window that still showed it would give matches the single call does not make."""
    w = world
    S, eng = w.S, w.eng
    texts = [DC.text(720000, 65536), DC.text(720001, 100), b"", DC.text(720003, 3), None, DC.text(720005, 65536)]
    texts[4] = texts[0]
    hds = []
    for t in texts[:4] + [None, texts[5]]:
        if t is None:
            hds.append(hds[0])                              # the same object again
            continue
        hd = S.HcDict(eng)
        if t:
            hd.load(_bytes_t(t), len(t))
        hds.append(hd)
    eng.synchronize()
    ds = S.DictSet(eng, hds)
    try:
        order = [NONE, 0, 1, 2, 3, 4, 5]
        blocks, idx = [], []
        for pos, k in enumerate(order):
            earlier = [texts[j] for j in order[:pos] if j != NONE and texts[j]]
            before = earlier[-1] if earlier else texts[5]       # the last member in front of this one that staged any bytes
            own = texts[k] if k != NONE else b""
            for c in range(2):
                blocks.append((before[-1500 - 100 * c:] + own[-700:] + before[:800])[:4096])
                idx.append(k)
        shuffle = np.random.RandomState(3).permutation(len(blocks)).tolist()       # (call order is not run order: the pass groups)
        blocks, idx = [blocks[i] for i in shuffle], [idx[i] for i in shuffle]
        want = []
        for b, k in zip(blocks, idx):
            fl, got, _ = w.call(w.empty if k == NONE else hds[k], [b], None, maxlen=4096)
            want.append(got[0])
        fl, got, _ = w.call(ds, blocks, idx, maxlen=4096, waves=-1)
        assert got == want
        assert ds.last() == (len(order), 1), "one wave, one staging per member it met"
        for g, b, k in zip(got, blocks, idx):
            kept = b"" if k == NONE else texts[k]
            lz4_check.check_block(g[8:], len(b), dict_len=len(kept))
            assert oracle.decompress_block(g[8:], len(b), kept if kept else None) == (len(b), b)
        # the same across calls, where -1 can stand anywhere: the one wave of every call gets the window the call before left, in the
        # order 65536 bytes, 100 bytes, none, 3 bytes, the 65536 bytes again, the other 65536 bytes
        for k in (0, 1, NONE, 3, 4, 5):
            mine = [i for i in range(len(blocks)) if idx[i] == k]
            fl, got, _ = w.call(ds, [blocks[i] for i in mine], [k] * len(mine), maxlen=4096, waves=-1)
            assert got == [want[i] for i in mine], k
            assert ds.last() == (1, 1)
    finally:
        ds.close()
        for hd in set(hds):
            hd.close()


@pytest.mark.parametrize("waves", [None, -2])
def test_bad_entries_are_skipped_and_their_neighbours_exact(world, waves):
    """an index outside -1..n-1 and a length outside 0..maxBlockLen: framedLen 0, the slot's fill intact, every other block exact"""
    w = world
    idx = list(ARRANGEMENTS["round-robin"])
    lens = [len(b) for b in BLOCKS]
    bad = {2: NM, 5: -2, 9: INT32_MAX, 13: INT32_MIN}
    for i, v in bad.items():
        idx[i] = v
    lens[16], lens[19] = -1, 4097
    dead = set(bad) | {16, 19}
    fl, got, rows = w.call(w.ds, BLOCKS, idx, lens=lens, maxlen=4096, waves=waves)
    for i in range(NB):
        if i in dead:
            assert fl[i] == 0 and (rows[i] == FILL).all(), i
        else:
            assert got[i] == w.single(idx[i], 1, 8, False)[i], i


def test_host_forms(world):
    """compress_fastdict_multi is the device call's slots compacted, decompress_dict_multi brings the records back, a bad index is
    E_ARG with nothing written"""
    w = world
    S, eng, L = w.S, w.eng, w.S.lib
    idx = ARRANGEMENTS["-1 mixed in"]
    for kind in (8, 4):
        fl, got, _ = w.call(w.ds, BLOCKS, idx, 7, kind)
        framed, hfl = eng.compress_fastdict_multi(BLOCKS, w.ds, idx, accel=7, header_kind=kind)
        assert hfl == fl and framed == b"".join(got)
    framed, hfl = eng.compress_fastdict_multi(BLOCKS, w.ds, idx)
    out, blen = eng.decompress_dict_multi(framed, w.ds, idx)
    assert blen == [len(b) for b in BLOCKS] and out == b"".join(BLOCKS)
    # a bad index: E_ARG in front of everything
    n = 3
    arrs = [np.frombuffer(b, dtype=np.uint8) for b in BLOCKS[-3:]]
    ptrs = (_u8p * n)(*[a.ctypes.data_as(_u8p) for a in arrs])
    lens = np.array([a.size for a in arrs], dtype=np.int32)
    for v in (NM, -2, INT32_MAX, INT32_MIN):
        bad = np.array([0, v, NONE], dtype=np.int32)
        dst = np.full(3 * 5000, FILL, dtype=np.uint8)
        ol = C.c_size_t(99)
        hf = np.full(n, -77, dtype=np.int32)
        rc = L.mi355lz4_compress_fastdict_multi(eng.ctx, w.ds._h, bad.ctypes.data_as(_i32p), ptrs, lens.ctypes.data_as(_i32p), n, 1, 8,
                                                dst.ctypes.data_as(_u8p), dst.size, C.byref(ol), hf.ctypes.data_as(_i32p), None)
        assert rc == E_ARG and ol.value == 0 and (dst == FILL).all() and (hf == -77).all(), v
        with pytest.raises(S.LZ4Error):
            eng.decompress_dict_multi(framed, w.ds, [0, v] + [NONE] * (NB - 2))
    lens[1] = -1
    ol = C.c_size_t(99)
    good = np.array([0, 1, NONE], dtype=np.int32)
    assert L.mi355lz4_compress_fastdict_multi(eng.ctx, w.ds._h, good.ctypes.data_as(_i32p), ptrs, lens.ctypes.data_as(_i32p), n, 1, 8,
                                              dst.ctypes.data_as(_u8p), dst.size, C.byref(ol), None, None) == E_ARG and ol.value == 0


def test_a_reload_is_seen_without_a_new_set(world):
    """hcdict_load on a member after the set was made: the next call gives the single call's bytes for the new dictionary"""
    w = world
    k = 3
    idx = [k if i % 2 else 6 for i in range(NB)]
    other = DC.text(730000, 30000)
    try:
        w.members[k].load(_bytes_t(other), len(other))
        w.eng.synchronize()
        fl, new_single, _ = w.call(w.members[k], BLOCKS, None)
        fl, got, _ = w.call(w.ds, BLOCKS, idx)
        assert got == [new_single[i] if i % 2 else w.single(6, 1, 8, False)[i] for i in range(NB)]
        assert new_single[-1] != w.single(k, 1, 8, False)[-1], "the reload changed nothing: the case shows nothing"
    finally:
        w.members[k].load(_bytes_t(DC.dictionary(DICT_LENS[k])), DICT_LENS[k])
        w.eng.synchronize()
    fl, got, _ = w.call(w.ds, BLOCKS, idx)
    assert got == [w.single(k if i % 2 else 6, 1, 8, False)[i] for i in range(NB)]


def test_the_staging_bound(world):
    """64 blocks, 8 members, 4 waves: at most grid + G - 1 = 11 stagings for shuffled indices, at most grid = 4 for equal ones"""
    w = world
    S, eng = w.S, w.eng
    hds = []
    for k in range(8):
        hd = S.HcDict(eng)
        hd.load(_bytes_t(DC.text(740000 + k, 4095)), 4095)
        hds.append(hd)
    eng.synchronize()
    ds = S.DictSet(eng, hds)
    try:
        blocks = [DC.text(741000 + i, 1000) for i in range(64)]
        idx = np.random.RandomState(8).randint(0, 8, size=64).tolist()
        assert len(set(idx)) == 8
        fl, got, _ = w.call(ds, blocks, idx, waves=-4)
        stagings, grid = ds.last()
        assert grid == 4 and 4 <= stagings <= 11, (stagings, grid)
        for k in range(8):
            mine = [i for i in range(64) if idx[i] == k]
            f1, g1, _ = w.call(hds[k], [blocks[i] for i in mine], None, maxlen=1000)
            assert [got[i] for i in mine] == g1, k
        fl, got, _ = w.call(ds, blocks, [5] * 64, waves=-4)
        stagings, grid = ds.last()
        assert grid == 4 and 1 <= stagings <= 4, (stagings, grid)
    finally:
        ds.close()
        for hd in hds:
            hd.close()


# ---- decode equals the single call -----------------------------------------------------------------------------------------------
def frame(blocks_caps, kind, trailer=False):
    from dstreams_model import xxh32
    framed, boff = bytearray(), []
    for blk, cap in blocks_caps:
        boff.append(len(framed))
        framed += len(blk).to_bytes(4, "little") + (int(cap).to_bytes(4, "little") if kind == 8 else b"") + bytes(blk)
        if trailer:
            framed += xxh32(bytes(blk)).to_bytes(4, "little")
    return framed, boff


def decode_multi(w, ds, blocks_caps, idx, kind, single=None, batch=False, framed_boff=None):
    """[(block, cap)] framed with `kind` headers, decoded into outputs APART bytes apart by decompress_dict_multi_device with idx --
    or, single = (dictionary tensor, length), by decompress_dict_device; batch: by decompress_batch_device.  (results, [bytes up to
    the capacity], whether every byte outside the outputs still holds FILL)"""
    import torch
    eng = w.eng
    framed, boff = framed_boff if framed_boff else frame(blocks_caps, kind)
    caps = [c for _, c in blocks_caps]
    ooff, pos = [], 5
    for c in caps:
        ooff.append(pos)
        pos += c + APART
    n = len(caps)
    out = torch.full((pos + 64,), FILL, dtype=torch.uint8, device=DEV)
    res = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    args = (_bytes_t(framed), len(framed), _t(np.array(boff, dtype=np.int64)), n)
    kw = dict(header_kind=kind, fixed_uncomp=max(caps) if kind == 4 else 0, out_cap=_t(np.array(caps, dtype=np.int32)) if kind == 4 else None)
    oo = _t(np.array(ooff, dtype=np.int64))
    if batch:
        eng.decompress_batch_device(*args, out, oo, res, linked=False, **kw)
    elif single is not None:
        eng.decompress_dict_device(*args, single[0], single[1], out, oo, res, **kw)
    else:
        eng.decompress_dict_multi_device(*args, ds, _t(np.array(list(idx) + [0], dtype=np.int64).astype(np.int32)), out, oo, res, **kw)
    eng.synchronize()
    hb, r = out.cpu().numpy(), res.cpu().tolist()
    keep = np.ones(hb.size, dtype=bool)
    for o, c in zip(ooff, caps):
        keep[o:o + c] = False
    return r, [hb[o:o + c].tobytes() for o, c in zip(ooff, caps)], bool((hb[keep] == FILL).all())


def test_decode_edges_in_one_call_across_two_members(world, vectors):
    """every hand-built block of dict_cases.decode_cases() in ONE call, each naming the member of its case's dictionary length (the
    cases interleaved across the 100- and the 70000-byte member): codes and bytes are decompress_dict_device's per member and the
    golden's"""
    w = world
    m100, m70000 = DICT_LENS.index(100), DICT_LENS.index(70000)
    cases = list(enumerate(DC.decode_cases()))
    a = [c for c in cases if c[1][1] == 100]
    b = [c for c in cases if c[1][1] == 70000]
    mixed = [c for pair in zip(a, b) for c in pair] + a[len(b):] + b[len(a):]
    assert len(mixed) == len(cases)
    idx = [m100 if c[1][1] == 100 else m70000 for c in mixed]
    assert idx[:4] == [m100, m70000, m100, m70000]
    bc = [(blk, cap) for _, (_, _, blk, cap) in mixed]
    r, outs, clean = decode_multi(w, w.ds, bc, idx, 4)
    assert clean, "bytes outside the outputs were written"
    for dl, m in ((100, m100), (70000, m70000)):
        d = DC.dictionary(dl)
        sel = [j for j, k in enumerate(idx) if k == m]
        r1, o1, _ = decode_multi(w, None, [bc[j] for j in sel], None, 4, single=(_bytes_t(d), dl))
        assert [r[j] for j in sel] == r1
        for j, code, dec in zip(sel, r1, o1):
            assert outs[j][:max(code, 0)] == dec[:max(code, 0)], mixed[j][1][0]
    for j, (i, (name, dl, blk, cap)) in enumerate(mixed):
        assert [name, dl, r[j], sha(outs[j][:max(r[j], 0)])] == vectors["decode"][i]
    assert any(x < 0 for x in r) and any(x > 0 for x in r)


def test_the_index_is_honoured(world):
    """the block whose first offset lies one byte in front of a 100-byte dictionary, once against each member: it fails on the
    100-byte member and decodes on the 70000-byte one"""
    w = world
    m100, m70000 = DICT_LENS.index(100), DICT_LENS.index(70000)
    (blk, cap), = [(b, c) for name, d, b, c in DC.decode_cases() if name == "offset one byte in front of the dictionary" and d == 100]
    r, outs, clean = decode_multi(w, w.ds, [(blk, cap)] * 4, [m100, m70000, m70000, m100], 8)
    assert clean and r[0] < 0 and r[3] < 0 and r[1] == cap and r[2] == cap and outs[1] == outs[2]
    r1, o1, _ = decode_multi(w, None, [(blk, cap)], None, 8, single=(_bytes_t(DC.dictionary(70000)), 70000))
    assert r1 == [cap] and o1[0] == outs[1]


def test_minus_one_is_decompress_batch_and_a_bad_index_writes_nothing(world):
    w = world
    fl, got, _ = w.call(w.ds, BLOCKS, [3] * NB)
    bc = [(g[8:], len(b)) for g, b in zip(got, BLOCKS)]                          # blocks that miss their dictionary, and some that need none
    for kind in (8, 4):
        a = decode_multi(w, w.ds, bc, [NONE] * NB, kind)
        b = decode_multi(w, None, bc, None, kind, batch=True)
        assert a[0] == b[0] and a[2] and b[2]
        for code, x, y in zip(a[0], a[1], b[1]):
            assert x[:max(code, 0)] == y[:max(code, 0)]
        assert any(c < 0 for c in a[0]) and any(c >= 0 for c in a[0])
        idx = [3] * NB
        bad = {1: NM, 4: -2, 10: INT32_MAX, 20: INT32_MIN}
        for i, v in bad.items():
            idx[i] = v
        r, outs, clean = decode_multi(w, w.ds, bc, idx, kind)
        assert clean
        for i in range(NB):
            if i in bad:
                assert r[i] == BLK_E_DICT and outs[i] == bytes([FILL]) * len(BLOCKS[i]), i
            else:
                assert r[i] == len(BLOCKS[i]) and outs[i] == BLOCKS[i], i


def test_checksum_trailers(world):
    """the compress call appends the trailers, the decode call verifies them: one flipped byte fails that block alone"""
    w = world
    idx = ARRANGEMENTS["round-robin"]
    fl, got, _ = w.call(w.ds, BLOCKS, idx, checksum=True)
    framed, boff = bytearray(), []
    for g in got:
        boff.append(len(framed))
        framed += g
    hit = NB - 1
    framed[boff[hit] + 8 + 5] ^= 0x40
    bc = [(g[8:-4], len(b)) for g, b in zip(got, BLOCKS)]
    w.eng.set_block_checksum(True)
    try:
        r, outs, clean = decode_multi(w, w.ds, bc, idx, 8, framed_boff=(framed, boff))
    finally:
        w.eng.set_block_checksum(False)
    assert clean and r[hit] == -0x7F000004
    assert r[:hit] == [len(b) for b in BLOCKS[:hit]] and outs[:hit] == BLOCKS[:hit]
