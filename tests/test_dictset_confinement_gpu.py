"""What the dictionary-set calls may write (include/mi355lz4.h, "what a call may write"), held with guard patterns around every
range the header grants (tests/guarded.py), as tests/test_dict_confinement_gpu.py does for the single-dictionary calls:
_compress_fastdict_multi_device the slot ranges of the blocks it does not skip and framedLen[0, nBlocks);
_decompress_dict_multi_device the blocks' output ranges -- nothing for a block whose index names no member -- and
result[0, nBlocks); neither an input, dictIdx or a byte of any member's two images."""
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

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLK_E_DICT = -0x7F000006
DICT_LENS = (100, 4095, 65536, 70000)
BLOCK_LENS = (0, 1, 12, 13, 64, 1000, 4096, 4096, 1000, 64, 13, 12)
MAXLEN = max(BLOCK_LENS)
KNOB = "MI355LZ4_FASTDICT_WAVES"


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_set(S, eng):
    hds = []
    for dl in DICT_LENS:
        hd = S.HcDict(eng)
        hd.load(_t(np.frombuffer(DC.dictionary(dl), dtype=np.uint8).copy()), dl)
        hds.append(hd)
    eng.synchronize()
    return hds, S.DictSet(eng, hds)


def images(hds):
    return [(hd.image(), hd.fast_image()) for hd in hds]


def single(S, eng, hd, block, checksum):
    """the framed block of the single-dictionary call with the same maxBlockLen"""
    import torch
    stride = S.slot_stride_ex(MAXLEN, 8, checksum)
    slots = torch.zeros(stride, dtype=torch.uint8, device=DEV)
    flen = torch.zeros(1, dtype=torch.int32, device=DEV)
    eng.compress_fastdict_device(hd, _t(np.frombuffer(block + b"\x00", dtype=np.uint8).copy()), 1, MAXLEN, slots, stride, flen,
                                 src_off=_t(np.zeros(1, dtype=np.int64)), src_len=_t(np.array([len(block)], dtype=np.int32)), block_stride=0)
    eng.synchronize()
    return slots.cpu().numpy()[:int(flen.item())].tobytes()


@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("extra", [0, 37])
@pytest.mark.parametrize("bad", [False, True])
@pytest.mark.parametrize("waves", [None, -2])
def test_compress_multi_call_is_confined(checksum, extra, bad, waves):
    import torch
    import streamly_lz4_amd as S
    blocks = [DC.text(750000 + i, bl) for i, bl in enumerate(BLOCK_LENS)]
    n = len(blocks)
    lens = [len(b) for b in blocks]
    idx = [(-1 if i % 5 == 4 else i % len(DICT_LENS)) for i in range(n)]
    dead = set()
    if bad:
        lens[2], lens[7] = -5, MAXLEN + 1
        idx[5], idx[9], idx[10] = len(DICT_LENS), -2, 2 ** 31 - 1
        dead = {2, 7, 5, 9, 10}
    need = S.slot_stride_ex(MAXLEN, 8, checksum)
    stride = need + extra
    lay_src = G.layout(lens_of(blocks))
    lay = G.layout([need] * n, stride=stride, first_residue=extra)
    eng = S.Engine(0)
    hds, ds = make_set(S, eng)
    os.environ.pop(KNOB, None)
    try:
        before = images(hds)
        eng.set_block_checksum(checksum)
        seed = 173
        buf = G.new_torch(lay.total, seed, DEV)
        flen = G.GuardedArray(n, torch.int32, seed + 50, DEV)
        src = _t(G.pair(lay_src, blocks)[0])
        off = _t(np.array(lay_src.starts, dtype=np.int64))
        ln = _t(np.array(lens, dtype=np.int32))
        di = _t(np.array(idx, dtype=np.int64).astype(np.int32))
        copies = [t.clone() for t in (src, off, ln, di)]
        if waves is not None:
            os.environ[KNOB] = str(waves)
        eng.compress_fastdict_multi_device(ds, di, src, n, MAXLEN, buf[lay.starts[0]:], stride, flen.view, accel=1, header_kind=8,
                                           src_off=off, src_len=ln, block_stride=0)
        eng.synchronize()
        torch.cuda.synchronize()
        os.environ.pop(KNOB, None)
        G.assert_confined(buf, [r for i, r in enumerate(lay.ranges()) if i not in dead], seed, "slots")
        flen.check(what="framedLen[]")
        for t, c in zip((src, off, ln, di), copies):
            assert torch.equal(t, c), "an input was written"
        assert images(hds) == before, "a member's image was written"
        fl, hb = flen.view.cpu().tolist(), buf.cpu().numpy()
        empty = S.HcDict(eng)
        try:
            for i in range(n):
                if i in dead:
                    assert fl[i] == 0
                    continue
                want = single(S, eng, empty if idx[i] < 0 else hds[idx[i]], blocks[i], checksum)
                assert fl[i] == len(want) and hb[lay.starts[i]:lay.starts[i] + len(want)].tobytes() == want, i
        finally:
            empty.close()
    finally:
        os.environ.pop(KNOB, None)
        ds.close()
        for hd in hds:
            hd.close()
        eng.close()


def lens_of(blocks):
    return [len(b) for b in blocks]


@pytest.mark.parametrize("kind", [8, 4])
def test_decompress_multi_call_is_confined(oracle, kind):
    """blocks that decode, blocks that fail in the decoder (the hand-built cases, a capacity too small), blocks whose header is
    rejected and blocks whose index names no member"""
    import torch
    import streamly_lz4_amd as S
    m = {dl: k for k, dl in enumerate(DICT_LENS)}
    cases = []                                               # (payload, cap, header override or None, index)
    for name, d, blk, cap in DC.decode_cases():
        cases.append((blk, cap, None, m[d]))
        cases.append((blk, cap + 37, None, m[d]))
        if cap > 40:
            cases.append((blk, cap - 23, None, m[d]))
    first = DC.decode_cases()[0]
    cases.append((first[2], first[3], 0, m[first[1]]))                           # compLen 0: rejected
    cases.append((first[2], first[3], len(first[2]) + (1 << 20), m[first[1]]))   # runs past the framed buffer: rejected
    for v in (len(DICT_LENS), -2, 2 ** 31 - 1, -2 ** 31):
        cases.append((first[2], first[3], None, v))
    cases.append((first[2], first[3], None, -1))
    n = len(cases)
    caps = [c for _, c, _, _ in cases]
    framed, boff = bytearray(), []
    for blk, cap, hdr, _ in cases:
        boff.append(len(framed))
        framed += int(len(blk) if hdr is None else hdr).to_bytes(4, "little", signed=True)
        if kind == 8:
            framed += int(cap).to_bytes(4, "little")
        framed += blk
    lay = G.layout(caps)
    eng = S.Engine(0)
    hds, ds = make_set(S, eng)
    try:
        before = images(hds)
        seed = 191
        out = G.new_torch(lay.total, seed, DEV)
        res = G.GuardedArray(n, torch.int32, seed + 7, DEV)
        fr = _t(np.frombuffer(bytes(framed), dtype=np.uint8).copy())
        bo, oo = _t(np.array(boff, dtype=np.int64)), _t(np.array(lay.starts, dtype=np.int64))
        di = _t(np.array([k for _, _, _, k in cases], dtype=np.int64).astype(np.int32))
        oc = _t(np.array(caps, dtype=np.int32)) if kind == 4 else None
        copies = [t.clone() for t in (fr, bo, oo, di)]
        eng.decompress_dict_multi_device(fr, len(framed), bo, n, ds, di, out, oo, res.view, header_kind=kind,
                                         fixed_uncomp=max(caps) if kind == 4 else 0, out_cap=oc)
        eng.synchronize()
        torch.cuda.synchronize()
        G.assert_confined(out, lay.ranges(), seed, "out")
        res.check(what="result[]")
        for t, c in zip((fr, bo, oo, di), copies):
            assert torch.equal(t, c), "an input was written"
        assert images(hds) == before, "a member's image was written"
        r, hb = res.view.cpu().tolist(), out.cpu().numpy()
        ok = fail = untouched = 0
        for i, (blk, cap, hdr, k) in enumerate(cases):
            start = lay.starts[i]
            if hdr is not None or k < -1 or k >= len(DICT_LENS):
                assert (r[i] <= -0x7F000000) if hdr is not None else (r[i] == BLK_E_DICT), (i, r[i])
                assert hb[start:start + cap].tobytes() == G.pattern(start, cap, seed).tobytes(), "a skipped block was written"
                untouched += 1
                continue
            code, dec = oracle.decompress_block(blk, cap, DC.dictionary(DICT_LENS[k]) if k >= 0 else None)
            assert r[i] == code, (i, code, r[i])
            if code >= 0:
                assert hb[start:start + code].tobytes() == dec
                ok += 1
            else:
                fail += 1
        assert ok >= 10 and fail >= 10 and untouched == 6, (ok, fail, untouched)
    finally:
        ds.close()
        for hd in hds:
            hd.close()
        eng.close()
