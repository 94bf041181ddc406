"""What the shared-dictionary calls may write (include/mi355lz4.h, "what a call may write"), held with guard patterns around every
range the header grants (tests/guarded.py), as tests/test_write_confinement_gpu.py does for the other calls:
_compress_dict_device the slot ranges and framedLen[0, nBlocks), never the set; _decompress_dict_device the blocks' output ranges
and result[0, nBlocks), never the dictionary; _cstreams_load_dict the slot it names."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dict_cases as DC  # noqa: E402
import dict_model as M  # noqa: E402
import guarded as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLK_E_COMPLEN = -0x7F000001
BLK_E_UNCOMPLEN = -0x7F000003
MAXLEN = max(DC.BLOCK_LENS)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded_dict(dl, seed):
    """the dictionary inside a guarded buffer: (buffer, the tensor view handed to the calls)"""
    lay = G.layout([dl])
    buf = _t(G.pair(lay, [DC.dictionary(dl)], seeds=(seed, seed + 1))[0])
    return buf, buf[lay.starts[0]:lay.starts[0] + max(dl, 1)]


@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("extra", [0, 37])
@pytest.mark.parametrize("bad", [False, True])
def test_compress_dict_call_is_confined(checksum, extra, bad):
    import torch
    import streamly_lz4_amd as S
    dl = 70000
    blocks = [DC.block(bl) for bl in DC.BLOCK_LENS]
    n = len(blocks)
    lens = [len(b) for b in blocks]
    dead = {2, 7} if bad else set()
    if bad:
        lens[2], lens[7] = -5, MAXLEN + 1
    need = S.slot_stride_ex(MAXLEN, 8, checksum)
    stride = need + extra
    lay_src = G.layout([len(b) for b in blocks])
    lay = G.layout([need] * n, stride=stride, first_residue=extra)
    eng = S.Engine(0)
    cs = S.CompressStreams(eng, 3)
    try:
        eng.set_block_checksum(checksum)
        dbuf, d = guarded_dict(dl, 31)
        cs.load_dict(1, d, dl)
        eng.synchronize()
        dcopy = dbuf.clone()
        state = [cs.slot_bytes(k) for k in range(3)]
        seed = 73
        buf = G.new_torch(lay.total, seed, DEV)
        flen = G.GuardedArray(n, torch.int32, seed + 50, DEV)
        src = _t(G.pair(lay_src, blocks)[0])
        off = _t(np.array(lay_src.starts, dtype=np.int64))
        ln = _t(np.array(lens, dtype=np.int32))
        copies = [t.clone() for t in (src, off, ln)]
        eng.compress_dict_device(cs, 1, src, n, MAXLEN, buf[lay.starts[0]:], stride, flen.view, accel=1, header_kind=8, src_off=off,
                                 src_len=ln, block_stride=0)
        eng.synchronize()
        torch.cuda.synchronize()
        G.assert_confined(buf, [r for i, r in enumerate(lay.ranges()) if i not in dead], seed, "slots")
        flen.check(what="framedLen[]")
        for t, c in zip((src, off, ln), copies):
            assert torch.equal(t, c), "an input was written"
        assert [cs.slot_bytes(k) for k in range(3)] == state, "the set was written"
        assert torch.equal(dbuf, dcopy)
        fl = flen.view.cpu().tolist()
        hb = buf.cpu().numpy()
        loaded = M.model_load(DC.dictionary(dl))
        for i, bl in enumerate(DC.BLOCK_LENS):
            if i in dead:
                assert fl[i] == 0
                continue
            code, comp = M.model_compress(loaded, blocks[i], 1)
            want = M.framed_block(code, comp, bl, 8)
            assert fl[i] == len(want) + (4 if checksum else 0)
            assert hb[lay.starts[i]:lay.starts[i] + len(want)].tobytes() == want, bl
    finally:
        cs.close()
        eng.close()


def decode_inputs(oracle, dl):
    """[(payload, cap, header override or None)]: blocks that decode (the model's, at exact and at larger capacities), blocks that
    fail in the decoder (a capacity too small, corrupted bytes, the hand-built error cases) and blocks whose header is rejected"""
    rng = random.Random(5)
    loaded = M.model_load(DC.dictionary(dl))
    out = []
    for bl in DC.BLOCK_LENS:
        comp = M.model_compress(loaded, DC.block(bl), 1)[1]
        out.append((comp, bl, None))
        out.append((comp, bl + 37, None))
        if bl >= 64:
            out.append((comp, bl - rng.randrange(1, 40), None))                  # too small: fails, having written up to cap
            bad = bytearray(comp)
            for _ in range(3):
                bad[rng.randrange(len(bad))] = rng.randrange(256)
            out.append((bytes(bad), bl, None))
            out.append((comp[:len(comp) - rng.randrange(1, 20)], bl, None))      # truncated
    for name, d, blk, cap in DC.decode_cases():
        if d == dl:
            out.append((blk, cap, None))
    comp = M.model_compress(loaded, DC.block(4096), 1)[1]
    out.append((comp, 4096, 0))                                                  # compLen 0: rejected
    out.append((comp, 4096, -3))
    out.append((comp, 4096, len(comp) + (1 << 20)))                              # runs past the framed buffer: rejected
    return out


@pytest.mark.parametrize("dl", [100, 70000])
@pytest.mark.parametrize("kind", [8, 4])
def test_decompress_dict_call_is_confined(oracle, dl, kind):
    import torch
    import streamly_lz4_amd as S
    cases = decode_inputs(oracle, dl)
    n = len(cases)
    caps = [c for _, c, _ in cases]
    framed, boff = bytearray(), []
    for blk, cap, hdr in cases:
        boff.append(len(framed))
        framed += int(len(blk) if hdr is None else hdr).to_bytes(4, "little", signed=True)
        if kind == 8:
            framed += int(cap).to_bytes(4, "little")
        framed += blk
    lay = G.layout(caps)
    eng = S.Engine(0)
    try:
        seed = 91
        out = G.new_torch(lay.total, seed, DEV)
        res = G.GuardedArray(n, torch.int32, seed + 7, DEV)
        dbuf, d = guarded_dict(dl, 41)
        fr = _t(np.frombuffer(bytes(framed), dtype=np.uint8).copy())
        bo, oo = _t(np.array(boff, dtype=np.int64)), _t(np.array(lay.starts, dtype=np.int64))
        oc = _t(np.array(caps, dtype=np.int32)) if kind == 4 else None
        copies = [t.clone() for t in (dbuf, fr, bo, oo)]
        eng.decompress_dict_device(fr, len(framed), bo, n, d, dl, out, oo, res.view, header_kind=kind,
                                   fixed_uncomp=max(caps) if kind == 4 else 0, out_cap=oc)
        eng.synchronize()
        torch.cuda.synchronize()
        G.assert_confined(out, lay.ranges(), seed, "out")
        res.check(what="result[]")
        for t, c in zip((dbuf, fr, bo, oo), copies):
            assert torch.equal(t, c), "the dictionary or an input was written"
        r, hb = res.view.cpu().tolist(), out.cpu().numpy()
        ok = fail = rejected = 0
        for i, (blk, cap, hdr) in enumerate(cases):
            if hdr is not None:
                assert r[i] <= -0x7F000000, (i, r[i])
                rejected += 1
                start = lay.starts[i]                                            # a rejected block: nothing written at all
                assert hb[start:start + cap].tobytes() == G.pattern(start, cap, seed).tobytes()
                continue
            code, dec = oracle.decompress_block(blk, cap, DC.dictionary(dl))
            assert r[i] == code, (i, code, r[i])
            if code >= 0:
                assert hb[lay.starts[i]:lay.starts[i] + code].tobytes() == dec
                ok += 1
            else:
                fail += 1
        assert ok >= 20 and fail >= 10 and rejected == 3, (ok, fail, rejected)
    finally:
        eng.close()


def test_load_dict_writes_only_its_slot(oracle):
    """streams live in slots 0 and 2; load_dict on slot 1 leaves their bytes alone, and continued they give what they gave
    before: the oracle's stream of both arrays"""
    import torch
    import streamly_lz4_amd as S
    from test_compress_streams_gpu import OracleStream, framed_by
    a, b = DC.block(65536), DC.block(4096)
    eng = S.Engine(0)
    cs = S.CompressStreams(eng, 3)
    try:
        stride = S.slot_stride_ex(65536, 8, False)

        def both(block):
            src = _t(np.frombuffer(block + block, dtype=np.uint8).copy())
            slots = torch.zeros(2 * stride, dtype=torch.uint8, device=DEV)
            flen = torch.zeros(2, dtype=torch.int32, device=DEV)
            eng.compress_streams_device(cs, src, 2, 65536, [0, 1, 2], [0, 2], slots, stride, flen, src_off=_t(np.array([0, len(block)], dtype=np.int64)),
                                        src_len=_t(np.array([len(block)] * 2, dtype=np.int32)), block_stride=0)
            eng.synchronize()
            fl, hb = flen.cpu().tolist(), slots.cpu().numpy()
            return [hb[i * stride:i * stride + fl[i]].tobytes() for i in range(2)]

        first = both(a)
        before = [cs.slot_bytes(0), cs.slot_bytes(2)]
        dbuf, d = guarded_dict(200000, 51)
        dcopy = dbuf.clone()
        cs.load_dict(1, d, 200000)
        eng.synchronize()
        assert torch.equal(dbuf, dcopy), "the dictionary handed in was written"
        assert [cs.slot_bytes(0), cs.slot_bytes(2)] == before
        assert cs.state(1) == (65536, 65536, 65536)
        second = both(b)
        want = framed_by(OracleStream(), [a, b], 1, 8)
        assert [first[0], second[0]] == want and [first[1], second[1]] == want
    finally:
        cs.close()
        eng.close()
