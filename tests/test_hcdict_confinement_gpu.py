"""What the high-compression dictionary calls may write (include/mi355lz4.h, "what a call may write"), held with guard patterns
around every range the header grants (tests/guarded.py), as tests/test_dict_confinement_gpu.py does for level 0's dictionary calls:
_hcdict_load the object alone, never the dictionary handed in; _compress_hcdict_device the slot ranges and framedLen[0, nBlocks),
never src, srcOff, srcLen, the dictionary tensor or the object's image.  Every buffer lies at an odd address."""
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

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAXLEN = max(DC.BLOCK_LENS)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded_dict(dl, seed):
    """the dictionary inside a guarded buffer: (buffer, the tensor view handed to the calls)"""
    lay = G.layout([dl], first_residue=5)
    buf = _t(G.pair(lay, [DC.dictionary(dl)], seeds=(seed, seed + 1))[0])
    return buf, buf[lay.starts[0]:lay.starts[0] + max(dl, 1)]


@pytest.mark.parametrize("dl", [0, 3, 4095, 200000])
def test_load_writes_only_the_object(dl):
    import streamly_lz4_amd as S
    import torch
    eng = S.Engine(0)
    hd, other = S.HcDict(eng), S.HcDict(eng)
    try:
        other.load(_t(np.frombuffer(DC.dictionary(100), dtype=np.uint8).copy()), 100)
        eng.synchronize()
        before = other.image()
        dbuf, d = guarded_dict(dl, 51)
        dcopy = dbuf.clone()
        hd.load(d, dl)
        eng.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(dbuf, dcopy), "the dictionary handed in was written"
        assert other.image() == before, "another object was written"
        keep = min(dl, 65536)
        img = hd.image()
        assert len(hd) == keep and int.from_bytes(img[155648:155652], "little") == keep
        assert img[155712:155712 + keep] == DC.dictionary(dl)[dl - keep:]
        if keep < 4:                                    # an empty image: no position was inserted
            assert img[131072:155648] == b"\xff" * 24576 and img[:131072] == bytes(131072)
    finally:
        hd.close()
        other.close()
        eng.close()


@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("extra", [0, 37])
@pytest.mark.parametrize("bad", [False, True])
def test_compress_hcdict_call_is_confined(oracle, checksum, extra, bad):
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
    hd = S.HcDict(eng)
    try:
        eng.set_block_checksum(checksum)
        eng.set_compression_level(6)
        dbuf, d = guarded_dict(dl, 31)
        hd.load(d, dl)
        eng.synchronize()
        dcopy = dbuf.clone()
        image = hd.image()
        seed = 73
        buf = G.new_torch(lay.total, seed, DEV)
        flen = G.GuardedArray(n, torch.int32, seed + 50, DEV)
        src = _t(G.pair(lay_src, blocks)[0])
        off = _t(np.array(lay_src.starts, dtype=np.int64))
        ln = _t(np.array(lens, dtype=np.int32))
        copies = [t.clone() for t in (src, off, ln)]
        eng.compress_hcdict_device(hd, src, n, MAXLEN, buf[lay.starts[0]:], stride, flen.view, header_kind=8, src_off=off, src_len=ln,
                                   block_stride=0)
        eng.synchronize()
        torch.cuda.synchronize()
        fl = flen.view.cpu().tolist()
        # a block may write its slot up to framedLen[i], and nothing behind it
        allowed = [(s, s + fl[i]) for i, (s, _) in enumerate(lay.ranges()) if i not in dead]
        G.assert_confined(buf, allowed, seed, "slots")
        flen.check(what="framedLen[]")
        for t, c in zip((src, off, ln), copies):
            assert torch.equal(t, c), "an input was written"
        assert torch.equal(dbuf, dcopy), "the dictionary tensor was written"
        assert hd.image() == image, "the prepared dictionary was written"
        hb = buf.cpu().numpy()
        trailer = 4 if checksum else 0
        for i, bl in enumerate(DC.BLOCK_LENS):
            if i in dead:
                assert fl[i] == 0
                continue
            comp = hb[lay.starts[i] + 8:lay.starts[i] + fl[i] - trailer].tobytes()
            assert int.from_bytes(hb[lay.starts[i]:lay.starts[i] + 4].tobytes(), "little") == len(comp)
            lz4_check.check_block(comp, bl, dict_len=65536)
            assert oracle.decompress_block(comp, bl, DC.dictionary(dl)[-65536:]) == (bl, blocks[i]), bl
    finally:
        hd.close()
        eng.close()
