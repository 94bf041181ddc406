"""What mi355lz4_compress_streams_device may write (include/mi355lz4.h, "what a call may write"): the slot ranges of
_compress_batch_device and framedLen[0, nBlocks) -- nothing else of the buffers it is handed, and no input.  Guard patterns
around every range (tests/guarded.py), as tests/test_write_confinement_gpu.py does for the other calls."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import guarded as G  # noqa: E402
from test_compress_streams_gpu import OracleStream, cut, data, framed_by  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ragged streams: an empty one, zero-length arrays, lengths around the copy widths and 64 KiB
LENS = [[4095, 0, 13], [], [65537, 1, 3, 4], [12, 65536], [5, 200000, 65535]]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("extra", [0, 37])
@pytest.mark.parametrize("bad", [False, True])
def test_streams_call_is_confined(checksum, extra, bad):
    import torch
    import streamly_lz4_amd as S
    streams = [cut(data("text" if s % 2 else "pysrc", sum(lens) + 16, first=20 + s), lens) for s, lens in enumerate(LENS)]
    blocks = [b for st in streams for b in st]
    n = len(blocks)
    sf = np.cumsum([0] + [len(st) for st in streams]).astype(np.int32)
    mx = max(len(b) for b in blocks)
    lens = [len(b) for b in blocks]
    victim, at = 2, int(sf[2]) + 1                                       # stream 2 stops at its second block
    if bad:
        lens[at] = mx + 1
    need = S.slot_stride_ex(mx, 8, checksum)
    stride = need + extra
    lay_src = G.layout([len(b) for b in blocks])
    lay = G.layout([need] * n, stride=stride, first_residue=extra)
    eng = S.Engine(0)
    cs = S.CompressStreams(eng, len(streams) + 2)
    try:
        eng.set_block_checksum(checksum)
        slots_of = [5, 0, 3, 6, 1]
        seed = 71
        buf = G.new_torch(lay.total, seed, DEV)
        flen = G.GuardedArray(n, torch.int32, seed + 50, DEV)
        src = _t(G.pair(lay_src, blocks)[0])
        off = _t(np.array(lay_src.starts, dtype=np.int64))
        ln = _t(np.array(lens, dtype=np.int32))
        copies = [t.clone() for t in (src, off, ln)]
        eng.compress_streams_device(cs, src, n, mx, sf, slots_of, buf[lay.starts[0]:], stride, flen.view, src_off=off,
                                    src_len=ln, block_stride=0)
        eng.synchronize()
        torch.cuda.synchronize()
        dead = set(range(at, int(sf[victim + 1]))) if bad else set()
        G.assert_confined(buf, [r for i, r in enumerate(lay.ranges()) if i not in dead], seed, "slots")
        flen.check(what="framedLen[]")
        for t, c in zip((src, off, ln), copies):
            assert torch.equal(t, c), "an input was written"
        fl = flen.view.cpu().tolist()
        hb = buf.cpu().numpy()
        for s, st in enumerate(streams):
            want = framed_by(OracleStream(), st, 1, 8, checksum)
            for k, i in enumerate(range(int(sf[s]), int(sf[s + 1]))):
                if i in dead:
                    assert fl[i] == 0
                else:
                    assert hb[lay.starts[i]:lay.starts[i] + fl[i]].tobytes() == want[k], (s, k)
        assert cs.state(2) == cs.state(4) == (0, 0, 0)                   # slots the call does not name
    finally:
        cs.close()
        eng.close()
