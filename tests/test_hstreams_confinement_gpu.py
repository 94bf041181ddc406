"""What mi355lz4_compress_streams_fast_device may write with the set at level 9 (include/mi355lz4.h, "what a call may write"; the
set's level changes nothing of it): slots[i*slotStride, i*slotStride + framedLen[i]) and framedLen[0, nBlocks) -- nothing else of
the buffers it is handed, no input, and of the set only the slots the call names.  Guard patterns around every range
(tests/guarded.py), as tests/test_fstreams_confinement_gpu.py has them at level 0; two workgroups serve the blocks
(MI355LZ4_HSTREAMS_GROUPS), so every window is used again, staged and in place."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import guarded as G  # noqa: E402
from test_hstreams_gpu import KNOB, dict_pairs, pair_oracle, text_stream  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVEL = 9

# ragged streams: an empty one, zero-length arrays, lengths around the copy widths, a parse round and 64 KiB
LENS = [[4095, 0, 13], [], [65537, 1, 3, 4096], [12, 65536], [5, 100000, 65535, 1025]]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("extra", [0, 37])
@pytest.mark.parametrize("bad", [False, True])
def test_fast_streams_call_at_level_nine_is_confined(oracle, checksum, extra, bad):
    import torch
    import streamly_lz4_amd as S
    streams = [text_stream(oracle, lens, 20 + 3000 * s) for s, lens in enumerate(LENS)]
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
    fs = S.FastCompressStreams(eng, len(streams) + 2)
    os.environ[KNOB] = "2"
    try:
        slots_of = [5, 0, 3, 6, 1]
        held = text_stream(oracle, [3000] * 7, 9000)                      # every slot holds something: 2 and 4 are not named
        for k, h in enumerate(held):
            fs.set_dict(k, _t(np.frombuffer(h, dtype=np.uint8).copy()), len(h))
        eng.synchronize()
        before = [fs.peek(k) for k in range(7)]
        assert before == [(3000, h) for h in held]
        eng.set_block_checksum(checksum)
        fs.set_level(LEVEL)
        seed = 71
        buf = G.new_torch(lay.total, seed, DEV)
        flen = G.GuardedArray(n, torch.int32, seed + 50, DEV)
        src = _t(G.pair(lay_src, blocks)[0])
        off = _t(np.array(lay_src.starts, dtype=np.int64))
        ln = _t(np.array(lens, dtype=np.int32))
        copies = [t.clone() for t in (src, off, ln)]
        eng.compress_streams_fast_device(fs, src, n, mx, sf, slots_of, buf[lay.starts[0]:], stride, flen.view, src_off=off,
                                         src_len=ln, block_stride=0)
        eng.synchronize()
        torch.cuda.synchronize()
        eng.set_block_checksum(False)
        fs.set_level(0)
        dead = set(range(at, int(sf[victim + 1]))) if bad else set()
        fl = flen.view.cpu().tolist()
        assert all(0 < f <= need for i, f in enumerate(fl) if i not in dead), fl
        G.assert_confined(buf, [(s, s + fl[i]) for i, s in enumerate(lay.starts) if i not in dead], seed, "slots")
        flen.check(what="framedLen[]")
        for t, c in zip((src, off, ln), copies):
            assert torch.equal(t, c), "an input was written"
        hb = buf.cpu().numpy()
        want = pair_oracle(S, eng, dict_pairs(streams, [held[k] for k in slots_of]), LEVEL, maxlen=mx, key="confinement")
        trailer = 4 if checksum else 0
        for i in range(n):
            if i in dead:
                assert fl[i] == 0
            else:
                assert hb[lay.starts[i] + 8:lay.starts[i] + fl[i] - trailer].tobytes() == want[i], i
        # the state slots: the ones the call does not name (2, 4) and the empty stream's (0) are byte-identical; the others moved on
        after = [fs.peek(k) for k in range(7)]
        for k in (2, 4, 0):
            assert after[k] == before[k], k
        for s, k in enumerate(slots_of):
            good = [b for i, b in zip(range(int(sf[s]), int(sf[s + 1])), streams[s]) if i not in dead]
            if good:
                assert after[k] == (min(len(good[-1]), 65536), good[-1][-65536:] if good[-1] else b""), (s, k)
    finally:
        os.environ.pop(KNOB, None)
        fs.close()
        eng.close()
