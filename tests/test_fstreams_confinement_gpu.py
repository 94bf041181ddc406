"""What mi355lz4_compress_streams_fast_device may write (include/mi355lz4.h, "what a call may write"): slots[i*slotStride,
i*slotStride + framedLen[i]) and framedLen[0, nBlocks) -- nothing else of the buffers it is handed, no input, and of the set only
the slots the call names.  Guard patterns around every range (tests/guarded.py), as the sibling confinement tests do; and one
placement case (tests/placement.py): two blocks of one stream more than 2^32 bytes apart, in descending address order."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dstreams_model as M  # noqa: E402
import guarded as G  # noqa: E402
import placement as P  # noqa: E402
from test_fstreams_gpu import dict_pairs, pair_oracle, text_stream  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ragged streams: an empty one, zero-length arrays, lengths around the copy widths and 64 KiB
LENS = [[4095, 0, 13], [], [65537, 1, 3, 4096], [12, 65536], [5, 200000, 65535]]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("extra", [0, 37])
@pytest.mark.parametrize("bad", [False, True])
def test_fast_streams_call_is_confined(oracle, checksum, extra, bad):
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
    try:
        slots_of = [5, 0, 3, 6, 1]
        held = text_stream(oracle, [3000] * 7, 9000)                      # every slot holds something: 2 and 4 are not named
        for k, h in enumerate(held):
            fs.set_dict(k, _t(np.frombuffer(h, dtype=np.uint8).copy()), len(h))
        eng.synchronize()
        before = [fs.peek(k) for k in range(7)]
        assert before == [(3000, h) for h in held]
        eng.set_block_checksum(checksum)
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
        dead = set(range(at, int(sf[victim + 1]))) if bad else set()
        fl = flen.view.cpu().tolist()
        assert all(0 < f <= need for i, f in enumerate(fl) if i not in dead), fl
        G.assert_confined(buf, [(s, s + fl[i]) for i, s in enumerate(lay.starts) if i not in dead], seed, "slots")
        flen.check(what="framedLen[]")
        for t, c in zip((src, off, ln), copies):
            assert torch.equal(t, c), "an input was written"
        hb = buf.cpu().numpy()
        want = pair_oracle(S, eng, dict_pairs(streams, [held[k] for k in slots_of]), maxlen=mx)
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
        fs.close()
        eng.close()


def test_blocks_of_one_stream_beyond_4_gib_apart_descending(oracle):
    """block 0 above 2^32, block 1 near 0 (its dictionary lies more than 2^32 bytes above it), slot 1 at slotStride 2^31 + 37"""
    import torch
    import streamly_lz4_amd as S
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(0)
    if free < P.MIN_FREE:
        pytest.skip("needs 40 GiB of free device memory")
    blocks = text_stream(oracle, [65536, 40000], 4242)
    decoy = M.data(oracle, "text", 30000, first=99)
    mx = 65536
    need = S.slot_stride_ex(mx, 8, False)
    stride = (1 << 31) + 37
    inp, out = P.new_far(DEV), P.new_far(DEV)
    eng = S.Engine(0)
    fs = S.FastCompressStreams(eng, 2)
    try:
        starts = [P.FAR.full + (1 << 20) + 5, G.END_GUARD + 3]            # descending, 2^32 and more apart
        assert starts[0] - (starts[1] + len(blocks[1])) > (1 << 32)
        P.put_inputs(inp, starts, blocks, [decoy])
        base = G.END_GUARD + 11
        sstarts = [base, base + stride]
        win = P.Windows(sstarts, [need] * 2, seed=33)
        win.fill(out)
        flen = G.GuardedArray(2, torch.int32, 19, DEV)
        eng.compress_streams_fast_device(fs, P.view(inp), 2, mx, [0, 2], [1], P.view(out)[base:], stride, flen.view,
                                         src_off=_t(np.array(starts + [0], dtype=np.int64)),
                                         src_len=_t(np.array([65536, 40000], dtype=np.int32)), block_stride=0)
        eng.synchronize()
        fl = flen.view.cpu().tolist()
        flen.check(what="framedLen[]")
        assert all(0 < f <= need for f in fl), fl
        got = [P.read(out, s, f) for s, f in zip(sstarts, fl)]
        win.allowed = [tuple(m) for m in G._merge([(s + P.FAR.front, s + P.FAR.front + f) for s, f in zip(sstarts, fl)], P.FAR.total)]
        win.check(out, "slots")
        want = pair_oracle(S, eng, dict_pairs([blocks]))
        assert [g[8:] for g in got] == want
        assert len(want[1]) < len(pair_oracle(S, eng, [(b"", blocks[1])])[0])     # block 1 used the block far above it
        assert fs.peek(1) == (40000, blocks[1]) and fs.peek(0) == (0, b"")
    finally:
        fs.close()
        eng.close()
        inp = out = None
        torch.cuda.empty_cache()
