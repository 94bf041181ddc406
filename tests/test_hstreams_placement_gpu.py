"""mi355lz4_compress_streams_fast_device with the set at level 9 and its regions placed anywhere (include/mi355lz4.h, "Where a
call's regions may lie"): the blocks, the dictionary handed to _set_dict and the slots lie where tests/placement.py's
"far_permuted" layout puts them -- not in ascending order, a block below its predecessor and below the call's first block, and,
where the card has the memory for two far buffers, near 0, across 2^31 and 2^32 and more than 2^32 bytes from the predecessor
whose tail k_encode_hc_fstreams stages in front of it.  On a card without that much free memory the same layout runs in a space
of 2^27 bytes.  The bytes are the pair oracle's; the slots lie in guard windows, with equal windows at every 32-bit alias."""
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
from test_hstreams_gpu import dict_pairs, pair_oracle, text_stream  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVEL = 9
LENS = [[4096, 65536, 13, 70000], [1, 65536, 4095], [30000, 30000, 5, 12, 60000]]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_level_nine_call_with_blocks_slots_and_dictionary_placed_anywhere(oracle, record):
    import torch
    import streamly_lz4_amd as S
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(0)
    space = P.FAR if free >= P.MIN_FREE else P.Space(27)
    record("hstreams_placement", {"free_bytes": int(free), "space_bits": space.bits})
    streams = [text_stream(oracle, lens, 500 + 4000 * s) for s, lens in enumerate(LENS)]
    blocks = [bytes(b) for st in streams for b in st]
    n = len(blocks)
    sf = np.cumsum([0] + [len(st) for st in streams]).astype(np.int32)
    slots_of = [2, 0, 1]
    dic = M.data(oracle, "text", 50000, first=900)                        # stream 0's slot holds it: what its first block matches
    decoy = M.data(oracle, "text", 777, first=31)
    mx = max(len(b) for b in blocks)
    need = S.slot_stride_ex(mx, 8, False)
    # the slots lie a fixed stride apart: the widest that keeps all of them inside the view
    stride = ((space.view_len - 4 * G.END_GUARD - need) // n) & ~15 | 5
    assert stride > need
    inp, out = P.new_far(DEV, space), P.new_far(DEV, space)
    eng = S.Engine(0)
    fs = S.FastCompressStreams(eng, 3)
    try:
        starts = P.place([len(b) for b in blocks] + [len(dic)], "far_permuted", space, first_residue=3)
        P.put_inputs(inp, starts, blocks + [dic], [decoy], space)
        if space is P.FAR:
            assert any(abs(starts[i] - starts[i - 1]) > (1 << 32) for i in range(1, n) if i not in set(sf.tolist()))
        base = G.END_GUARD + 11
        sstarts = [base + i * stride for i in range(n)]
        win = P.Windows(sstarts, [need] * n, space, seed=33)
        win.fill(out)
        flen = G.GuardedArray(n, torch.int32, 19, DEV)
        fs.set_dict(slots_of[0], P.view(inp, space)[starts[n]:starts[n] + len(dic)], len(dic))
        fs.set_level(LEVEL)
        eng.compress_streams_fast_device(fs, P.view(inp, space), n, mx, sf, slots_of, P.view(out, space)[base:], stride, flen.view,
                                         src_off=_t(np.array(starts[:n] + [0], dtype=np.int64)),
                                         src_len=_t(np.array([len(b) for b in blocks] + [0], dtype=np.int32)), block_stride=0)
        fs.set_level(0)
        eng.synchronize()
        fl = flen.view.cpu().tolist()
        flen.check(what="framedLen[]")
        assert all(0 < f <= need for f in fl), fl
        got = [P.read(out, s, f, space) for s, f in zip(sstarts, fl)]
        win.allowed = [tuple(m) for m in G._merge([(s + space.front, s + space.front + f) for s, f in zip(sstarts, fl)], space.total)]
        win.check(out, "slots")
        for s, b in zip(starts, blocks):
            assert P.read(inp, s, len(b), space) == b, "src was written"
        want = pair_oracle(S, eng, dict_pairs(streams, [dic, b"", b""]), LEVEL, maxlen=mx)
        assert [g[8:] for g in got] == want
        assert [int.from_bytes(g[:4], "little") for g in got] == [len(w) for w in want]
        assert [fs.peek(k) for k in slots_of] == [(min(len(st[-1]), 65536), bytes(st[-1][-65536:])) for st in streams]
    finally:
        fs.close()
        eng.close()
        inp = out = None
        torch.cuda.empty_cache()
