"""What mi355lz4_decompress_dstreams_device may write (include/mi355lz4.h, "what a call may write"): `out` only in the union of
[outOff[i], outOff[i] + cap_i), result only in [0, nBlocks), of the set only the slots named for a stream with blocks, the
inputs never -- whatever the blocks' results.  Guard patterns (tests/guarded.py) lie around every output range, around
result, around framed, and in a second set's worth of slots that no call names."""
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
from oracle.oracle import Oracle  # noqa: E402

pytestmark = pytest.mark.gpu

FIXED = 262144
_ORC = None


def orc():
    global _ORC
    if _ORC is None:
        _ORC = Oracle()
    return _ORC


@pytest.fixture
def eng():
    import streamly_lz4_amd as S
    e = S.Engine(0)
    yield e
    e.close()


@pytest.fixture
def ds16(eng):
    """eight slots for the streams and eight more that no call names, filled with a guard pattern"""
    import streamly_lz4_amd as S
    ds = S.DecompressStreams(eng, 16)
    for k in range(8, 16):
        ds.state(k, set_bytes=G.pattern(0, 65536, seed=900 + k).tobytes())
    yield ds
    ds.close()


def check_unused_slots(ds, touched=()):
    for k in range(8, 16):
        cnt, held = ds.state(k)
        assert cnt == 0 and held == G.pattern(0, 65536, seed=900 + k).tobytes(), "slot %d, which no call names, was written" % k
    for k in range(8):
        if k not in touched:
            assert ds.state(k)[0] == 0, "slot %d, which no call names, was written" % k


def guarded_call(eng, ds, per_stream, slots, kind, call_no):
    """device_call of tests/test_dstreams_gpu.py with guards; returns per stream [(code, bytes)]"""
    import torch
    blocks = [b for st in per_stream for b in st]
    n = len(blocks)
    sf = np.cumsum([0] + [len(st) for st in per_stream]).astype(np.int32)
    framed = b"".join(b.framed for b in blocks)
    lay_in = G.layout([len(framed)], first_residue=3 + call_no)
    inp = G.new_torch(lay_in.total, seed=300 + call_no)
    f0 = lay_in.starts[0]
    inp[f0:f0 + len(framed)] = torch.from_numpy(np.frombuffer(framed, dtype=np.uint8).copy()).cuda()
    inp_before = inp.clone()
    lay = G.layout([b.cap for b in blocks], first_residue=call_no)
    out = G.new_torch(lay.total, seed=400 + call_no)
    res = G.GuardedArray(n, torch.int32, seed=500 + call_no, device="cuda:0")
    boff = np.cumsum([f0] + [len(b.framed) for b in blocks])[:n].astype(np.int64)
    boff_d = torch.from_numpy(np.append(boff, 0)).cuda()
    ooff_d = torch.tensor(lay.starts + [0], dtype=torch.int64).cuda()
    cap_d = torch.tensor([b.cap for b in blocks] + [0], dtype=torch.int32).cuda() if kind == 4 else None
    keep = [t.clone() for t in (boff_d, ooff_d)] + ([cap_d.clone()] if cap_d is not None else [])
    # the framed buffer is the whole guarded allocation: headers and data are bounds-checked against its end
    eng.decompress_dstreams_device(ds, inp, lay_in.total, boff_d, n, sf, slots, out, ooff_d, res.view, header_kind=kind,
                                   fixed_uncomp=FIXED if kind == 4 else 0, out_cap=cap_d)
    torch.cuda.synchronize()
    G.assert_confined(out, lay.ranges(), 400 + call_no, "out, call %d" % call_no)
    res.check(0, n, "result, call %d" % call_no)
    assert torch.equal(inp, inp_before), "framed was written, call %d" % call_no
    for t, k in zip([boff_d, ooff_d] + ([cap_d] if cap_d is not None else []), keep):
        assert torch.equal(t, k), "an input array was written, call %d" % call_no
    codes = res.view.cpu().tolist()
    got = out.cpu().numpy()
    flat = [(codes[i], got[lay.starts[i]:lay.starts[i] + codes[i]].tobytes() if codes[i] > 0 else b"") for i in range(n)]
    return [flat[sf[s]:sf[s + 1]] for s in range(len(per_stream))]


def feed(eng, ds, streams, slots, partition, kind):
    done = [0] * len(streams)
    got = [[] for _ in streams]
    for c, counts in enumerate(partition):
        per = [st[d:d + k] for st, d, k in zip(streams, done, counts)]
        r = guarded_call(eng, ds, per, slots, kind, c)
        touched = {slots[s] for s in range(len(streams)) if done[s] + counts[s] > 0}
        check_unused_slots(ds, touched)
        for s, k in enumerate(counts):
            got[s] += r[s]
            done[s] += k
    return got


def expect(streams):
    return [list(zip(*M.model(orc(), st)[:2])) for st in streams]


@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("partition", ["two_three", "uneven"])
def test_cut_streams_confined(eng, ds16, kind, partition):
    streams, _ = M.cut_streams(orc(), kind)
    for st in streams:
        M.assert_dependent(orc(), st)
    got = feed(eng, ds16, streams, M.CUT_SLOTS, M.PARTITIONS[partition], kind)
    assert got == expect(streams)


@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("cuts", [[3, 3], [2, 4]], ids=["bad_last", "bad_first"])
def test_failing_blocks_confined(eng, ds16, kind, cuts):
    """a corrupted block, a zero-byte array and a header-rejected block: no guard byte changes, whatever the results"""
    st, _ = M.failing_stream(orc(), kind)
    M.assert_dependent(orc(), st)
    other = M.cut_streams(orc(), kind)[0][4]
    got = feed(eng, ds16, [st, other], [6, 1], [[a, 3] for a in cuts], kind)
    assert got == expect([st, other])
