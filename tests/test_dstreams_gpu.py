"""Many linked decode streams continued across calls (mi355lz4_dstreams, mi355lz4_decompress_dstreams_device / _dstreams).
Every stream of a call continues its own slot of device-resident state.  However a stream is cut into calls, result[] and the
bytes must be the model's (tests/dstreams_model.py: the CPU oracle, block by block with the previous output as dictionary)
and those of ONE mi355lz4_decompress_streams_device call on the whole streams."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from conftest import DECODERS  # noqa: E402
import dstreams_model as M  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG = -3
FIXED = 262144                     # headerKind 4: the largest block of the tests
_i32p = C.POINTER(C.c_int32)
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
def ds8(eng):
    import streamly_lz4_amd as S
    ds = S.DecompressStreams(eng, 8)
    yield ds
    ds.close()


def device_call(eng, ds, per_stream, slots, kind, gap=7, scribble=True):
    """One call: per_stream[s] = the Blocks stream s brings (may be empty), continuing slot slots[s]; ds = None runs the same
    blocks through ONE decompress_streams_device call instead.  The outputs lie `gap` bytes apart at their capacities
    (kind 4: outCap = the block's capacity).  Returns per stream [(code, bytes)]."""
    import torch
    blocks = [b for st in per_stream for b in st]
    n = len(blocks)
    sf = np.cumsum([0] + [len(st) for st in per_stream]).astype(np.int32)
    framed = b"".join(b.framed for b in blocks)
    boff = np.cumsum([0] + [len(b.framed) for b in blocks])[:n].astype(np.int64)
    ooff = np.array([sum(b.cap for b in blocks[:i]) + i * gap for i in range(n)] + [0], dtype=np.int64)
    total = sum(b.cap for b in blocks) + n * gap + 64
    f_d = torch.from_numpy(np.frombuffer(framed + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    boff_d = torch.from_numpy(np.append(boff, 0)).cuda()
    ooff_d = torch.from_numpy(ooff).cuda()
    cap_d = torch.tensor([b.cap for b in blocks] + [0], dtype=torch.int32).cuda() if kind == 4 else None
    out = torch.full((total,), 0x5C, dtype=torch.uint8).cuda()
    res = torch.full((max(n, 1),), -12345, dtype=torch.int32).cuda()
    if ds is None:
        eng.decompress_streams_device(f_d, len(framed), boff_d, n, torch.from_numpy(sf).cuda(), len(per_stream), out, ooff_d, res,
                                      header_kind=kind, fixed_uncomp=FIXED if kind == 4 else 0, out_cap=cap_d)
    else:
        eng.decompress_dstreams_device(ds, f_d, len(framed), boff_d, n, sf, slots, out, ooff_d, res, header_kind=kind,
                                       fixed_uncomp=FIXED if kind == 4 else 0, out_cap=cap_d)
    torch.cuda.synchronize()
    codes = res.cpu().tolist()[:n]
    got = out.cpu().numpy()
    if scribble:                                   # the call has run: its output and its input are the caller's again
        out.fill_(0xAA)
        f_d.fill_(0xAA)
        torch.cuda.synchronize()
    flat = [(codes[i], got[ooff[i]:ooff[i] + codes[i]].tobytes() if codes[i] > 0 else b"") for i in range(n)]
    return [flat[sf[s]:sf[s + 1]] for s in range(len(per_stream))]


def feed(eng, ds, streams, slots, partition, kind, scribble=True, whole=True):
    """The streams cut into calls: partition[c][s] = blocks of stream s in call c.  Returns per stream [(code, bytes)].
    whole = False: the partition may stop before the streams' ends."""
    done = [0] * len(streams)
    got = [[] for _ in streams]
    for counts in partition:
        per = [st[d:d + k] for st, d, k in zip(streams, done, counts)]
        r = device_call(eng, ds, per, slots, kind, scribble=scribble)
        for s, k in enumerate(counts):
            got[s] += r[s]
            done[s] += k
    assert not whole or done == [len(st) for st in streams]
    return got


def expected(streams):
    out = []
    for st in streams:
        codes, outs, _ = M.model(orc(), st)
        out.append(list(zip(codes, outs)))
    return out


def check(got, want, what):
    for s, (g, w) in enumerate(zip(got, want)):
        assert [c for c, _ in g] == [c for c, _ in w], "%s: stream %d: codes" % (what, s)
        for i, ((_, gb), (_, wb)) in enumerate(zip(g, w)):
            assert gb == wb, "%s: stream %d block %d: bytes differ" % (what, s, i)


# ---- 1. cut anywhere --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder", DECODERS)
@pytest.mark.parametrize("kind", [8, 4])
def test_cut_anywhere(eng, ds8, kind, decoder):
    streams, arrays = M.cut_streams(orc(), kind)
    for st in streams:
        M.assert_dependent(orc(), st)
    want = expected(streams)
    for s, a in enumerate(arrays):                               # (the model decodes the streams to their data)
        assert [b for _, b in want[s]] == a
    eng.set_decoder(decoder)                                     # what the whole-stream call below decodes with
    whole = device_call(eng, None, streams, None, kind)
    check(whole, want, "one decompress_streams_device call")
    for name, part in M.PARTITIONS.items():
        ds8.reset()
        got = feed(eng, ds8, streams, M.CUT_SLOTS, part, kind, scribble=False)
        check(got, want, "partition %s vs the model" % name)
        check(got, whole, "partition %s vs the whole-stream call" % name)


# ---- 2. the slot owns its copy ----------------------------------------------------------------------------------------------
def test_slot_owns_its_copy(eng, ds8):
    streams, _ = M.cut_streams(orc(), 8)
    for st in streams:
        M.assert_dependent(orc(), st)
    # (feed() fills all of `out` and `framed` of every call with 0xAA before the next one)
    got = feed(eng, ds8, streams, M.CUT_SLOTS, M.PARTITIONS["one"], 8, scribble=True)
    check(got, expected(streams), "inputs and outputs overwritten between calls")


# ---- 3. failures leave the state --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("cuts", [[3, 3], [2, 4], [2, 1, 1, 1, 1], [6]], ids=["bad_last", "bad_first", "one_each", "one_call"])
def test_failures_leave_the_state(eng, ds8, kind, cuts):
    st, arrays = M.failing_stream(orc(), kind)
    M.assert_dependent(orc(), st)
    codes, outs, _ = M.model(orc(), st)
    assert codes[:2] == [4096, 4096] and -0x7F000000 < codes[2] < 0 and codes[3] == 0 and codes[4] == M.BLK_E_COMPLEN
    assert codes[5] == 4096 and outs[5] == arrays[2]             # against the second block, the last one with r > 0
    # a second stream shares the calls and must not notice
    other, oarr = M.cut_streams(orc(), kind)
    other, oarr = other[0], oarr[0]
    ocuts = {2: [3, 3], 5: [1, 1, 1, 1, 2], 1: [6]}[len(cuts)]
    got = feed(eng, ds8, [st, other], [6, 1], [[a, b] for a, b in zip(cuts, ocuts)], kind)
    check(got, expected([st, other]), "cuts %r" % (cuts,))
    whole = device_call(eng, None, [st, other], None, kind)
    check(got, whole, "cuts %r vs the whole-stream call" % (cuts,))


# ---- 4. reset and set_dict --------------------------------------------------------------------------------------------------
def test_reset_and_set_dict(eng, ds8):
    import torch
    streams, arrays = M.cut_streams(orc(), 8)
    a, b, c = (streams[s] for s in (0, 1, 3))
    for st in (a, b, c):
        M.assert_dependent(orc(), st)
    slots = [4, 6, 1]
    want = expected([a, b, c])
    got = feed(eng, ds8, [a, b, c], slots, [[2, 2, 2]], 8, whole=False)
    check(got, [w[:2] for w in want], "the first two blocks of each stream")
    ds8.reset([6])
    got2 = device_call(eng, ds8, [a[2:3], b[2:3], c[2:3]], slots, 8)
    assert got2[0] == [want[0][2]] and got2[2] == [want[2][2]], "the other slots go on unharmed"
    alone = orc().decompress_block(b[2].comp, b[2].cap)
    assert alone[0] < 0 and got2[1][0][0] == alone[0], "after a reset: the model's no-dictionary code"
    # LZ4_setStreamDecode with the previous block's output: the block decodes
    prev = torch.from_numpy(np.frombuffer(arrays[1][1], dtype=np.uint8).copy()).cuda()
    ds8.set_dict(6, prev)
    torch.cuda.synchronize()
    prev.fill_(0xAA)                                             # the slot keeps its own copy
    got3 = device_call(eng, ds8, [[], b[2:3], []], slots, 8)
    assert got3[1] == [want[1][2]]
    # len == 0 equals a reset
    ds8.set_dict(6, prev, 0)
    got4 = device_call(eng, ds8, [[], b[3:4], []], slots, 8)
    assert got4[1][0][0] == orc().decompress_block(b[3].comp, b[3].cap)[0] < 0
    assert ds8.state(6)[0] == 0 and len(ds8) == 8


def test_set_dict_keeps_the_last_64k(eng, ds8):
    """a 200 KiB dictionary: the slot keeps its last 64 KiB, and the block's matches reach 65535 bytes back into them"""
    import torch
    big = orc().gen("random", 1, 200 << 10).tobytes()
    arr = big[len(big) - 65535:len(big) - 65535 + 2000] + M.data(orc(), "text", 3000)
    comp = M.linked_stream(orc(), [big, arr])[1]
    r, out = orc().decompress_block(comp, len(arr), dict_bytes=big[-65536:])
    assert r == len(arr) and out == arr
    assert orc().decompress_block(comp, len(arr), dict_bytes=big[-65535:]) == (r, out)
    short = orc().decompress_block(comp, len(arr), dict_bytes=big[-65534:])
    assert short != (r, out), "the block does not reach 65535 bytes back"
    d = torch.from_numpy(np.frombuffer(big, dtype=np.uint8).copy()).cuda()
    ds8.set_dict(3, d)
    got = device_call(eng, ds8, [[M.good_block(comp, len(arr), 8)]], [3], 8)
    assert got[0] == [(r, out)]
    cnt, held = ds8.state(3)
    assert cnt == len(arr) and held[:cnt] == arr                 # ... and the slot has moved on to the block's own output
    # a dictionary one byte short of that reach: the model's result for it
    ds8.set_dict(3, d[len(big) - 65534:])
    got = device_call(eng, ds8, [[M.good_block(comp, len(arr), 8)]], [3], 8)
    assert got[0] == [short]


# ---- 5. block checksums -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [8, 4])
def test_block_checksums(eng, ds8, kind):
    streams, arrays = M.cut_streams(orc(), kind, checksum=True)
    streams = [list(st) for st in streams]
    for st in streams:
        M.assert_dependent(orc(), st)
    bad = streams[1][2]
    streams[1][2] = M.bad_checksum_block(bad.comp, bad.cap, kind)  # one trailer mismatch: a header-rejected block
    want = expected(streams)
    assert want[1][2][0] == M.BLK_E_CHECKSUM
    eng.set_block_checksum(True)
    try:
        whole = device_call(eng, None, streams, None, kind)
        for name, part in M.PARTITIONS.items():
            ds8.reset()
            got = feed(eng, ds8, streams, M.CUT_SLOTS, part, kind)
            check(got, want, "checksums, partition %s" % name)
            check(got, whole, "checksums, partition %s vs the whole-stream call" % name)
    finally:
        eng.set_block_checksum(False)


# ---- 6. round trip with cstreams --------------------------------------------------------------------------------------------
def test_round_trip_with_cstreams(eng):
    """compress_streams_device one array per call, each call's slots straight into decompress_dstreams_device: device-resident,
    no host copy between"""
    import torch
    import streamly_lz4_amd as S
    lens = [[65536, 4096, 70000, 1000], [1000, 65536, 65536, 40], [70000, 70000, 4096, 65536], [4096, 1000, 65536, 70000]]
    arrays = [M.cut(M.data(orc(), "pysrc" if s % 2 else "text", sum(ln), first=5000 * s), ln) for s, ln in enumerate(lens)]
    cs, ds = S.CompressStreams(eng, 4), S.DecompressStreams(eng, 6)
    try:
        mx = 70000
        stride = S.slot_stride_ex(mx, 8, False)
        sf, cslots, dslots = [0, 1, 2, 3, 4], [3, 1, 0, 2], [5, 2, 0, 4]
        for k in range(4):
            blocks = [arrays[s][k] for s in range(4)]
            src = torch.zeros(4 * mx, dtype=torch.uint8)
            for s, a in enumerate(blocks):
                src[s * mx:s * mx + len(a)] = torch.from_numpy(np.frombuffer(a, dtype=np.uint8).copy())
            src = src.cuda()
            ln = torch.tensor([len(a) for a in blocks], dtype=torch.int32).cuda()
            slots = torch.zeros(4 * stride, dtype=torch.uint8).cuda()
            flen = torch.zeros(4, dtype=torch.int32).cuda()
            eng.compress_streams_device(cs, src, 4, mx, sf, cslots, slots, stride, flen, src_len=ln)
            boff = torch.arange(4, dtype=torch.int64).cuda() * stride
            ooff = torch.arange(5, dtype=torch.int64).cuda() * mx
            out = torch.zeros(4 * mx, dtype=torch.uint8).cuda()
            res = torch.zeros(4, dtype=torch.int32).cuda()
            eng.decompress_dstreams_device(ds, slots, 4 * stride, boff, 4, sf, dslots, out, ooff, res)
            torch.cuda.synchronize()
            assert res.cpu().tolist() == [len(a) for a in blocks], "call %d" % k
            got = out.cpu().numpy()
            for s, a in enumerate(blocks):
                assert got[s * mx:s * mx + len(a)].tobytes() == a, "call %d stream %d" % (k, s)
    finally:
        cs.close()
        ds.close()


# ---- 7. argument errors -----------------------------------------------------------------------------------------------------
def test_argument_errors(eng, ds8):
    import torch
    import streamly_lz4_amd as S
    from guarded import GuardedArray, new_torch, assert_confined
    st = M.cut_streams(orc(), 8)[0][2][:2]                       # 40 and 4096 bytes
    framed = b"".join(b.framed for b in st)
    f_d = torch.from_numpy(np.frombuffer(framed, dtype=np.uint8).copy()).cuda()
    boff = torch.tensor([0, len(st[0].framed)], dtype=torch.int64).cuda()
    ooff = torch.tensor([40000, 50000, 0], dtype=torch.int64).cuda()
    out = new_torch(100000, seed=5)
    res = GuardedArray(2, torch.int32, seed=6, device="cuda:0")
    device_call(eng, ds8, [st[:1]], [0], 8)                      # slot 0 holds something to lose
    before = ds8.state(0)

    def call(sf, sl, n_streams=None, n_blocks=2, dset=None, framed_p=f_d, boff_p=boff, ooff_p=ooff, res_p=res.view, ctx=None):
        sf = np.asarray(sf, dtype=np.int32)
        sl = np.asarray(sl + [0], dtype=np.int32)
        eng._follow_torch()
        return S.lib.mi355lz4_decompress_dstreams_device(
            eng.ctx if ctx is None else ctx, (ds8 if dset is None else dset)._h if dset is not False else None,
            S._dptr(framed_p), len(framed), S._dptr(boff_p), n_blocks, 8, 0, sf.ctypes.data_as(_i32p), sl.ctypes.data_as(_i32p),
            len(sf) - 1 if n_streams is None else n_streams, S._dptr(out), S._dptr(ooff_p), None, S._dptr(res_p))

    assert call([0, 2, 1], [0, 1]) == E_ARG                      # not ascending
    assert call([0, 1], [0]) == E_ARG                            # does not cover the blocks
    assert call([1, 2], [0]) == E_ARG                            # does not start at block 0
    assert call([0, 2], [8]) == E_ARG                            # slot out of range
    assert call([0, 2], [-1]) == E_ARG
    assert call([0, 1, 2], [3, 3]) == E_ARG                      # the same slot twice
    assert call([0, 2], [0], framed_p=None) == E_ARG             # null pointers with nBlocks > 0
    assert call([0, 2], [0], boff_p=None) == E_ARG
    assert call([0, 2], [0], ooff_p=None) == E_ARG
    assert call([0, 2], [0], res_p=None) == E_ARG
    assert call([0, 2], [0], dset=False) == E_ARG                # null set
    assert call([0, 2], [0], n_blocks=-1) == E_ARG
    if S.device_count() > 1:                                     # a set from another device
        e1 = S.Engine(1)
        try:
            assert call([0, 2], [0], ctx=e1.ctx) == E_ARG
        finally:
            e1.close()
    # an open mi355lz4_decompress_linked_begin range
    ln, lbl = 8, 65536
    lframed = orc().frame_compress(orc().gen("text", ln, lbl).tobytes(), lbl, 1, 8, True)
    lfr = torch.from_numpy(np.frombuffer(lframed, dtype=np.uint8).copy()).cuda()
    lboff = torch.tensor(S.index_host(lframed, 8, 0)[0], dtype=torch.int64).cuda()
    looff = torch.arange(ln + 1, dtype=torch.int64).cuda() * lbl
    lout = torch.zeros(ln * lbl, dtype=torch.uint8).cuda()
    lres = torch.zeros(ln, dtype=torch.int32).cuda()
    eng.decompress_linked_begin(lfr, len(lframed), lboff, ln, lout, looff, lres, 0)
    try:
        assert call([0, 2], [0]) == E_ARG
    finally:
        eng.decompress_linked_end()
        eng.synchronize()
    assert lres.cpu().tolist() == [lbl] * ln
    torch.cuda.synchronize()
    # nothing was written by any of them
    assert_confined(out, [], 5, "out after argument errors")
    res.check(0, 0, "result after argument errors")
    assert ds8.state(0) == before
    # nBlocks == 0, and a table with empty streams
    assert call([0], [], n_blocks=0) == 0
    assert call([0, 0, 0], [1, 2], n_blocks=0) == 0
    assert call([0, 0], [0], n_blocks=0, framed_p=None, boff_p=None, ooff_p=None, res_p=None) == 0
    torch.cuda.synchronize()
    assert_confined(out, [], 5, "out after empty calls")
    assert ds8.state(0) == before
    got = device_call(eng, ds8, [[], st[1:2], []], [4, 0, 5], 8)  # empty streams beside one that continues slot 0
    assert got[1] == [expected([st])[0][1]]
    assert ds8.state(4)[0] == 0 and ds8.state(5)[0] == 0


# ---- 8. host form -----------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
for p in (%r, %r + "/streamly-lz4_amd", %r + "/tests"):
    sys.path.insert(0, p)
import numpy as np
import streamly_lz4_amd as S
import dstreams_model as M
from oracle.oracle import Oracle
O = Oracle()
eng = S.Engine(0)
ds = S.DecompressStreams(eng, 6)
# four streams of 64 KiB blocks, one of them 3 MiB: groups of 1 MiB cut it, and a call boundary does too
lens = [[65536] * 3, [65536] * 48, [65536, 1000, 4096], [65536] * 5]
arrays = [M.cut(M.data(O, "pysrc" if s %% 2 else "text", sum(ln), first=3000 * s), ln) for s, ln in enumerate(lens)]
streams = [M.make_stream(O, a, 8) for a in arrays]
for st in streams:
    M.assert_dependent(O, st)
want = [M.model(O, st) for st in streams]
slots = [4, 1, 5, 0]
done = [0] * 4
for counts in ([1, 30, 2, 0], [2, 18, 1, 5]):
    per = [st[d:d + k] for st, d, k in zip(streams, done, counts)]
    framed = b"".join(b.framed for st in per for b in st)
    sf = np.cumsum([0] + counts)
    out, blen = eng.decompress_dstreams(framed, sf, ds, slots=slots)
    codes = [c for s in range(4) for c in want[s][0][done[s]:done[s] + counts[s]]]
    data = b"".join(o for s in range(4) for o in want[s][1][done[s]:done[s] + counts[s]])
    assert blen == codes, (blen, codes)
    assert out == data
    done = [d + k for d, k in zip(done, counts)]
# a bad length: MI355LZ4_E_ARG, and nothing is enqueued -- the slots are as they were
before = [ds.state(k) for k in range(6)]
good = b"".join(b.framed for b in streams[0][:2])
for bad in (good[:-5], (0).to_bytes(4, "little") + good[4:], good[:4] + (-7 & 0xFFFFFFFF).to_bytes(4, "little") + good[8:]):
    try:
        eng.decompress_dstreams(bad, [0, 2], ds, slots=[2], cap=1 << 20)
        raise SystemExit("a bad length was accepted")
    except S.LZ4Error as e:
        assert "(-3)" in str(e), str(e)
try:
    eng.decompress_dstreams(good, [0, 1], ds, slots=[2])          # a table that does not cover the chain
    raise SystemExit("a short table was accepted")
except S.LZ4Error as e:
    assert "(-3)" in str(e), str(e)
assert [ds.state(k) for k in range(6)] == before
ds.close()
eng.close()
print("dstreams host ok")
"""


def test_host_form_crosses_group_seams():
    env = dict(os.environ, MI355LZ4_GROUP_MB="1")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, ROOT, ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "dstreams host ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
