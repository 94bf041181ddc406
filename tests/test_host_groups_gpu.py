"""Every host-buffer compress form across the seams of the group pipeline (compress_host, csrc/host_batch.cpp).

The pipeline cuts a call into groups of about MI355LZ4_GROUP_MB and launches one device call per group with every array moved
up by the group's first block b0: the offsets, the lengths, the results, the dictionary indices, the slot base, the stream
table.  At the default 64 MiB the calls of the other test files are one group with b0 == 0, where none of that can go wrong.
Here every call runs with groups of 1 MiB (the smallest), carries 6 to 8 MiB and is cut into at least 6 groups: the stream
table's four-entry ring wraps, both pinned input slots and both output slots are reused twice, and the dictionary forms have
two groups in flight on the two compute streams.

The group size is read once per process, so every family runs in a child process of its own: this file, started as a script
with the family's name (`python tests/test_host_groups_gpu.py dict 8 0`).  A child makes one engine, runs straight through and
stops at its first failed assert.  MI355LZ4_TRACE=1 makes the pipeline name every group on stderr; the child counts the groups
of every call and the test holds the count to the cut rule restated here, so a run that went through one group fails.

What the bytes are compared with: the CPU models (dict_model for compress_dict, one OracleStream per stream for
compress_streams and the exact mode), or, where the encoder is the engine's own, the ONE device call over the whole batch
(a block's bytes do not depend on its batch: HC levels, hcdict, fastdict, fastdict_multi, level 0 without segments) -- and then
every block is decoded by the CPU oracle against its dictionary and walked by the strict validator.
"""
import ctypes as C
import os
import random
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GROUP = 1 << 20                # MI355LZ4_GROUP_MB=1
BIG = 3 << 19                  # 1.5 MiB: a block that is a group by itself (every form here takes blocks of up to 4 MiB)
BLK_E_CHECKSUM = -0x7F000004   # include/mi355lz4.h
E_BLOCK = -5


def cut_groups(lens, group=GROUP):
    """cut_groups of csrc/host_batch.cpp restated: a new group before block i when the bytes since the last cut are >= group.
    Returns the first block of every group, and len(lens) behind them."""
    first, acc = [], 0
    for i, n in enumerate(lens):
        if i == 0 or acc >= group:
            first.append(i)
            acc = 0
        acc += n
    return first + [len(lens)]


# Uniform: the cuts fall exactly where the sum equals 1 MiB, every 16 blocks.
UNIFORM = [65536] * 112
# Ragged: every length of the set, one block a group by itself, groups of 14, 9, 1, 12, 8, 16 and 3 blocks.  Group 1 and group 4
# start with an empty block; the last group is empty blocks only (no input byte at all, and the call's last blocks are empty).
# A group can only end with an empty block at the end of the call: a cut comes directly behind the block that reaches 1 MiB.
RAGGED = ([65536, 0, 1, 12, 13, 4095, 4096, 65535, 70000] + [200000] * 4 + [65536]
          + [0, 0, 1] + [200000] * 5 + [70000]
          + [BIG]
          + [13, 12, 4095, 4096, 65535, 65536] + [200000] * 4 + [70000, 200000]
          + [0, 65535, 1] + [200000] * 5
          + [4096] + [70000] * 14 + [65536]
          + [0, 0, 0])
LISTS = (("uniform", "pysrc", UNIFORM), ("ragged", "text", RAGGED))

# compress_streams: four streams in slots out of order (of a set of six).  Stream 1 is 3 MiB: the seams behind groups 0 and 1
# fall inside it.  Stream 0 is three short blocks, stream 2 lies inside group 3, stream 3 runs from group 3 to the end.
STREAM_LENS = [
    [1000, 13, 4096],
    [65536] * 48,
    [65536] * 4 + [0, 12],
    [200000] * 4 + [1 << 20] + [65535, 0, 70000, 4095] + [200000] * 5 + [0, 13, 0],
]
STREAM_SLOTS = [4, 1, 5, 0]
STREAM_CALLS = 5               # more than the ring's four entries: it wraps across calls as well as across groups
STREAM_ACCEL = [1, 1, 7, 1, 3]


def flat(streams):
    return [n for st in streams for n in st]


def multi_indices(lens):
    """compress_fastdict_multi's dictIdx for a set of five members: every group its own arrangement of -1 and the members, so
    indices that stay behind when the lengths go up by b0 name other dictionaries"""
    rng = random.Random(20261020)
    g = cut_groups(lens)
    idx = []
    for a, b in zip(g, g[1:]):
        part = [(-1, 0, 1, 2, 3, 4)[(j + a) % 6] for j in range(b - a)]
        rng.shuffle(part)
        idx += part
    return idx


def test_shapes_reach_the_seams():
    """the lists are what the comments above say, by the restated rule (no GPU)"""
    assert cut_groups([GROUP - 1, 1, 5]) == [0, 2, 3] and cut_groups([GROUP, 0, 0]) == [0, 1, 3] and cut_groups([]) == [0]
    for lens in (UNIFORM, RAGGED, flat(STREAM_LENS)):
        assert 6 << 20 <= sum(lens) <= 8 << 20
        assert len(cut_groups(lens)) - 1 >= 6
    g = cut_groups(UNIFORM)
    assert g == list(range(0, 113, 16))
    g = cut_groups(RAGGED)
    sizes = [b - a for a, b in zip(g, g[1:])]
    assert sizes == [14, 9, 1, 12, 8, 16, 3] and RAGGED[g[2]] == BIG
    assert set(RAGGED) == {0, 1, 12, 13, 4095, 4096, 65535, 65536, 70000, 200000, BIG}
    assert RAGGED[g[1]] == 0 and RAGGED[g[4]] == 0                     # groups that start with an empty block
    assert RAGGED[g[-2]:] == [0, 0, 0]                                  # the last group: empty blocks only
    g = cut_groups(flat(STREAM_LENS))
    sf = np.cumsum([0] + [len(st) for st in STREAM_LENS]).tolist()
    assert len(g) - 1 == 7
    assert sum(1 for b in g if sf[1] < b < sf[2]) == 2                 # two seams inside the 3 MiB stream
    assert sum(1 for b in g if sf[2] < b < sf[3]) == 0 and sum(1 for b in g if b == sf[2]) == 1   # stream 2: inside one group
    assert sum(1 for b in g if sf[3] < b < sf[4]) >= 2
    assert STREAM_CALLS > 4 and sorted(STREAM_SLOTS) != STREAM_SLOTS
    for lens in (UNIFORM, RAGGED):
        g, idx = cut_groups(lens), multi_indices(lens)
        pats = [idx[a:b] for a, b in zip(g, g[1:])]
        assert len(idx) == len(lens) and -1 in idx
        assert all(p != q for p, q in zip(pats, pats[1:]))             # no two consecutive groups alike,
        assert all(len(set(p) - {-1}) >= 3 for p in pats if len(p) >= 6)   # every group of some size names several members,
        assert idx[:len(pats[1])] != pats[1]                           # and group 0's indices are not group 1's


# ---- the tests: one child per family -------------------------------------------------------------------------------------------
def run_child(calls, family, *args):
    """Runs the family's child with groups of 1 MiB and the trace on; every call it reports went through the restated rule's
    number of groups, at least 6, and it reports `calls` of them."""
    env = dict(os.environ, MI355LZ4_GROUP_MB="1", MI355LZ4_TRACE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), family] + [str(a) for a in args], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "host groups ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    seen = re.findall(r"^call (\S+) blocks (\d+) groups (\d+)$", r.stdout, re.M)
    assert len(seen) == calls, r.stdout[-3000:]
    rule = {"uniform": UNIFORM, "ragged": RAGGED, "streams": flat(STREAM_LENS), "exact": UNIFORM[:96]}
    for name, blocks, groups in seen:
        lens = rule[name.split("/")[0]]
        assert int(blocks) == len(lens), name
        assert int(groups) == len(cut_groups(lens)) - 1 and int(groups) >= 6, (name, groups)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [4, 8])
@pytest.mark.parametrize("checksum", [0, 1])
def test_compress_dict(kind, checksum):
    """every block is the CPU model's LZ4_loadDict + LZ4_compress_fast_continue, accel 1 and 7; with checksums the CPU's
    trailers, and decompress_dict names exactly the two blocks that were damaged"""
    run_child(4, "dict", kind, checksum)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,checksum", [(8, 0), (4, 0), (8, 1)])
def test_compress_streams(kind, checksum):
    """five calls in a row on the same four slots: every slot's blocks, joined over the calls, are one oracle stream"""
    run_child(STREAM_CALLS, "streams", kind, checksum)


@pytest.mark.gpu
def test_exact_mode():
    """compress_batch in exact mode, two calls over the uniform list and one over the ragged: one oracle stream over all arrays"""
    run_child(3, "exact")


@pytest.mark.gpu
@pytest.mark.parametrize("level", [3, 9])
def test_hc_levels(level):
    """compress_batch at an HC level is the one device call over the whole batch; every block valid, every block decodes"""
    run_child(2, "hc", level)


@pytest.mark.gpu
def test_compress_hcdict():
    """level 3 against a prepared dictionary is the one device call; every block decodes against the kept bytes"""
    run_child(2, "hcdict", 3)


@pytest.mark.gpu
@pytest.mark.parametrize("checksum", [0, 1])
def test_compress_fastdict(checksum):
    """accel 1 and 7, staged and with page-locked buffers; with checksums the CPU's trailers and the damaged blocks named"""
    run_child(6, "fastdict", checksum)


@pytest.mark.gpu
def test_compress_fastdict_multi():
    """five members, one of them empty, and -1, shuffled per group: the one device call's bytes, decoded member by member"""
    run_child(2, "multi")


@pytest.mark.gpu
def test_level0_without_segments():
    """set_segments(0): one wave per block, so compress_batch is the one device call over the whole batch"""
    run_child(2, "level0")


# ---- the child -----------------------------------------------------------------------------------------------------------------
_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)


class Child:
    """one engine, the oracle, and the calls"""

    def __init__(self):
        import torch
        import streamly_lz4_amd as S
        import dstreams_model as M
        from oracle.oracle import Oracle
        self.torch, self.S, self.M = torch, S, M
        self.O = Oracle()
        self.eng = S.Engine(0)
        self.checksum = False

    def set_checksum(self, on):
        self.checksum = bool(on)
        self.eng.set_block_checksum(self.checksum)

    def blocks(self, kind, lens, first=0):
        """text-like bytes cut into blocks: every block its own content"""
        return self.M.cut(self.M.data(self.O, kind, sum(lens), first=first), lens)

    def dictionary(self, n, seed):
        """n bytes in the words of the blocks, half text and half Python source: the blocks do reach into it"""
        t = self.O.gen("text", 1, n // 2, first_block=1000 + seed).tobytes()
        return t + self.M.data(self.O, "pysrc", n - len(t), first=7500000 + 50000 * seed)

    def device_tensor(self, b):
        return self.torch.from_numpy(np.frombuffer(bytes(b) + bytes(16), dtype=np.uint8).copy()).cuda()

    def traced(self, fn):
        """fn() with stderr caught: (its result, the distinct groups the pipeline named, whether the input went directly)"""
        sys.stderr.flush()
        saved = os.dup(2)
        with tempfile.TemporaryFile() as tmp:
            os.dup2(tmp.fileno(), 2)
            try:
                r = fn()
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            txt = tmp.read().decode(errors="replace")
        sys.stderr.write(txt[-2000:])
        hits = re.findall(r"compress: group (\d+) H2D enqueued \(\d+ bytes, direct (\d)\)", txt)
        return r, len(set(g for g, _ in hits)), set(d for _, d in hits)

    def host(self, name, fn, head, blocks, mid, kind, pinned=False):
        """One host-buffer compress call, fn(ctx, *head, src, srcLen, n, *mid, kind, out, cap, &outLen, framedLen, status).
        Checks the group count, outLen, blockFramedLen[] and status[]; returns (the framed bytes, blockFramedLen)."""
        torch, S = self.torch, self.S
        n = len(blocks)
        lens = [len(b) for b in blocks]
        ln = np.array(lens + [0], dtype=np.int32)
        cap = sum(S.compress_bound(x) + kind + 4 for x in lens) + 16
        if pinned:                                 # back to back, every start 16-aligned, page-locked: the direct path both ways
            offs = np.cumsum([0] + [(x + 15) & ~15 for x in lens])
            buf = torch.zeros(int(offs[-1]) + 16, dtype=torch.uint8).pin_memory()
            for o, b in zip(offs, blocks):
                buf.numpy()[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
            ptrs = (_u8p * n)(*[C.cast(buf.data_ptr() + int(o), _u8p) for o in offs[:n]])
            out_t = torch.full((cap,), 0xEE, dtype=torch.uint8).pin_memory()
            out, out_p = out_t.numpy(), C.cast(out_t.data_ptr(), _u8p)
        else:
            arrs = [np.frombuffer(b, dtype=np.uint8) for b in blocks]
            ptrs = (_u8p * n)(*[a.ctypes.data_as(_u8p) for a in arrs])
            out = np.full(cap, 0xEE, dtype=np.uint8)
            out_p = out.ctypes.data_as(_u8p)
        flen = np.full(n + 1, -77, dtype=np.int32)
        st = np.full(n + 1, -77, dtype=np.int32)
        olen = C.c_size_t(99)
        rc, groups, direct = self.traced(lambda: fn(self.eng.ctx, *head, ptrs, ln.ctypes.data_as(_i32p), n, *mid, kind, out_p, cap,
                                                    C.byref(olen), flen.ctypes.data_as(_i32p), st.ctypes.data_as(_i32p)))
        assert rc == 0, (name, rc, S.lib.mi355lz4_last_error())
        want = len(cut_groups(lens)) - 1
        assert groups == want and groups >= 6, (name, groups, want)
        assert direct == ({"1"} if pinned else {"0"}), (name, direct)
        fl = flen[:n].tolist()
        trailer = 4 if self.checksum else 0
        assert flen[n] == -77 and st[n] == -77, name
        assert min(fl) > kind + trailer, (name, fl)
        assert st[:n].tolist() == [f - kind - trailer for f in fl], name
        assert olen.value == sum(fl), (name, olen.value, sum(fl))
        assert (out[olen.value:] == 0xEE).all(), name                  # nothing behind the stream
        print("call %s blocks %d groups %d" % (name, n, groups), flush=True)
        return out[:olen.value].tobytes(), fl

    def device(self, call, blocks, kind):
        """The one device call over the whole batch, call(src, n, maxLen, slots, stride, framedLen, src_off, src_len), the
        blocks 16-aligned with a gap between them; returns (the slots compacted, framedLen)."""
        torch, S = self.torch, self.S
        n = len(blocks)
        lens = [len(b) for b in blocks]
        offs = np.cumsum([0] + [((x + 15) & ~15) + 16 for x in lens])
        buf = np.zeros(int(offs[-1]) + 64, dtype=np.uint8)
        for o, b in zip(offs, blocks):
            buf[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
        mx = max(lens)
        stride = S.slot_stride_ex(mx, kind, self.checksum)
        src = torch.from_numpy(buf).cuda()
        off = torch.tensor(offs.tolist(), dtype=torch.int64).cuda()
        ln = torch.tensor(lens + [0], dtype=torch.int32).cuda()
        slots = torch.zeros(n * stride, dtype=torch.uint8).cuda()
        flen = torch.full((n,), -7, dtype=torch.int32).cuda()
        call(src, n, mx, slots, stride, flen, off, ln)
        torch.cuda.synchronize()
        fl = flen.cpu().tolist()
        assert min(fl) > kind, fl
        return torch.cat([slots[i * stride:i * stride + fl[i]] for i in range(n)]).cpu().numpy().tobytes(), fl

    def split(self, framed, fl, kind):
        """the compressed bytes of every block of a framed stream"""
        out, p = [], 0
        trailer = 4 if self.checksum else 0
        for f in fl:
            assert int.from_bytes(framed[p:p + 4], "little") == f - kind - trailer
            out.append(framed[p + kind:p + f - trailer])
            p += f
        assert p == len(framed)
        return out

    def same(self, name, got, fl, want, wfl):
        """byte equality with the first differing block named"""
        if got == want and fl == wfl:
            return
        p = 0
        for i, (a, b) in enumerate(zip(fl, wfl)):
            assert a == b and got[p:p + a] == want[p:p + a], "%s: block %d of %d differs (framed %d, expected %d)" % (name, i, len(fl), a, b)
            p += a
        raise AssertionError("%s: %d blocks for %d" % (name, len(fl), len(wfl)))

    def decodes(self, name, comps, blocks, kept, every=False):
        """every block decodes to its input on the CPU against its dictionary's kept bytes (kept: one for all, or one per
        block); the first and last block of every group pass the strict validator (all blocks: every=True)"""
        from lz4_check import check_block
        per = kept if isinstance(kept, list) else [kept] * len(blocks)
        g = cut_groups([len(b) for b in blocks])
        ends = set(g[:-1]) | set(b - 1 for b in g[1:])
        reached = 0
        for i, (c, b, d) in enumerate(zip(comps, blocks, per)):
            r, out = self.O.decompress_block(c, len(b), dict_bytes=d or None)
            assert r == len(b) and out == b, "%s: block %d decodes to %d of %d bytes" % (name, i, r, len(b))
            if every or i in ends:
                try:
                    into = check_block(c, len(b), len(d or b""))[3]
                except AssertionError as e:
                    raise AssertionError("%s: block %d: %s" % (name, i, e))
                reached += bool(d) and into > 0
        return reached

    def damaged(self, framed, fl, kind, data_block, trailer_block):
        """the stream with one data byte of data_block and one trailer byte of trailer_block wrong"""
        bad = bytearray(framed)
        at = np.cumsum([0] + fl).tolist()
        bad[at[data_block] + kind] ^= 0x40
        bad[at[trailer_block + 1] - 1] ^= 0x01
        return bytes(bad)


def two_groups_apart(lens):
    """(the first block of a middle group, the last block of the group behind it): where the checksum runs do damage"""
    g = cut_groups(lens)
    mid = (len(g) - 1) // 2
    return g[mid], g[mid + 2] - 1


def child_dict(kind, checksum):
    """1. compress_dict against the CPU model, 6. its trailers and decompress_dict"""
    import dict_model as DM
    from test_compress_streams_gpu import frame_block
    w = Child()
    S, L = w.S, w.S.lib
    w.set_checksum(checksum)
    d = w.dictionary(70000, 1)
    cs = S.CompressStreams(w.eng, 3)
    cs.load_dict(1, w.device_tensor(d), len(d))
    loaded = DM.model_load(d)
    for name, data, lens in LISTS:
        blocks = w.blocks(data, lens, first=11)
        by_accel = {}
        for accel in (1, 7):
            model = [DM.model_compress(loaded, b, accel) for b in blocks]
            if checksum:
                want = [frame_block(c, b, kind, True) for (r, c), b in zip(model, blocks)]
            else:
                want = [DM.framed_block(r, c, len(b), kind) for (r, c), b in zip(model, blocks)]
            tag = "%s/dict/a%d" % (name, accel)
            framed, fl = w.host(tag, L.mi355lz4_compress_dict, (cs._h, 1), blocks, (accel,), kind)
            w.same(tag, framed, fl, b"".join(want), [len(x) for x in want])
            by_accel[accel] = framed
        assert by_accel[1] != by_accel[7]
        if checksum and kind == 8:
            # mi355lz4_decompress_dict is one group whatever the group size; on a failed block it returns the codes and no bytes
            # (host_tail), so the bytes are those of the undamaged run
            out, blen = w.eng.decompress_dict(framed, d)
            assert blen == lens and out == b"".join(blocks), tag
            x, y = two_groups_apart(lens)
            out, blen = w.eng.decompress_dict(w.damaged(framed, fl, kind, x, y), d, raise_on_block_error=False)
            assert blen == [BLK_E_CHECKSUM if i in (x, y) else n for i, n in enumerate(lens)], (tag, x, y)
    cs.close()
    w.eng.close()
    print("host groups ok")


def child_streams(kind, checksum):
    """2. compress_streams: slots that continue through the seams of a call and from call to call, 6. trailers and decode"""
    from test_compress_streams_gpu import OracleStream, framed_by
    w = Child()
    S, L = w.S, w.S.lib
    w.set_checksum(checksum)
    cs = S.CompressStreams(w.eng, 6)
    oracle = {k: OracleStream() for k in STREAM_SLOTS}
    lens = flat(STREAM_LENS)
    total = sum(lens)
    sf = np.cumsum([0] + [len(st) for st in STREAM_LENS]).astype(np.int32)
    text = w.M.data(w.O, "text", STREAM_CALLS * total, first=5)
    for k in range(STREAM_CALLS):
        # the same table every call, the slots moved round: a slot gets another stream's shape each time
        slots = STREAM_SLOTS[k % 4:] + STREAM_SLOTS[:k % 4]
        blocks = w.M.cut(text[k * total:(k + 1) * total], lens)
        accel = STREAM_ACCEL[k]
        want = []
        for s, slot in enumerate(slots):
            want += framed_by(oracle[slot], blocks[sf[s]:sf[s + 1]], accel, kind, bool(checksum))
        sl = np.array(slots, dtype=np.int32)
        tag = "streams/call%d" % k
        framed, fl = w.host(tag, L.mi355lz4_compress_streams, (cs._h,), blocks,
                            (sf.ctypes.data_as(_i32p), sl.ctypes.data_as(_i32p), len(slots), accel), kind)
        w.same(tag, framed, fl, b"".join(want), [len(x) for x in want])
        if k == 0 and checksum and kind == 8:
            # Fresh streams one behind the other read as ONE linked stream: a stream's first block reaches into nothing.  The
            # damage goes to the last block of stream 1 (group 2) and of stream 2 (group 3): no block depends on those.
            x, y = int(sf[2]) - 1, int(sf[3]) - 1
            g = cut_groups(lens)
            assert g[2] <= x < g[3] <= y < g[4]
            out, blen = w.eng.decompress_batch(framed, linked=True)
            assert blen == lens and out == b"".join(blocks)
            bad = np.frombuffer(w.damaged(framed, fl, kind, x, y), dtype=np.uint8)
            out = np.full(total + 16, 0xEE, dtype=np.uint8)
            res = np.full(len(lens), -77, dtype=np.int32)
            olen, got = C.c_size_t(), C.c_int()
            rc = L.mi355lz4_decompress_batch(w.eng.ctx, bad.ctypes.data_as(_u8p), bad.size, kind, 0, 1, None, 0, out.ctypes.data_as(_u8p),
                                             out.size, C.byref(olen), res.ctypes.data_as(_i32p), len(lens), C.byref(got))
            assert rc == E_BLOCK and got.value == len(lens), (rc, got.value)
            assert res.tolist() == [BLK_E_CHECKSUM if i in (x, y) else n for i, n in enumerate(lens)], (x, y)
            at = np.cumsum([0] + lens).tolist()                        # every other block's bytes, at its place of the layout
            for i, b in enumerate(blocks):
                assert i in (x, y) or out[at[i]:at[i + 1]].tobytes() == b, i
    cs.close()
    w.eng.close()
    print("host groups ok")


def child_exact():
    """3. the engine's own exact stream through three calls of six and seven groups"""
    from test_compress_streams_gpu import OracleStream, framed_by
    w = Child()
    L = w.S.lib
    w.eng.set_compress_exact(True)
    lens = UNIFORM[:96]
    arrays = w.blocks("text", lens * 2, first=77)
    o = OracleStream()
    # (a third call goes on with the ragged list: in the uniform one every length is the same, and the exact encoder plans its
    # pieces from the host's lengths, which go up with b0 too)
    calls = [("exact/call%d" % k, arrays[k * 96:(k + 1) * 96]) for k in range(2)] + [("ragged/exact", w.blocks("text", RAGGED, first=31))]
    for tag, blocks in calls:
        want = framed_by(o, blocks, 1, 8)
        framed, fl = w.host(tag, L.mi355lz4_compress_batch, (), blocks, (1,), 8)
        w.same(tag, framed, fl, b"".join(want), [len(x) for x in want])
    w.eng.close()
    print("host groups ok")


def child_hc(level):
    """4. an HC level: one workgroup per block, so the groups' bytes are the whole batch's"""
    w = Child()
    L = w.S.lib
    w.eng.set_compression_level(level)
    for name, data, lens in LISTS:
        blocks = w.blocks(data, lens, first=300)
        tag = "%s/hc%d" % (name, level)
        want, wfl = w.device(lambda src, n, mx, slots, stride, flen, off, ln: w.eng.compress_batch_device(
            src, n, mx, slots, stride, flen, header_kind=8, src_off=off, src_len=ln, block_stride=0), blocks, 8)
        framed, fl = w.host(tag, L.mi355lz4_compress_batch, (), blocks, (1,), 8)
        w.same(tag, framed, fl, want, wfl)
        w.decodes(tag, w.split(framed, fl, 8), blocks, None, every=True)
    w.eng.close()
    print("host groups ok")


def child_hcdict(level):
    """5. compress_hcdict: per-stream staging windows used from both compute streams"""
    w = Child()
    S, L = w.S, w.S.lib
    w.eng.set_compression_level(level)
    d = w.dictionary(70000, 2)
    hd = S.HcDict(w.eng)
    hd.load(w.device_tensor(d), len(d))
    kept = d[-65536:]
    for name, data, lens in LISTS:
        blocks = w.blocks(data, lens, first=4000)
        tag = "%s/hcdict%d" % (name, level)
        want, wfl = w.device(lambda src, n, mx, slots, stride, flen, off, ln: w.eng.compress_hcdict_device(
            hd, src, n, mx, slots, stride, flen, header_kind=8, src_off=off, src_len=ln, block_stride=0), blocks, 8)
        framed, fl = w.host(tag, L.mi355lz4_compress_hcdict, (hd._h,), blocks, (), 8)
        w.same(tag, framed, fl, want, wfl)
        assert w.decodes(tag, w.split(framed, fl, 8), blocks, kept) >= 6, tag      # the dictionary is in use
    hd.close()
    w.eng.close()
    print("host groups ok")


def child_fastdict(checksum):
    """5. compress_fastdict, 8. with page-locked buffers, 6. its trailers and decompress_dict"""
    from test_compress_streams_gpu import frame_block
    w = Child()
    S, L = w.S, w.S.lib
    w.set_checksum(checksum)
    d = w.dictionary(70000, 3)
    hd = S.HcDict(w.eng)
    hd.load(w.device_tensor(d), len(d))
    kept = d[-65536:]
    for name, data, lens in LISTS:
        blocks = w.blocks(data, lens, first=9000)
        for accel in (1, 7):
            tag = "%s/fastdict/a%d" % (name, accel)
            want, wfl = w.device(lambda src, n, mx, slots, stride, flen, off, ln: w.eng.compress_fastdict_device(
                hd, src, n, mx, slots, stride, flen, accel=accel, header_kind=8, src_off=off, src_len=ln, block_stride=0), blocks, 8)
            framed, fl = w.host(tag, L.mi355lz4_compress_fastdict, (hd._h,), blocks, (accel,), 8)
            w.same(tag, framed, fl, want, wfl)
            comps = w.split(framed, fl, 8)
            assert w.decodes(tag, comps, blocks, kept) >= 6, tag
            if checksum:                           # the trailers are the CPU's
                assert framed == b"".join(frame_block(c, b, 8, True) for c, b in zip(comps, blocks)), tag
        # page-locked input and output: no staging slot either way, the same bytes
        tag = "%s/fastdict/pinned" % name
        pinned, pfl = w.host(tag, L.mi355lz4_compress_fastdict, (hd._h,), blocks, (7,), 8, pinned=True)
        w.same(tag, pinned, pfl, framed, fl)
        if checksum:                               # (one group, and codes without bytes on a failure: see child_dict)
            out, blen = w.eng.decompress_dict(framed, d)
            assert blen == lens and out == b"".join(blocks), tag
            x, y = two_groups_apart(lens)
            out, blen = w.eng.decompress_dict(w.damaged(framed, fl, 8, x, y), d, raise_on_block_error=False)
            assert blen == [BLK_E_CHECKSUM if i in (x, y) else n for i, n in enumerate(lens)], (tag, x, y)
    hd.close()
    w.eng.close()
    print("host groups ok")


def child_multi():
    """5. compress_fastdict_multi: the indices go up with the lengths"""
    w = Child()
    S, L = w.S, w.S.lib
    dicts = [w.dictionary(70000, 4), w.dictionary(65536, 5), b"", w.dictionary(4095, 6), w.dictionary(20000, 7)]
    members = [S.HcDict(w.eng) for _ in dicts]
    for m, d in zip(members, dicts):
        if d:                                      # (member 2 stays the empty dictionary)
            m.load(w.device_tensor(d), len(d))
    ds = S.DictSet(w.eng, members)
    for name, data, lens in LISTS:
        blocks = w.blocks(data, lens, first=70000)
        idx = multi_indices(lens)
        tag = "%s/multi" % name
        idx_t = w.torch.tensor(idx + [0], dtype=w.torch.int32).cuda()
        want, wfl = w.device(lambda src, n, mx, slots, stride, flen, off, ln: w.eng.compress_fastdict_multi_device(
            ds, idx_t, src, n, mx, slots, stride, flen, accel=1, header_kind=8, src_off=off, src_len=ln, block_stride=0), blocks, 8)
        ix = np.array(idx + [0], dtype=np.int32)
        framed, fl = w.host(tag, L.mi355lz4_compress_fastdict_multi, (ds._h, ix.ctypes.data_as(_i32p)), blocks, (1,), 8)
        # (no look at mi355lz4_debug_dictset_last behind a host call: the groups in flight on the two compute streams share
        # that word, so what it holds afterwards is any group's)
        w.same(tag, framed, fl, want, wfl)
        kept = [dicts[k][-65536:] if k >= 0 else b"" for k in idx]
        assert w.decodes(tag, w.split(framed, fl, 8), blocks, kept) >= 4, tag
        out, blen = w.eng.decompress_dict_multi(framed, ds, idx)
        assert blen == lens and out == b"".join(blocks), tag
    ds.close()
    for m in members:
        m.close()
    w.eng.close()
    print("host groups ok")


def child_level0():
    """7. level 0 with the segmented encoder off: one wave per block, the groups' bytes are the whole batch's"""
    w = Child()
    L = w.S.lib
    w.eng.set_segments(0)
    for name, data, lens in LISTS:
        blocks = w.blocks(data, lens, first=123)
        tag = "%s/level0" % name
        want, wfl = w.device(lambda src, n, mx, slots, stride, flen, off, ln: w.eng.compress_batch_device(
            src, n, mx, slots, stride, flen, accel=1, header_kind=8, src_off=off, src_len=ln, block_stride=0), blocks, 8)
        framed, fl = w.host(tag, L.mi355lz4_compress_batch, (), blocks, (1,), 8)
        w.same(tag, framed, fl, want, wfl)
        w.decodes(tag, w.split(framed, fl, 8), blocks, None)
    w.eng.close()
    print("host groups ok")


if __name__ == "__main__":
    globals()["child_" + sys.argv[1]](*[int(a) for a in sys.argv[2:]])
