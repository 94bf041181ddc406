"""Fast linked streams at a set's own level: mi355lz4_fstreams_set_level / _get_level.

The engine's level stays 0 -- it selects the encoder of the batch calls -- and the set's level L in 1..12 selects the hash-chain
encoder for mi355lz4_compress_streams_fast_device / _compress_streams_fast.  The contract is level 0's with the other encoder on
its right-hand side: block k of a stream is, byte for byte, what mi355lz4_compress_batch_device with the linked switch on and the
ENGINE at level L writes for the second block of the contiguous two-block call [D, B_k] with max(|D|, maxBlockLen) as its
maxBlockLen; with an empty D the block of the one-block linked call.  D is the last min(len, 65536) bytes of the block before it
in its stream -- what the slot holds, for a stream's first block of a call.

The helpers are those of tests/test_fstreams_gpu.py (placement with gaps, the pair oracle), restated here with a level."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dstreams_model as M  # noqa: E402
import lz4_check  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG = -3
APART = 7
FILL = 0xA5
KNOB = "MI355LZ4_HSTREAMS_GROUPS"
NSLOTS = 80
# the all-literals edge, one parse round (1024 positions) and one more or less, two rounds and a bit, the ring's 65536 positions,
# and blocks whose positions wrap the ring
BLOCK_LENS = [0, 1, 12, 13, 14, 1023, 1024, 1025, 2053, 65536, 70000, 100000]
# none; fewer than a hash's four bytes; four and one more; the shortest block with a match; a round and one more or less; the
# whole window and one less; more than a slot keeps
DICT_LENS = [0, 1, 3, 4, 5, 12, 1023, 1024, 1025, 65535, 65536, 70000]
MAXLEN = 100000


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rnd(seed, n):
    return np.random.RandomState(seed).randint(0, 256, size=n).astype(np.uint8).tobytes()


@pytest.fixture(scope="module")
def setup():
    import streamly_lz4_amd as S
    os.environ.pop(KNOB, None)
    eng = S.Engine(0)
    fs = S.FastCompressStreams(eng, NSLOTS)
    yield S, eng, fs
    os.environ.pop(KNOB, None)
    fs.close()
    eng.close()


def place(blocks, glue=(), lead=3):
    """the blocks in one buffer, APART bytes apart, laid down in a permuted order; block i of `glue` lies directly behind block
    i - 1.  (buffer, offsets)"""
    runs = []
    for i in range(len(blocks)):
        if i in glue and runs:
            runs[-1].append(i)
        else:
            runs.append([i])
    order = [runs[k] for k in np.random.RandomState(len(blocks)).permutation(len(runs))]
    off, pos = [0] * len(blocks), lead
    for run in order:
        for i in run:
            off[i] = pos
            pos += len(blocks[i])
        pos += APART
    buf = np.full(pos + 64, FILL, dtype=np.uint8)
    for o, d in zip(off, blocks):
        buf[o:o + len(d)] = np.frombuffer(bytes(d), dtype=np.uint8)
    return buf, off


def followers(streams):
    """the flat indices of every block that has a block of its stream in front of it in the call"""
    out, i = set(), 0
    for st in streams:
        out |= set(range(i + 1, i + len(st)))
        i += len(st)
    return out


def fs_call(S, eng, fs, streams, level, slots=None, accel=1, kind=8, checksum=False, lens=None, maxlen=None, glue=(), groups=None):
    """one compress_streams_fast_device call with the set at `level` (put back to 0 behind it): streams[s] = the blocks stream s
    brings, continuing slot slots[s] (default s).  Returns (framedLen[], [slot bytes up to framedLen], all slots as rows)"""
    import torch
    blocks = [b for st in streams for b in st]
    n = len(blocks)
    sf = np.cumsum([0] + [len(st) for st in streams]).astype(np.int32)
    slots_of = list(range(len(streams))) if slots is None else list(slots)
    mx = max([len(b) for b in blocks] + [1]) if maxlen is None else maxlen
    buf, off = place(blocks, glue)
    stride = S.slot_stride_ex(mx, kind, checksum)
    out = torch.full((max(n, 1) * stride,), FILL, dtype=torch.uint8, device=DEV)
    flen = torch.full((max(n, 1),), -77, dtype=torch.int32, device=DEV)
    eng.set_compression_level(0)
    eng.set_block_checksum(checksum)
    fs.set_level(level)
    assert fs.level == level
    if groups is not None:
        os.environ[KNOB] = str(groups)
    try:
        src = _t(buf)
        eng.compress_streams_fast_device(fs, src, n, mx, sf, slots_of, out, stride, flen, accel=accel, header_kind=kind,
                                         src_off=_t(np.array(off + [0], dtype=np.int64)),
                                         src_len=_t(np.array(([len(b) for b in blocks] if lens is None else list(lens)) + [0],
                                                             dtype=np.int32)), block_stride=0)
        fs.set_level(0)                           # a call already enqueued keeps its level
        eng.synchronize()
        untouched = src.cpu().numpy()
        assert (untouched == buf).all(), "src was written"
        src.fill_(0x3C)                           # the call has run: the slot owns its copy
        eng.synchronize()
    finally:
        fs.set_level(0)
        eng.set_block_checksum(False)
        os.environ.pop(KNOB, None)
    fl, hb = flen.cpu().tolist()[:n], out.cpu().numpy()
    return fl, [hb[i * stride:i * stride + max(fl[i], 0)].tobytes() for i in range(n)], hb.reshape(max(n, 1), stride)


def payloads(fl, got, blocks, kind=8, trailer=0):
    out = []
    for f, g, b in zip(fl, got, blocks):
        assert f == len(g) and f > kind and int.from_bytes(g[:4], "little") == f - kind - trailer, (f, len(b))
        if kind == 8:
            assert int.from_bytes(g[4:8], "little") == len(b)
        out.append(g[kind:len(g) - trailer])
    return out


def linked_batch(S, eng, data, offs, lens, big, level, accel=1):
    """ONE linked compress_batch_device call with the engine at `level`: the payload of every block"""
    import torch
    n = len(offs)
    stride = S.slot_stride_ex(big, 8, False)
    slots = torch.full((n * stride,), FILL, dtype=torch.uint8, device=DEV)
    flen = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    eng.set_compression_level(level)
    eng.set_linked_compress(True)
    try:
        eng.compress_batch_device(_t(data), n, big, slots, stride, flen, accel=accel, header_kind=8,
                                  src_off=_t(np.array(offs, dtype=np.int64)), src_len=_t(np.array(lens, dtype=np.int32)), block_stride=0)
        eng.synchronize()
    finally:
        eng.set_linked_compress(False)
        eng.set_compression_level(0)
    fl, hb = flen.cpu().tolist(), slots.cpu().numpy()
    return [hb[i * stride + 8:i * stride + fl[i]].tobytes() for i in range(n)]


_oracle_cache = {}


def pair_oracle(S, eng, pairs, level, maxlen=None, key=None):
    """The contract's right-hand side: all pairs [D, B] in one buffer with gaps between the pairs, ONE linked
    compress_batch_device call with the engine at `level` and max(|D|, maxlen) as its maxBlockLen; the payload of every pair's
    second block (an empty D: the one-block pair [B]).  Computed once per (key, level)."""
    if key is not None and (key, level) in _oracle_cache:
        return _oracle_cache[(key, level)]
    mx = max([len(b) for _, b in pairs] + [1]) if maxlen is None else maxlen
    parts, offs, second, pos = [], [], [], 5
    for d, b in pairs:
        assert len(d) <= 65536
        if d:
            parts.append(bytes(d))
            offs.append(pos)
            pos += len(d)
        second.append(len(offs))
        parts.append(bytes(b))
        offs.append(pos)
        pos += len(b) + APART + 4             # the gap: the next pair is not linked to this one
    data = np.full(pos + 64, FILL, dtype=np.uint8)
    for o, x in zip(offs, parts):
        data[o:o + len(x)] = np.frombuffer(x, dtype=np.uint8)
    big = max([len(d) for d, _ in pairs] + [mx])
    all_blocks = linked_batch(S, eng, data, offs, [len(x) for x in parts], big, level)
    out = [all_blocks[i] for i in second]
    if key is not None:
        _oracle_cache[(key, level)] = out
    return out


def dict_pairs(streams, held=None):
    """[(D, B)] for every block of every stream; held[s] = what stream s's slot holds before (default: nothing)"""
    out = []
    for s, st in enumerate(streams):
        prev = b"" if held is None else held[s]
        for b in st:
            out.append((bytes(prev[-65536:]), bytes(b)))
            prev = bytes(b)
    return out


def contiguous_linked(S, eng, streams, level, maxlen=None):
    """every stream laid out contiguously, one byte between the streams, ONE linked compress_batch_device call: payload per block"""
    blocks = [b for st in streams for b in st]
    mx = max([len(b) for b in blocks] + [1]) if maxlen is None else maxlen
    offs, pos = [], 9
    for st in streams:
        for b in st:
            offs.append(pos)
            pos += len(b)
        pos += 1
    data = np.full(pos + 64, FILL, dtype=np.uint8)
    for o, b in zip(offs, blocks):
        data[o:o + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    return linked_batch(S, eng, data, offs, [len(b) for b in blocks], mx, level)


# ---- the streams ---------------------------------------------------------------------------------------------------------------
def text_stream(oracle, lens, first):
    """blocks that overlap each other in a text: a block's predecessor holds most of what it holds"""
    text = M.data(oracle, "text", 400000, first=first)
    return [text[1000 * k + 37 * (k % 3):1000 * k + 37 * (k % 3) + n] for k, n in enumerate(lens)]


def random_stream(seed, lens):
    """slices of one random buffer: only the link makes them compressible"""
    r = rnd(seed, max(lens) + 400)
    return [r[(53 * k) % 300:(53 * k) % 300 + n] for k, n in enumerate(lens)]


def edge_streams(oracle):
    """12 streams of 12 blocks: stream j's slot holds a dictionary of DICT_LENS[j] bytes (the text in front of its first block)
    and its blocks have BLOCK_LENS rotated by j, so every length stands first behind a slot once and behind every other length's
    neighbour.  (streams, [dictionary handed to set_dict per stream])"""
    text = M.data(oracle, "text", 400000, first=5)
    streams, dicts = [], []
    for j, dl in enumerate(DICT_LENS):
        base = 72000 + 3000 * j
        lens = BLOCK_LENS[j:] + BLOCK_LENS[:j]
        streams.append([text[base + 700 * k:base + 700 * k + n] for k, n in enumerate(lens)])
        dicts.append(text[base + 400 - dl:base + 400])
    return streams, dicts


def mixed_streams(oracle):
    """text and random streams of five blocks, lengths up to 100000 on both sides of 65536, empty blocks in the middle"""
    return [text_stream(oracle, [4096, 65536, 65535, 75, 13], 11),
            text_stream(oracle, [75, 0, 4096, 12, 4096], 5003),
            random_stream(7, [65536, 65535, 4096, 75, 13]),
            text_stream(oracle, [1, 13, 65536, 0, 65536], 977),
            text_stream(oracle, [100000, 65537, 4096, 100000, 13], 31),
            random_stream(9, [65537, 100000, 75, 65536, 0])]


def load_dicts(eng, fs, dicts):
    fs.reset()
    keep = []
    for s, d in enumerate(dicts):
        t = _t(np.frombuffer(bytes(d) + b"\0", dtype=np.uint8).copy())
        fs.set_dict(s, t, len(d))
        keep.append(t)
    eng.synchronize()
    return [bytes(d[-65536:]) for d in dicts]


# ---- 1. the pair contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("level", [1, 4, 9, 12])
def test_contract_every_block_is_the_linked_pair_s_second_block(setup, oracle, level, kind):
    S, eng, fs = setup
    streams, dicts = edge_streams(oracle)
    blocks = [b for st in streams for b in st]
    held = load_dicts(eng, fs, dicts)
    assert [fs.peek(s)[0] for s in range(len(dicts))] == [min(d, 65536) for d in DICT_LENS]
    want = pair_oracle(S, eng, dict_pairs(streams, held), level, MAXLEN, key="edges")
    # D from the block before in the call: apart (staged), then directly in front (in place); the bytes are the same
    for glue in (set(), followers(streams)):
        load_dicts(eng, fs, dicts)
        fl, got, _ = fs_call(S, eng, fs, streams, level, kind=kind, maxlen=MAXLEN, glue=glue)
        have = payloads(fl, got, blocks, kind)
        for i, (h, w) in enumerate(zip(have, want)):
            assert h == w, (level, kind, bool(glue), "block %d of %d bytes" % (i, len(blocks[i])), len(h), len(w))
        assert [fs.peek(s) for s in range(len(streams))] == [(min(len(st[-1]), 65536), bytes(st[-1][-65536:])) for st in streams]
    # the link was really used: blocks are smaller than they are without their dictionary
    alone = pair_oracle(S, eng, [(b"", b) for b in blocks], level, MAXLEN, key="edges alone")
    assert sum(len(h) < len(a) for h, a in zip(want, alone)) >= 40
    if level == 12:                                                      # levels 10..12 search as 9
        assert want == pair_oracle(S, eng, dict_pairs(streams, held), 9, MAXLEN, key="edges")
    if level == 9:                                                       # accel is ignored
        load_dicts(eng, fs, dicts)
        fl7, got7, _ = fs_call(S, eng, fs, streams, level, kind=kind, maxlen=MAXLEN, accel=7)
        assert (fl7, got7) == (fl, got)


# ---- 2. cut independence -----------------------------------------------------------------------------------------------------------
def feed(S, eng, fs, streams, partition, level, **kw):
    """the streams cut into calls: partition[c][s] = blocks of stream s in call c; per flat block (framedLen, slot bytes)"""
    done = [0] * len(streams)
    out = [[] for _ in streams]
    for counts in partition:
        per = [st[d:d + k] for st, d, k in zip(streams, done, counts)]
        fl, got, _ = fs_call(S, eng, fs, per, level, **kw)
        sf = np.cumsum([0] + list(counts))
        for s, k in enumerate(counts):
            out[s] += list(zip(fl[sf[s]:sf[s + 1]], got[sf[s]:sf[s + 1]]))
            done[s] += k
    assert done == [len(st) for st in streams]
    return [x for st in out for x in st]


@pytest.fixture(scope="module")
def mixed_whole(setup, oracle):
    """the mixed streams in one call at level 9, and at level 3: computed once, read by the tests below"""
    S, eng, fs = setup
    streams = mixed_streams(oracle)
    out = {}
    for level in (9, 3):
        fs.reset()
        out[level] = feed(S, eng, fs, streams, [[5] * len(streams)], level, maxlen=MAXLEN)
    return streams, out


@pytest.mark.parametrize("level", [9, 3])
def test_cut_independence(setup, mixed_whole, level):
    S, eng, fs = setup
    streams, whole = mixed_whole
    ns = len(streams)
    ways = {"whole": whole[level]}
    fs.reset()
    ways["one block per call"] = feed(S, eng, fs, streams, [[1] * ns] * 5, level, maxlen=MAXLEN)
    fs.reset()
    ways["mixed"] = feed(S, eng, fs, streams, [[3, 1, 2, 4, 1, 2], [0, 3, 1, 1, 2, 2], [2, 1, 2, 0, 2, 1]], level, maxlen=MAXLEN)
    fs.reset()
    ways["in place"] = feed(S, eng, fs, streams, [[5] * ns], level, maxlen=MAXLEN, glue=followers(streams))
    for name, got in ways.items():
        assert [f for f, _ in got] == [f for f, _ in ways["whole"]], name
        assert [g for _, g in got] == [g for _, g in ways["whole"]], name
    blocks = [b for st in streams for b in st]
    have = payloads([f for f, _ in ways["whole"]], [g for _, g in ways["whole"]], blocks)
    assert have == contiguous_linked(S, eng, streams, level, MAXLEN), "not the linked call over the streams laid out contiguously"


# ---- 3. the level changes inside a stream ------------------------------------------------------------------------------------------
def dstreams_decode(S, eng, ds, per_stream, slots, sizes_per_stream, kind=8, checksum=False):
    """one decompress_dstreams_device call over framed blocks: per stream [(code, bytes)]"""
    import torch
    blocks = [g for st in per_stream for g in st]
    sizes = [n for st in sizes_per_stream for n in st]
    n = len(blocks)
    sf = np.cumsum([0] + [len(st) for st in per_stream]).astype(np.int32)
    framed = b"".join(blocks)
    boff = np.cumsum([0] + [len(g) for g in blocks])[:n].astype(np.int64)
    ooff = np.array([sum(sizes[:i]) + i * APART for i in range(n)] + [0], dtype=np.int64)
    out = torch.full((sum(sizes) + n * APART + 64,), 0x5C, dtype=torch.uint8, device=DEV)
    res = torch.full((max(n, 1),), -12345, dtype=torch.int32, device=DEV)
    eng.set_block_checksum(checksum)
    try:
        eng.decompress_dstreams_device(ds, _t(np.frombuffer(framed + b"\0" * 16, dtype=np.uint8).copy()), len(framed),
                                       _t(np.append(boff, 0)), n, sf, slots, out, _t(ooff), res, header_kind=kind)
        eng.synchronize()
    finally:
        eng.set_block_checksum(False)
    codes, hb = res.cpu().tolist()[:n], out.cpu().numpy()
    flat = [(codes[i], hb[ooff[i]:ooff[i] + max(codes[i], 0)].tobytes()) for i in range(n)]
    return [flat[sf[s]:sf[s + 1]] for s in range(len(per_stream))]


def test_level_changes_inside_a_stream(setup, oracle):
    """levels 0, 9, 9, 3, 0 over the five blocks of two streams: a slot is the stream's last 64 KiB whatever encoder wrote the
    block, so every block meets the pair contract at its own level and the whole is one linked stream"""
    S, eng, fs = setup
    levels = [0, 9, 9, 3, 0]
    streams = [text_stream(oracle, [30000, 65536, 70000, 4096, 20000], 3100), random_stream(21, [4096, 4000, 65536, 65535, 300])]
    fs.reset()
    framed = [[], []]
    for k, level in enumerate(levels):
        per = [[st[k]] for st in streams]
        fl, got, _ = fs_call(S, eng, fs, per, level)
        held = [st[k - 1] if k else b"" for st in streams]
        assert payloads(fl, got, [st[k] for st in streams]) == pair_oracle(S, eng, dict_pairs(per, held), level), (k, level)
        for s in range(2):
            framed[s].append(got[s])
    for s, st in enumerate(streams):
        prev = b""
        for g, b in zip(framed[s], st):
            lz4_check.check_block(g[8:], len(b), dict_len=min(len(prev), 65536))
            assert oracle.decompress_block(g[8:], len(b), prev[-65536:] if prev else None) == (len(b), b), (s, len(b))
            prev = b
    ds = S.DecompressStreams(eng, 2)
    try:
        got = [[], []]
        for lo, hi in ((0, 2), (2, 5)):
            r = dstreams_decode(S, eng, ds, [f[lo:hi] for f in framed], [0, 1], [[len(b) for b in st[lo:hi]] for st in streams])
            for s in range(2):
                got[s] += r[s]
        assert [[b for _, b in g] for g in got] == [[bytes(b) for b in st] for st in streams]
    finally:
        ds.close()


# ---- 4. few workgroups serve many blocks ----------------------------------------------------------------------------------------------
def test_three_workgroups_serve_seventy_streams(setup, oracle):
    """a window is used again by blocks of other streams, staged behind in place and in place behind staged"""
    S, eng, fs = setup
    rs = np.random.RandomState(3)
    text = M.data(oracle, "text", 400000, first=77)
    streams = []
    for s in range(70):
        at = int(rs.randint(0, 300000))
        streams.append([text[at + 700 * k:at + 700 * k + int(rs.randint(1024, 4097))] for k in range(1 + s % 4)])
    flat_followers = sorted(followers(streams))
    glue = set(flat_followers[::3])                                      # some in place, most staged
    fs.reset()
    fl, got, _ = fs_call(S, eng, fs, streams, 9, groups=3, glue=glue)
    blocks = [b for st in streams for b in st]
    assert payloads(fl, got, blocks) == pair_oracle(S, eng, dict_pairs(streams), 9)
    assert [fs.peek(s) for s in range(70)] == [(len(st[-1]), bytes(st[-1])) for st in streams]


def test_one_workgroup_serves_three_hundred_blocks(setup, oracle):
    S, eng, fs = setup
    text = M.data(oracle, "text", 400000, first=901)
    streams = [[text[9000 * s + 500 * k:9000 * s + 500 * k + 2048] for k in range(10)] for s in range(30)]
    glue = {i for i in followers(streams) if i % 2}
    fs.reset()
    fl, got, _ = fs_call(S, eng, fs, streams, 9, groups=1, glue=glue)
    blocks = [b for st in streams for b in st]
    assert len(blocks) == 300
    assert payloads(fl, got, blocks) == pair_oracle(S, eng, dict_pairs(streams), 9)


# ---- 5. every block is a valid LZ4 block; the streams decode however they are cut ----------------------------------------------------
def test_blocks_are_valid_and_streams_decode_however_they_are_cut(setup, oracle, mixed_whole):
    S, eng, fs = setup
    streams, whole = mixed_whole
    ns = len(streams)
    flat = whole[9]                                                      # written in one call
    framed = [[g for _, g in flat[5 * s:5 * s + 5]] for s in range(ns)]
    into_dict = 0
    for s, st in enumerate(streams):                                     # the strict validator, and the CPU oracle's dictionary decode
        prev = b""
        for g, b in zip(framed[s], st):
            into_dict += lz4_check.check_block(g[8:], len(b), dict_len=min(len(prev), 65536))[3]
            assert oracle.decompress_block(g[8:], len(b), prev[-65536:] if prev else None) == (len(b), b), (s, len(b))
            prev = b
    assert into_dict > 100, "hardly a match reaches into a dictionary"
    ds = S.DecompressStreams(eng, ns)
    try:
        got = [[] for _ in streams]
        for lo, hi in ((0, 1), (1, 4), (4, 5)):                          # read 1 + 3 + 1
            r = dstreams_decode(S, eng, ds, [f[lo:hi] for f in framed], list(range(ns)), [[len(b) for b in st[lo:hi]] for st in streams])
            for s in range(ns):
                got[s] += r[s]
        for s, st in enumerate(streams):
            assert [c for c, _ in got[s]] == [len(b) for b in st] and [b for _, b in got[s]] == [bytes(b) for b in st], s
    finally:
        ds.close()


def test_edge_blocks_are_valid(setup, oracle):
    """the contract's streams at level 9 (the oracle's side, which the contract test has pinned the set's bytes to)"""
    S, eng, fs = setup
    streams, dicts = edge_streams(oracle)
    held = [bytes(d[-65536:]) for d in dicts]
    pairs = dict_pairs(streams, held)
    want = pair_oracle(S, eng, pairs, 9, MAXLEN, key="edges")
    for (d, b), w in zip(pairs, want):
        lz4_check.check_block(w, len(b), dict_len=len(d))
        assert oracle.decompress_block(w, len(b), d if d else None) == (len(b), b), (len(d), len(b))


# ---- 6. bad lengths, empty streams, empty blocks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["negative", "above"])
def test_bad_length_stops_its_stream_only(setup, oracle, bad):
    S, eng, fs = setup
    streams = [text_stream(oracle, [3000, 4096, 2000, 4096, 100], 200 + 900 * s) for s in range(3)]
    blocks = [b for st in streams for b in st]
    lens = [len(b) for b in blocks]
    lens[5 + 2] = -1 if bad == "negative" else 4096 + 1
    fs.reset()
    fl, got, rows = fs_call(S, eng, fs, streams, 9, lens=lens, maxlen=4096, groups=2)
    want = pair_oracle(S, eng, dict_pairs(streams), 9, maxlen=4096)
    dead = {7, 8, 9}
    for i in range(15):
        if i in dead:
            assert fl[i] == 0 and (rows[i] == FILL).all(), i
        else:
            assert payloads([fl[i]], [got[i]], [blocks[i]]) == [want[i]], i
    assert fs.peek(1) == (4096, streams[1][1]) and fs.peek(0) == (100, streams[0][4]) and fs.peek(2) == (100, streams[2][4])
    # the next call continues from block 1's tail
    nxt = [[st[0][::-1]] for st in streams]
    fl, got, _ = fs_call(S, eng, fs, nxt, 9, maxlen=4096)
    held = [streams[0][4], streams[1][1], streams[2][4]]
    assert payloads(fl, got, [st[0] for st in nxt]) == pair_oracle(S, eng, dict_pairs(nxt, held), 9, maxlen=4096)


def test_empty_streams_and_empty_blocks(setup, oracle):
    S, eng, fs = setup
    a, b, c = text_stream(oracle, [5000, 5000, 5000], 4000)
    fs.reset()
    fs_call(S, eng, fs, [[a], [a]], 9, slots=[0, 1])
    assert fs.peek(0) == fs.peek(1) == (5000, a)
    # stream 0 is empty in this call: its slot is untouched; stream 1 brings an empty block and one behind it
    fl, got, _ = fs_call(S, eng, fs, [[], [b"", c]], 9, slots=[0, 1])
    assert fs.peek(0) == (5000, a)
    assert got[0][8:] == b"\0" and payloads(fl[1:], got[1:], [c]) == pair_oracle(S, eng, [(b"", c)], 9)
    assert fs.peek(1) == (5000, c)
    fl, got, _ = fs_call(S, eng, fs, [[b""]], 9, slots=[1])       # an empty block last: the count is 0
    assert fs.peek(1) == (0, b"")
    fl, got, _ = fs_call(S, eng, fs, [[b]], 9, slots=[1])
    assert payloads(fl, got, [b]) == pair_oracle(S, eng, [(b"", b)], 9)


# ---- 7. block checksums -----------------------------------------------------------------------------------------------------------
def test_block_checksums(setup, oracle):
    S, eng, fs = setup
    streams = [text_stream(oracle, [4096, 0, 13, 30000], 600), random_stream(12, [12, 4096, 4096, 75])]
    blocks = [b for st in streams for b in st]
    fs.reset()
    fl, got, _ = fs_call(S, eng, fs, streams, 9, checksum=True)
    have = payloads(fl, got, blocks, trailer=4)
    assert have == pair_oracle(S, eng, dict_pairs(streams), 9)
    for g, h in zip(got, have):
        assert int.from_bytes(g[-4:], "little") == M.xxh32(h)
    ds = S.DecompressStreams(eng, 2)
    try:
        r = dstreams_decode(S, eng, ds, [got[:4], got[4:]], [0, 1], [[len(b) for b in st] for st in streams], checksum=True)
        assert [[b for _, b in st] for st in r] == [[bytes(b) for b in st] for st in streams]
    finally:
        ds.close()


# ---- 8. the level is the set's, the engine's stays 0 --------------------------------------------------------------------------------
def test_the_attribute_and_the_engine_s_level(setup):
    import ctypes as C
    import torch
    S, eng, fs = setup
    L = S.lib
    assert fs.level == 0
    for bad in (13, -1):
        fs.set_level(9)
        with pytest.raises(S.LZ4Error):
            fs.set_level(bad)
        assert L.mi355lz4_fstreams_set_level(fs._h, bad) == E_ARG and b"0..12" in L.mi355lz4_last_error()
        assert fs.level == 9
    assert L.mi355lz4_fstreams_set_level(None, 3) == E_ARG and L.mi355lz4_fstreams_get_level(None) == E_ARG
    # any engine level other than 0 is refused with the level-0 message, whatever the set's level is
    _i32p = C.POINTER(C.c_int32)
    src = torch.zeros(256, dtype=torch.uint8, device=DEV)
    slots = torch.full((2 * 64,), FILL, dtype=torch.uint8, device=DEV)
    flen = torch.full((2,), -77, dtype=torch.int32, device=DEV)
    off = torch.zeros(3, dtype=torch.int64, device=DEV)
    ln = torch.zeros(3, dtype=torch.int32, device=DEV)
    sf, sl = np.array([0, 1, 2], dtype=np.int32), np.array([0, 1, 0], dtype=np.int32)
    fs.reset()

    def call():
        return L.mi355lz4_compress_streams_fast_device(eng.ctx, fs._h, src.data_ptr(), off.data_ptr(), ln.data_ptr(), 0, 16, 2,
                                                       sf.ctypes.data_as(_i32p), sl.ctypes.data_as(_i32p), 2, 1, 8, slots.data_ptr(), 64,
                                                       flen.data_ptr())
    try:
        for set_level in (0, 9):
            fs.set_level(set_level)
            for level in (1, 9, 12):
                eng.set_compression_level(level)
                assert call() == E_ARG and b"fast streams are level 0's encoder" in L.mi355lz4_last_error()
        eng.set_compression_level(0)
        fs.set_level(9)
        assert call() == 0
        eng.synchronize()
        assert flen.cpu().tolist() == [9, 9]                             # two empty blocks
    finally:
        eng.set_compression_level(0)
        fs.set_level(0)


# ---- 9. the host form ------------------------------------------------------------------------------------------------------------
def host_form_child():
    """(a process of its own: the pipeline reads MI355LZ4_GROUP_MB once)"""
    import streamly_lz4_amd as S
    from oracle.oracle import Oracle
    assert os.environ.get("MI355LZ4_GROUP_MB") == "1"                     # group seams fall inside the streams
    oracle = Oracle()
    eng = S.Engine(0)
    fs = S.FastCompressStreams(eng, 4)
    streams = [text_stream(oracle, [65536] * 10 + [300], 100 + 2000 * s) for s in range(4)]
    blocks = [b for st in streams for b in st]
    assert sum(len(b) for b in blocks) > 5 << 19                               # three groups and more
    fl, got, _ = fs_call(S, eng, fs, streams, 9)
    assert fl == [len(g) for g in got] and payloads(fl, got, blocks) == pair_oracle(S, eng, dict_pairs(streams), 9)
    fl0, got0, _ = fs_call(S, eng, fs, streams, 0)
    assert got0 != got
    fs.reset()
    eng.set_compression_level(0)
    fs.set_level(9)
    framed, bfl, status = eng.compress_streams_fast(streams, fs)
    assert fs.level == 9
    assert bfl == fl and framed == b"".join(got), "the host form's bytes are not the device call's"
    assert status == [f - 8 for f in fl]
    assert [fs.peek(s) for s in range(4)] == [(300, st[-1]) for st in streams]
    fs.close()
    eng.close()
    print("hstreams host form ok")


def test_host_form_across_group_seams():
    """compress_streams_fast at set level 9 with groups of 1 MiB: the framed bytes are the device call's, status and
    blockFramedLen agree"""
    import subprocess
    env = dict(os.environ, MI355LZ4_GROUP_MB="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "host_form"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "hstreams host form ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


# ---- 10. size ---------------------------------------------------------------------------------------------------------------------
def test_level_nine_is_smaller(setup, oracle, record):
    """a linked text stream of 16 blocks of 64 KiB: strictly smaller at set level 9 than at set level 0, and not larger than at
    level 1 (a condition, not a tolerance: batches measured 0.865 of level 0's bytes at level 9 for text)"""
    S, eng, fs = setup
    raw = oracle.gen("text", 16, 65536).tobytes()
    stream = [raw[i * 65536:(i + 1) * 65536] for i in range(16)]
    total = {}
    for level in (0, 1, 9):
        fs.reset()
        fl, _, _ = fs_call(S, eng, fs, [stream], level)
        assert all(f > 8 for f in fl)
        total[level] = sum(fl)
    rec = {"bytes": 16 * 65536, "framed": total, "level9_vs_level0": total[9] / total[0], "level1_vs_level0": total[1] / total[0]}
    print(rec)
    record("hstreams_size", rec)
    assert total[9] < total[0] and total[9] <= total[1], total


if __name__ == "__main__":
    assert sys.argv[1:] == ["host_form"]
    host_form_child()
