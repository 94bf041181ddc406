"""Fast linked streams continued across calls: mi355lz4_fstreams, mi355lz4_compress_streams_fast_device / _compress_streams_fast
(DESIGN.md 7p).

The contract needs no CPU codec.  Block k of a stream has D as its dictionary: the last min(len, 65536) bytes of the block before
it in its stream -- what the slot holds, for a stream's first block of a call -- and none when that block was empty or the slot is
reset.  Its bytes are what mi355lz4_compress_batch_device with the linked switch on writes for the SECOND block of the contiguous
two-block call [D, B_k] at level 0 with the same accel and max(|D|, maxBlockLen) as its maxBlockLen; with an empty D the block of
the one-block linked call.  One linked call over all the pairs, laid into one buffer with gaps between the pairs, gives every
oracle block (as linked_oracle does in tests/test_fastdict_gpu.py).

The blocks of a call lie 7 bytes apart, so every alignment occurs; the arrays are in stream order and the bytes are laid down in a
permuted order."""
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
KNOB = "MI355LZ4_FSTREAMS_WAVES"
NSLOTS = 80


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


def fs_call(S, eng, fs, streams, slots=None, accel=1, kind=8, checksum=False, lens=None, maxlen=None, glue=(), waves=None):
    """one compress_streams_fast_device call: streams[s] = the blocks stream s brings, continuing slot slots[s] (default s).
    Returns (framedLen[], [slot bytes up to framedLen], all slots as rows)"""
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
    if waves is not None:
        os.environ[KNOB] = str(waves)
    try:
        src = _t(buf)
        eng.compress_streams_fast_device(fs, src, n, mx, sf, slots_of, out, stride, flen, accel=accel, header_kind=kind,
                                         src_off=_t(np.array(off + [0], dtype=np.int64)),
                                         src_len=_t(np.array(([len(b) for b in blocks] if lens is None else list(lens)) + [0],
                                                             dtype=np.int32)), block_stride=0)
        eng.synchronize()
        src.fill_(0x3C)                           # the call has run: the slot owns its copy
        eng.synchronize()
    finally:
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


_oracle_cache = {}


def pair_oracle(S, eng, pairs, accel=1, maxlen=None, key=None):
    """The contract's right-hand side: all pairs [D, B] in one buffer with gaps between the pairs, ONE linked
    compress_batch_device call at level 0 with max(|D|, maxlen) as its maxBlockLen; the payload of every pair's second block
    (an empty D: the one-block pair [B])."""
    import torch
    if key is not None and (key, accel) in _oracle_cache:
        return _oracle_cache[(key, accel)]
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
    lens = [len(x) for x in parts]
    data = np.full(pos + 64, FILL, dtype=np.uint8)
    for o, x in zip(offs, parts):
        data[o:o + len(x)] = np.frombuffer(x, dtype=np.uint8)
    n, big = len(offs), max([len(d) for d, _ in pairs] + [mx])
    stride = S.slot_stride_ex(big, 8, False)
    slots = torch.full((n * stride,), FILL, dtype=torch.uint8, device=DEV)
    flen = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    eng.set_compression_level(0)
    eng.set_linked_compress(True)
    try:
        eng.compress_batch_device(_t(data), n, big, slots, stride, flen, accel=accel, header_kind=8,
                                  src_off=_t(np.array(offs, dtype=np.int64)), src_len=_t(np.array(lens, dtype=np.int32)), block_stride=0)
        eng.synchronize()
    finally:
        eng.set_linked_compress(False)
    fl, hb = flen.cpu().tolist(), slots.cpu().numpy()
    out = [hb[i * stride + 8:i * stride + fl[i]].tobytes() for i in second]
    if key is not None:
        _oracle_cache[(key, accel)] = out
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


def contiguous_linked(S, eng, streams, accel=1, maxlen=None):
    """every stream laid out contiguously, one byte between the streams, ONE linked compress_batch_device call: payload per block"""
    import torch
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
    n = len(blocks)
    stride = S.slot_stride_ex(mx, 8, False)
    slots = torch.full((n * stride,), FILL, dtype=torch.uint8, device=DEV)
    flen = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    eng.set_compression_level(0)
    eng.set_linked_compress(True)
    try:
        eng.compress_batch_device(_t(data), n, mx, slots, stride, flen, accel=accel, header_kind=8,
                                  src_off=_t(np.array(offs, dtype=np.int64)), src_len=_t(np.array([len(b) for b in blocks], dtype=np.int32)),
                                  block_stride=0)
        eng.synchronize()
    finally:
        eng.set_linked_compress(False)
    fl, hb = flen.cpu().tolist(), slots.cpu().numpy()
    return [hb[i * stride + 8:i * stride + fl[i]].tobytes() for i in range(n)]


# ---- the streams ---------------------------------------------------------------------------------------------------------------
def text_stream(oracle, lens, first):
    """blocks that overlap each other in a text: a block's predecessor holds most of what it holds"""
    text = M.data(oracle, "text", 400000, first=first)
    return [text[1000 * k + 37 * (k % 3):1000 * k + 37 * (k % 3) + n] for k, n in enumerate(lens)]


def random_stream(seed, lens):
    """slices of one random buffer: only the link makes them compressible"""
    r = rnd(seed, max(lens) + 400)
    return [r[(53 * k) % 300:(53 * k) % 300 + n] for k, n in enumerate(lens)]


def small_streams(oracle):
    """5 blocks each, every length of {0, 1, 12, 13, 75, 4096, 65535, 65536} with a successor and a predecessor somewhere"""
    return [text_stream(oracle, [4096, 65536, 65535, 75, 13], 11),
            text_stream(oracle, [75, 0, 4096, 12, 4096], 5003),
            random_stream(7, [65536, 65535, 4096, 75, 13]),
            text_stream(oracle, [1, 13, 65536, 0, 65536], 977),
            random_stream(8, [12, 4096, 1, 65536, 65536])]


def big_streams(oracle):
    """maxBlockLen 100000: the non-PAIR instantiation, and a dictionary tail cut from a longer block"""
    return [text_stream(oracle, [100000, 65537, 4096, 100000, 13], 31),
            random_stream(9, [65537, 100000, 75, 65536, 0]),
            text_stream(oracle, [13, 100000, 100000, 0, 65537], 7001)]


SETS = {"small": (small_streams, None), "big": (big_streams, 100000)}


# ---- 1. the contract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("accel", [1, 7])
@pytest.mark.parametrize("which", ["small", "big"])
def test_contract_every_block_is_the_linked_pair_s_second_block(setup, oracle, which, accel, kind):
    S, eng, fs = setup
    make, maxlen = SETS[which]
    streams = make(oracle)
    blocks = [b for st in streams for b in st]
    fs.reset()
    fl, got, _ = fs_call(S, eng, fs, streams, accel=accel, kind=kind, maxlen=maxlen)
    want = pair_oracle(S, eng, dict_pairs(streams), accel, maxlen, key=which)
    have = payloads(fl, got, blocks, kind)
    for i, (h, w) in enumerate(zip(have, want)):
        assert h == w, (which, accel, kind, "block %d of %d bytes" % (i, len(blocks[i])), len(h), len(w))
    # the link was really used: some block is smaller than it is without its dictionary
    alone = pair_oracle(S, eng, [(b"", b) for b in blocks], accel, maxlen, key=which + " alone")
    assert sum(len(h) < len(a) for h, a in zip(have, alone)) >= 4


# ---- 2. cut independence -----------------------------------------------------------------------------------------------------------
def feed(S, eng, fs, streams, partition, **kw):
    """the streams cut into calls: partition[c][s] = blocks of stream s in call c; per flat block (framedLen, slot bytes)"""
    done = [0] * len(streams)
    out = [[] for _ in streams]
    for counts in partition:
        per = [st[d:d + k] for st, d, k in zip(streams, done, counts)]
        fl, got, _ = fs_call(S, eng, fs, per, **kw)
        sf = np.cumsum([0] + list(counts))
        for s, k in enumerate(counts):
            out[s] += list(zip(fl[sf[s]:sf[s + 1]], got[sf[s]:sf[s + 1]]))
            done[s] += k
    assert done == [len(st) for st in streams]
    return [x for st in out for x in st]


def test_cut_independence(setup, oracle):
    S, eng, fs = setup
    streams = small_streams(oracle)
    ns = len(streams)
    ways = {}
    fs.reset()
    ways["whole"] = feed(S, eng, fs, streams, [[5] * ns])
    fs.reset()
    ways["one block per call"] = feed(S, eng, fs, streams, [[1] * ns] * 5)
    fs.reset()
    ways["cut after block 2"] = feed(S, eng, fs, streams, [[3] * ns, [2] * ns])
    fs.reset()
    # blocks 1|2 of stream 0 (65536 -> 65535), 3|4 of stream 2, 2|3 of stream 1 (4096 -> 12) directly behind their predecessors
    ways["in place"] = feed(S, eng, fs, streams, [[5] * ns], glue={2, 14, 8})
    for name, got in ways.items():
        assert [f for f, _ in got] == [f for f, _ in ways["whole"]], name
        assert [g for _, g in got] == [g for _, g in ways["whole"]], name
    blocks = [b for st in streams for b in st]
    have = payloads([f for f, _ in ways["whole"]], [g for _, g in ways["whole"]], blocks)
    assert have == contiguous_linked(S, eng, streams), "not the linked call over the streams laid out contiguously"


# ---- 3. the link crosses the call ---------------------------------------------------------------------------------------------------
def test_the_link_crosses_the_call(setup):
    """A random block is sent, then the same bytes again in the next call: one long match (about 270 bytes), where the block
    without its dictionary is above 65536.  The block is 65535 bytes, not 65536: a byte's copy in the block before then lies
    65535 bytes back, the largest offset an LZ4 block can hold -- the same 65536 bytes again have no match at all."""
    S, eng, fs = setup
    r = rnd(41, 65535)
    fs.reset()
    fl, _, _ = fs_call(S, eng, fs, [[r]], slots=[9])
    assert fl[0] > 65536
    fl, _, _ = fs_call(S, eng, fs, [[r]], slots=[9])
    assert 8 < fl[0] < 1024, fl
    fs.reset([9])
    fl, _, _ = fs_call(S, eng, fs, [[r]], slots=[9])
    assert fl[0] > 65536, fl


# ---- 4. _set_dict ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dl", [0, 7, 4096, 65536, 70000])
def test_set_dict(setup, oracle, dl):
    S, eng, fs = setup
    text = M.data(oracle, "text", 200000, first=123)
    D, B = text[:dl], text[max(dl - 3000, 0):max(dl - 3000, 0) + 20000]
    fs.reset()
    d = _t(np.frombuffer(D + b"\0", dtype=np.uint8).copy())
    fs.set_dict(3, d, dl)
    eng.synchronize()
    d.fill_(0x11)                                  # the slot keeps its own copy
    assert fs.peek(3) == (min(dl, 65536), D[-65536:] if dl else b"")
    fl, got, _ = fs_call(S, eng, fs, [[B]], slots=[3])
    assert payloads(fl, got, [B]) == pair_oracle(S, eng, [(D[-65536:] if dl else b"", B)])
    assert fs.peek(3) == (len(B), B) and fs.peek(2) == (0, b"")


# ---- 5. waves that serve many streams ------------------------------------------------------------------------------------------------
def test_three_waves_serve_seventy_streams(setup, oracle):
    S, eng, fs = setup
    rs = np.random.RandomState(3)
    text = M.data(oracle, "text", 400000, first=77)
    streams = []
    for s in range(70):
        at = int(rs.randint(0, 300000))
        streams.append([text[at + 700 * k:at + 700 * k + int(rs.randint(1024, 4097))] for k in range(3)])
    glue = {3 * s + 1 for s in range(0, 70, 3)} | {3 * s + 2 for s in range(0, 70, 5)}     # some in place, most staged
    fs.reset()
    fl, got, _ = fs_call(S, eng, fs, streams, waves=-3, glue=glue)
    for s, st in enumerate(streams):
        fs.reset([s])
        f1, g1, _ = fs_call(S, eng, fs, [st], slots=[s])
        assert (fl[3 * s:3 * s + 3], got[3 * s:3 * s + 3]) == (f1, g1), s


# ---- 6. bad lengths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["negative", "above"])
def test_bad_length_stops_its_stream_only(setup, oracle, bad):
    S, eng, fs = setup
    streams = [text_stream(oracle, [3000, 4096, 2000, 4096, 100], 200 + 900 * s) for s in range(3)]
    blocks = [b for st in streams for b in st]
    lens = [len(b) for b in blocks]
    lens[5 + 2] = -1 if bad == "negative" else 4096 + 1
    fs.reset()
    fl, got, rows = fs_call(S, eng, fs, streams, lens=lens, maxlen=4096)
    want = pair_oracle(S, eng, dict_pairs(streams), maxlen=4096)
    dead = {7, 8, 9}
    for i in range(15):
        if i in dead:
            assert fl[i] == 0 and (rows[i] == FILL).all(), i
        else:
            assert payloads([fl[i]], [got[i]], [blocks[i]]) == [want[i]], i
    assert fs.peek(1) == (4096, streams[1][1]) and fs.peek(0) == (100, streams[0][4])
    # the next call continues from block 1's tail
    nxt = [[st[0][::-1]] for st in streams]
    fl, got, _ = fs_call(S, eng, fs, nxt, maxlen=4096)
    held = [streams[0][4], streams[1][1], streams[2][4]]
    assert payloads(fl, got, [st[0] for st in nxt]) == pair_oracle(S, eng, dict_pairs(nxt, held), maxlen=4096)


# ---- 7. resets and empties --------------------------------------------------------------------------------------------------------
def test_empty_streams_and_empty_blocks(setup, oracle):
    S, eng, fs = setup
    a, b, c = text_stream(oracle, [5000, 5000, 5000], 4000)
    fs.reset()
    fs_call(S, eng, fs, [[a], [a]], slots=[0, 1])
    assert fs.peek(0) == fs.peek(1) == (5000, a)
    # stream 0 is empty in this call: its slot is untouched; stream 1 brings an empty block and one behind it
    fl, got, _ = fs_call(S, eng, fs, [[], [b"", c]], slots=[0, 1])
    assert fs.peek(0) == (5000, a)
    assert got[0][8:] == b"\0" and payloads(fl[1:], got[1:], [c]) == pair_oracle(S, eng, [(b"", c)])
    assert fs.peek(1) == (5000, c)
    fl, got, _ = fs_call(S, eng, fs, [[b""]], slots=[1])          # an empty block last: the count is 0
    assert fs.peek(1) == (0, b"")
    fl, got, _ = fs_call(S, eng, fs, [[b]], slots=[1])
    assert payloads(fl, got, [b]) == pair_oracle(S, eng, [(b"", b)])


# ---- 8. decoding ---------------------------------------------------------------------------------------------------------------
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


def test_streams_decode_however_they_are_cut(setup, oracle):
    S, eng, fs = setup
    streams = small_streams(oracle)
    ns = len(streams)
    fs.reset()
    flat = feed(S, eng, fs, streams, [[2] * ns, [3] * ns])                # written 2 + 3
    framed = [[g for _, g in flat[5 * s:5 * s + 5]] for s in range(ns)]
    for s, st in enumerate(streams):                                     # the CPU oracle's linked decode, and the strict validator
        prev = b""
        for g, b in zip(framed[s], st):
            lz4_check.check_block(g[8:], len(b), dict_len=min(len(prev), 65536))
            assert oracle.decompress_block(g[8:], len(b), prev[-65536:] if prev else None) == (len(b), b), (s, len(b))
            prev = b
    ds = S.DecompressStreams(eng, ns)
    try:
        got = [[] for _ in streams]
        for lo, hi in ((0, 1), (1, 4), (4, 5)):                          # read 1 + 3 + 1
            r = dstreams_decode(S, eng, ds, [f[lo:hi] for f in framed], list(range(ns)), [[len(b) for b in st[lo:hi]] for st in streams])
            for s in range(ns):
                got[s] += r[s]
        for s, st in enumerate(streams):
            # (an empty block decodes to 0 bytes)
            assert [c for c, _ in got[s]] == [len(b) for b in st] and [b for _, b in got[s]] == [bytes(b) for b in st], s
    finally:
        ds.close()


# ---- 9. block checksums ----------------------------------------------------------------------------------------------------------
def test_block_checksums(setup, oracle):
    S, eng, fs = setup
    streams = [text_stream(oracle, [4096, 0, 13, 30000], 600), random_stream(12, [12, 4096, 4096, 75])]
    blocks = [b for st in streams for b in st]
    fs.reset()
    fl, got, _ = fs_call(S, eng, fs, streams, checksum=True)
    have = payloads(fl, got, blocks, trailer=4)
    assert have == pair_oracle(S, eng, dict_pairs(streams))
    for g, h in zip(got, have):
        assert int.from_bytes(g[-4:], "little") == M.xxh32(h)
    ds = S.DecompressStreams(eng, 2)
    try:
        framed = [got[:4], got[4:]]
        r = dstreams_decode(S, eng, ds, framed, [0, 1], [[len(b) for b in st] for st in streams], checksum=True)
        assert [[b for _, b in st] for st in r] == [[bytes(b) for b in st] for st in streams]
        broken = bytearray(got[1 + 4])
        broken[-1] ^= 1
        ds.reset()
        r = dstreams_decode(S, eng, ds, [[got[4], bytes(broken)]], [0], [[12, 4096]], checksum=True)
        assert r[0][0][0] == 12 and r[0][1][0] == M.BLK_E_CHECKSUM
    finally:
        ds.close()


# ---- 10. the host form ------------------------------------------------------------------------------------------------------------
def host_form_child():
    """(a process of its own: the pipeline reads MI355LZ4_GROUP_MB once)"""
    import ctypes as C
    import streamly_lz4_amd as S
    from oracle.oracle import Oracle
    assert os.environ.get("MI355LZ4_GROUP_MB") == "1"                     # group seams fall inside the streams
    oracle = Oracle()
    eng = S.Engine(0)
    fs = S.FastCompressStreams(eng, 4)
    streams = [text_stream(oracle, [65536] * 20 + [300], 100 + 2000 * s) for s in range(4)]
    blocks = [b for st in streams for b in st]
    assert sum(len(b) for b in blocks) > 5 << 20                               # five groups and more
    fl, got, _ = fs_call(S, eng, fs, streams)
    assert fl == [len(g) for g in got] and payloads(fl, got, blocks) == pair_oracle(S, eng, dict_pairs(streams))
    fs.reset()
    eng.set_compression_level(0)
    framed, bfl, status = eng.compress_streams_fast(streams, fs)
    assert bfl == fl and framed == b"".join(got), "the host form's bytes are not the device call's"
    assert status == [f - 8 for f in fl]
    before = [fs.peek(s) for s in range(4)]
    assert before == [(300, st[-1]) for st in streams]
    _u8p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    arrs = [np.frombuffer(b, dtype=np.uint8) for b in blocks[:2]]
    ptrs = (_u8p * 2)(*[a.ctypes.data_as(_u8p) for a in arrs])
    out = np.empty(1 << 18, dtype=np.uint8)
    sf, sl = np.array([0, 2], dtype=np.int32), np.array([0], dtype=np.int32)
    for bad in (-1, (4 << 20) + 1):
        lens = np.array([65536, bad], dtype=np.int32)
        out_len = C.c_size_t(5)
        rc = S.lib.mi355lz4_compress_streams_fast(eng.ctx, fs._h, ptrs, lens.ctypes.data_as(_i32p), 2, sf.ctypes.data_as(_i32p),
                                                  sl.ctypes.data_as(_i32p), 1, 1, 8, out.ctypes.data_as(_u8p), out.size,
                                                  C.byref(out_len), None, None)
        assert rc == E_ARG and out_len.value == 0, (bad, rc)
    assert [fs.peek(s) for s in range(4)] == before
    fs.close()
    eng.close()
    print("fstreams host form ok")


def test_host_form_across_group_seams():
    """compress_streams_fast with groups of 1 MiB: the framed bytes are the device call's, status and blockFramedLen agree; a bad
    length is E_ARG and the slots stay"""
    import subprocess
    env = dict(os.environ, MI355LZ4_GROUP_MB="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "host_form"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fstreams host form ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


# ---- 11. every argument check, with a real set ------------------------------------------------------------------------------------
def test_argument_checks(setup):
    import ctypes as C
    import torch
    S, eng, fs = setup
    L = S.lib
    _i32p = C.POINTER(C.c_int32)
    src = torch.zeros(256, dtype=torch.uint8, device=DEV)
    slots = torch.full((2 * 64,), FILL, dtype=torch.uint8, device=DEV)
    flen = torch.full((2,), -77, dtype=torch.int32, device=DEV)
    off = torch.zeros(3, dtype=torch.int64, device=DEV)
    ln = torch.zeros(3, dtype=torch.int32, device=DEV)
    fs.reset()
    eng.synchronize()

    def call(sf=(0, 1, 2), sl=(0, 1), n=2, ns=None, mx=16, kind=8, stride=64, src_=src, slots_=slots, flen_=flen):
        a = np.array(sf, dtype=np.int32)
        b = np.array(list(sl) + [0], dtype=np.int32)
        return L.mi355lz4_compress_streams_fast_device(eng.ctx, fs._h, src_.data_ptr() if src_ is not None else None, off.data_ptr(),
                                                       ln.data_ptr(), 0, mx, n, a.ctypes.data_as(_i32p), b.ctypes.data_as(_i32p),
                                                       len(sl) if ns is None else ns, 1, kind,
                                                       slots_.data_ptr() if slots_ is not None else None, stride,
                                                       flen_.data_ptr() if flen_ is not None else None)
    eng.set_compression_level(0)
    assert call() == 0
    assert call(sf=(0, 3, 2)) == E_ARG and b"not ascending" in L.mi355lz4_last_error()
    assert call(sf=(0, 1, 1)) == E_ARG and b"do not cover" in L.mi355lz4_last_error()
    assert call(sf=(1, 1, 2)) == E_ARG
    assert call(n=-1) == E_ARG and call(ns=-1) == E_ARG
    for bad in (-1, NSLOTS, 2 ** 31 - 1):
        assert call(sl=(0, bad)) == E_ARG and b"names slot" in L.mi355lz4_last_error()
    assert call(sl=(5, 5)) == E_ARG and b"named twice" in L.mi355lz4_last_error()
    assert call(kind=5) == E_ARG and call(mx=-1) == E_ARG
    assert call(mx=(4 << 20) + 1, stride=8 << 20) == E_ARG and b"maxBlockLen" in L.mi355lz4_last_error()
    assert call(src_=None) == E_ARG and call(slots_=None) == E_ARG and call(flen_=None) == E_ARG
    assert call(stride=16 + 16 + 8 - 1) == -4                             # MI355LZ4_E_CAPACITY
    for level in (1, 9, 12):
        eng.set_compression_level(level)
        assert call() == E_ARG and b"level 0's encoder" in L.mi355lz4_last_error()
    eng.set_compression_level(0)
    # the switches that are ignored: linked, segments, exact
    eng.set_linked_compress(True)
    eng.set_segments(2)
    eng.set_compress_exact(True)
    try:
        assert call() == 0
    finally:
        eng.set_linked_compress(False)
        eng.set_segments(-1)
        eng.set_compress_exact(False)
    assert call(sf=(0,), sl=(), n=0) == 0 and call(sf=(0, 0, 0), n=0) == 0   # nothing to do
    # the set's own calls
    assert L.mi355lz4_fstreams_count(fs._h) == NSLOTS == len(fs)
    bad = np.array([0, NSLOTS], dtype=np.int32)
    assert L.mi355lz4_fstreams_reset(eng.ctx, fs._h, bad.ctypes.data_as(_i32p), 2) == E_ARG
    assert L.mi355lz4_fstreams_reset(eng.ctx, fs._h, bad.ctypes.data_as(_i32p), -1) == E_ARG
    for slot in (-1, NSLOTS):
        assert L.mi355lz4_fstreams_set_dict(eng.ctx, fs._h, slot, src.data_ptr(), 8) == E_ARG
    assert L.mi355lz4_fstreams_set_dict(eng.ctx, fs._h, 0, src.data_ptr(), -1) == E_ARG
    assert L.mi355lz4_fstreams_set_dict(eng.ctx, fs._h, 0, None, 8) == E_ARG
    cnt = C.c_int(7)
    assert L.mi355lz4_debug_fstreams_peek(fs._h, NSLOTS, None, C.byref(cnt)) == E_ARG and cnt.value == 7
    eng.synchronize()
    assert flen.cpu().tolist() == [9, 9] and fs.peek(0) == (0, b"")        # two empty blocks were written, nothing else


if __name__ == "__main__":
    assert sys.argv[1:] == ["host_form"]
    host_form_child()
