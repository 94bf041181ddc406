"""mi355lz4_decompress_partial_device / mi355lz4_decompress_partial on the GPU: the first target[i] bytes of every block, as
LZ4_decompress_safe_partial gives them.

Well-formed blocks need no oracle (result = min(target, cap, n), bytes = the prefix; tests/test_partial_decode_host.py holds
that law to the reference for the targets used here); mutated blocks are checked against the reference's recorded results
(tests/golden/partial_vectors.json).  Every case runs under every decoder variant and 0, and the variants must agree byte
for byte.  No byte outside [outOff[i], outOff[i] + min(target, cap)) may change, whatever the block's result."""
import random
import statistics

import numpy as np
import pytest

import guarded as G
import lz4_synth as Z
import partial_cases as P
from conftest import DECODERS

import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E_ARG, E_BLOCK, E_CAPACITY = -3, -5, -4
BLK_E_COMPLEN, BLK_E_TRUNCATED, BLK_E_UNCOMPLEN, BLK_E_CHECKSUM = -0x7F000001, -0x7F000002, -0x7F000003, -0x7F000004
VARIANTS = DECODERS + [0]
SEED = 41


def _t(a, dtype=None):
    a = np.frombuffer(bytes(a), dtype=np.uint8).copy() if isinstance(a, (bytes, bytearray)) else np.asarray(a, dtype=dtype)
    return torch.from_numpy(a).to(DEV)


def frame(blocks, hk, uncomp=None, trailer=None):
    """dense framing: | compLen | uncompLen (kind 8) | data | xxh32 (trailer) |; returns (bytes, offsets)"""
    buf, offs = bytearray(), []
    for i, b in enumerate(blocks):
        offs.append(len(buf))
        buf += len(b).to_bytes(4, "little")
        if hk == 8:
            buf += int(uncomp[i]).to_bytes(4, "little", signed=True)
        buf += bytes(b)
        if trailer:
            buf += int(trailer(bytes(b))).to_bytes(4, "little")
    return bytes(buf), offs


class Call:
    """One partial call over guarded memory.  entries: [(block index, target, cap)]; the blocks are framed once (kind 4, the
    capacity comes through outCap) and an entry names one of them, so many targets go over the same compressed bytes.
    starts: where each entry's output begins (None: packed back to back at scan(min(target, cap)))."""

    def __init__(self, blocks, entries, starts=None):
        self.blob, offs = frame(blocks, 4)
        self.entries = entries
        self.n = len(entries)
        self.boff = np.array([offs[b] for b, _, _ in entries], dtype=np.int64)
        self.tgt = np.array([t for _, t, _ in entries], dtype=np.int32)
        self.cap = np.array([c for _, _, c in entries], dtype=np.int32)
        self.room = np.where(self.tgt < 0, 0, np.minimum(self.tgt, self.cap)).astype(np.int64)
        if starts is None:
            self.starts = G.END_GUARD + np.concatenate([[0], np.cumsum(self.room)[:-1]]) if self.n else np.zeros(0, dtype=np.int64)
            self.total = int(G.END_GUARD * 2 + self.room.sum())
        else:
            self.starts, self.total = np.asarray(starts.starts, dtype=np.int64), starts.total
        self.d = {"blob": _t(self.blob), "boff": _t(self.boff), "tgt": _t(self.tgt), "cap": _t(self.cap), "ooff": _t(self.starts)}
        self.keep = {k: v.clone() for k, v in self.d.items()}

    def run(self, engine, decoder):
        """(result[], the output buffer on the device); asserts the confinement of out, result[] and the inputs"""
        out = G.new_torch(self.total, SEED, DEV)
        res = G.GuardedArray(self.n, torch.int32, SEED + 1, DEV)
        engine.set_decoder(decoder)
        try:
            engine.decompress_partial_device(self.d["blob"], len(self.blob), self.d["boff"], self.n, out, self.d["ooff"], self.d["tgt"],
                                             res.view, header_kind=4, fixed_uncomp=0, out_cap=self.d["cap"])
            engine.synchronize()
        finally:
            engine.set_decoder(0)
        G.assert_confined(out, [(s, s + r) for s, r in zip(self.starts.tolist(), self.room.tolist())], SEED, "out, decoder %d" % decoder)
        res.check(what="result[], decoder %d" % decoder)
        for k in self.d:
            assert torch.equal(self.d[k], self.keep[k]), "the call wrote its input %s" % k
        return res.view.cpu().numpy().copy(), out

    def check(self, result, out, want_res, want_bytes, what):
        bad = np.nonzero(result != np.asarray(want_res))[0]
        assert bad.size == 0, "%s: entry %d (block %d, target %d, cap %d): result %d, expected %d" % (
            (what, bad[0]) + tuple(self.entries[bad[0]]) + (result[bad[0]], want_res[bad[0]]))
        host = out.cpu().numpy()
        for i, (s, w) in enumerate(zip(self.starts.tolist(), want_bytes)):
            if w is not None and host[s:s + len(w)].tobytes() != w:
                got, w = host[s:s + len(w)].tobytes(), bytes(w)
                at = next(k for k in range(len(w)) if got[k] != w[k])
                raise AssertionError("%s: entry %d (block %d, target %d, cap %d): byte %d of %d differs" % (
                    (what, i) + tuple(self.entries[i]) + (at, len(w))))


def run_all_variants(engine, call, want_res, want_bytes, what):
    first = None
    for d in VARIANTS:
        res, out = call.run(engine, d)
        if want_res is not None:
            call.check(res, out, want_res, want_bytes, "%s, decoder %d" % (what, d))
        if first is None:
            first = (res, out)
        else:
            assert np.array_equal(res, first[0]), "%s: decoder %d and %d disagree on result[]" % (what, VARIANTS[0], d)
            assert torch.equal(out, first[1]), "%s: decoder %d and %d disagree on the bytes" % (what, VARIANTS[0], d)
    return first


def split4(framed, flen):
    out, pos = [], 0
    for f in flen:
        out.append(framed[pos + 4:pos + f])
        pos += f
    return out


BIG = 8192       # blocks above this get a sample of their sequence boundaries (partial_cases.sampled_boundaries), not all


def well_formed_entries(blocks, rng):
    """entries and expectations for [(name, block, data)]: every target of partial_cases.targets_for -- with every sequence
    boundary of a block of up to 8 KiB, and the sample partial_cases.sampled_boundaries describes of a bigger one -- the
    capacity below, at and above the target in turn.  The expected bytes are views of the data, not copies."""
    entries, want_res, want_bytes = [], [], []
    for b, (name, block, data) in enumerate(blocks):
        n = len(data)
        near, alone = (P.boundaries_of(block), ()) if n <= BIG else P.sampled_boundaries(block, n, rng)
        view = memoryview(data)
        for k, t in enumerate(P.targets_for(n, near, rng, 36, alone)):
            cap = P.caps_for(t, n, k)
            r = min(t, cap, n)
            entries.append((b, t, cap))
            want_res.append(r)
            want_bytes.append(view[:r])
    return entries, want_res, want_bytes


def run_one_variant(engine, call, decoder, want_res, want_bytes, what):
    """One variant against the expectation.  Every byte inside the allowed ranges is compared with it and every byte outside
    with the guard pattern, so variants that all pass are identical to each other byte for byte."""
    res, out = call.run(engine, decoder)
    call.check(res, out, want_res, want_bytes, "%s, decoder %d" % (what, decoder))


# ---- 1. well-formed blocks -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hand_built():
    """{small, big}: (Call, expected results, expected bytes) over lz4_synth's valid blocks up to / above 8 KiB"""
    blocks = P.hand_built_blocks()
    assert len(blocks) > 100
    out = {}
    for part, keep in (("small", lambda n: n <= BIG), ("big", lambda n: n > BIG)):
        sel = [x for x in blocks if keep(len(x[2]))]
        assert len(sel) > 50
        entries, want_res, want_bytes = well_formed_entries(sel, random.Random(3))
        assert len(entries) > 10000
        out[part] = (Call([b for _, b, _ in sel], entries), want_res, want_bytes)
    return out


@pytest.mark.parametrize("part", ["small", "big"])
@pytest.mark.parametrize("decoder", VARIANTS)
def test_hand_built_blocks(engine, hand_built, decoder, part):
    """lz4_synth's structural edges, packed densely in one call.  Blocks of up to 8 KiB: every sequence boundary and its
    neighbours as a target.  Bigger blocks (window, batch, ring and segment edges of the decoders): the boundaries around
    the decoders' marks and every 32 KiB seam, the first and last eight, 24 at random (partial_cases.sampled_boundaries says
    why and which), and like all blocks n - 40 .. n + 1, the 16-byte marks and three dozen random targets."""
    call, want_res, want_bytes = hand_built[part]
    run_one_variant(engine, call, decoder, want_res, want_bytes, "hand-built " + part)


def _inputs(oracle, n):
    return [("text", oracle.gen("text", 1, max(n, 1))[:n].tobytes()), ("lzsynth", oracle.gen("lzsynth", 1, max(n, 1))[:n].tobytes()),
            ("random", oracle.gen("random", 1, max(n, 1))[:n].tobytes()), ("run", b"q" * n)]


@pytest.mark.parametrize("encoder", ["level0", "level9", "exact"])
def test_engine_written_blocks(engine, oracle, encoder):
    """blocks of this engine's encoders: 0, 1, 12, 13 bytes, 1 KiB, 64 KiB (several windows of the lane-parallel decoder) and
    256 KiB (several 32 KiB segments of the workgroup form); text-like, lzsynth, incompressible, one long run"""
    raws = [r for n in (0, 1, 12, 13, 1024, 65536, 262144) for _, r in _inputs(oracle, n)]
    try:
        if encoder == "level9":
            engine.set_compression_level(9)
        elif encoder == "exact":
            engine.set_compress_exact(True)
        framed, flen = engine.compress_batch(raws, accel=1, header_kind=4)
    finally:
        engine.set_compression_level(0)
        engine.set_compress_exact(False)
    blocks = split4(framed, flen)
    if encoder == "exact":
        # the exact mode writes ONE linked stream: only the blocks that decode on their own are well-formed without a dictionary
        keep = [i for i, (b, r) in enumerate(zip(blocks, raws)) if oracle.decompress_block(b, len(r)) == (len(r), r)]
        assert len(keep) >= 8
        blocks, raws = [blocks[i] for i in keep], [raws[i] for i in keep]
    named = [("%s %d" % (encoder, len(r)), b, r) for b, r in zip(blocks, raws)]
    entries, want_res, want_bytes = well_formed_entries(named, random.Random(5))
    call = Call(blocks, entries)
    for d in VARIANTS:
        run_one_variant(engine, call, d, want_res, want_bytes, encoder)


# ---- 2. the fixture: the reference's results on mutated blocks -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixture_cases():
    return P.load()


def test_fixture(engine, fixture_cases):
    """result[i] and the first max(result, 0) bytes are the reference's, for every recorded case, in a layout with guards
    between the prefixes"""
    cs = fixture_cases
    assert len(cs) >= 550
    entries = [(i, c.target, c.cap) for i, c in enumerate(cs)]
    lay = G.layout([min(c.target, c.cap) for c in cs])
    call = Call([c.block for c in cs], entries, lay)
    run_all_variants(engine, call, [c.result for c in cs], [c.prefix for c in cs], "fixture")


# ---- 3. confinement -----------------------------------------------------------------------------------------------------------------

def test_confinement_with_guards(engine, oracle):
    """well-formed blocks, blocks with an offset of 0, negative targets: nothing outside [outOff, outOff + min(target, cap)),
    with a guard behind every prefix (Call.run asserts it)"""
    rng = random.Random(9)
    data = oracle.gen("text", 1, 65536).tobytes()
    long_block = oracle.compress_block(data)
    zero_off = [Z.write_block([(b"abcdefgh", 0, 20)], b"0123456789ab"),
                Z.write_block([(b"abcdefghijklmnopqrstuvwxyz", 0, 300)], b"0123456789ab"),
                Z.write_block([(bytes(range(40, 140)), 7, 9), (b"xy", 0, 40), (b"", 5, 200)], b"0123456789ab")]
    zero_off += [c.block for c in Z.end_family() if c.name.startswith("offset 0")]
    blocks = [long_block] + zero_off
    entries, want_res, want_bytes = [], [], []
    for t in (0, 1, 15, 16, 17, 100, 255, 256, 1000, 1024, 6143, 6144, 6145, 32767, 32768, 32769, 65535, 65536, 70000, -1, -2 ** 31):
        for cap in (65536, 70000, 1000, 0):
            entries.append((0, t, cap))
            r = BLK_E_UNCOMPLEN if t < 0 else min(t, cap, 65536)
            want_res.append(r)
            want_bytes.append(data[:max(r, 0)] if t >= 0 else None)
    n_known = len(entries)
    for b in range(1, len(blocks)):
        for t in list(range(0, 64)) + [100, 200, 329, 330, 400]:
            entries.append((b, t, rng.choice((t, 64, 400, 1000))))
    lay = G.layout([0 if t < 0 else min(t, c) for _, t, c in entries])
    call = Call(blocks, entries, lay)
    first = None
    for d in VARIANTS:
        res, out = call.run(engine, d)
        call.check(res[:n_known], out, want_res, want_bytes, "decoder %d" % d)
        if first is None:
            first = (res, out)
        assert np.array_equal(res, first[0]) and torch.equal(out, first[1]), "decoder %d and %d disagree" % (VARIANTS[0], d)
        # offset 0: confinement (asserted by run) and some result: a count within the prefix asked for, or a codec error
        for (b, t, c), r in zip(entries[n_known:], res[n_known:]):
            assert -len(blocks[b]) - 1 <= r <= min(t, c), (d, b, t, c, r)


# ---- 4. framing and switches ----------------------------------------------------------------------------------------------------------

def _device_call(engine, blob, offs, targets, hk, fixed=0, caps=None, framed_len=None, room=None):
    n = len(offs)
    room = room if room is not None else [max(t, 0) for t in targets]
    lay = G.layout(room)
    out = G.new_torch(lay.total, SEED, DEV)
    res = G.GuardedArray(n, torch.int32, SEED + 1, DEV)
    engine.decompress_partial_device(_t(blob), len(blob) if framed_len is None else framed_len, _t(offs, np.int64), n, out,
                                     _t(lay.starts, np.int64), _t(targets, np.int32), res.view, header_kind=hk, fixed_uncomp=fixed,
                                     out_cap=None if caps is None else _t(caps, np.int32))
    engine.synchronize()
    return res, out, lay


@pytest.mark.parametrize("decoder", VARIANTS)
def test_framing(engine, oracle, decoder):
    datas = [oracle.gen("text", 1, 3000, first_block=i)[:n].tobytes() for i, n in enumerate((3000, 1000, 64, 2000))]
    blocks = [oracle.compress_block(d) for d in datas]
    targets = [100, 5000, 64, 0]
    engine.set_decoder(decoder)
    try:
        # kind 4: the capacity is fixedUncomp
        blob, offs = frame(blocks, 4)
        res, out, lay = _device_call(engine, blob, offs, targets, 4, fixed=3000, room=[100, 3000, 64, 0])
        assert res.view.cpu().tolist() == [100, 1000, 64, 0]
        G.assert_confined(out, [(s, s + r) for s, r in zip(lay.starts, (100, 1000, 64, 0))], SEED, "kind 4")
        for s, d, r in zip(lay.starts, datas, (100, 1000, 64, 0)):
            assert out[s:s + r].cpu().numpy().tobytes() == d[:r]
        # kind 8: the header's size is the capacity, with and without outCap; outCap below the header's size rejects the block
        blob, offs = frame(blocks, 8, [len(d) for d in datas])
        for caps, want in ((None, [100, 1000, 64, 0]), ([3000, 1000, 64, 2000], [100, 1000, 64, 0]), ([3000, 999, 64, 2000], [100, BLK_E_UNCOMPLEN, 64, 0])):
            res, out, lay = _device_call(engine, blob, offs, targets, 8, caps=caps, room=[100, 1000, 64, 0])
            assert res.view.cpu().tolist() == want
            G.assert_confined(out, [(s, s + max(r, 0)) for s, r in zip(lay.starts, want)], SEED, "kind 8")
            for s, d, r in zip(lay.starts, datas, want):
                assert out[s:s + max(r, 0)].cpu().numpy().tobytes() == d[:max(r, 0)]
        # negative target: MI355LZ4_BLK_E_UNCOMPLEN, nothing written
        res, out, lay = _device_call(engine, blob, offs, [100, -1, -5, 7], 8)
        assert res.view.cpu().tolist() == [100, BLK_E_UNCOMPLEN, BLK_E_UNCOMPLEN, 7]
        G.assert_confined(out, [(lay.starts[0], lay.starts[0] + 100), (lay.starts[3], lay.starts[3] + 7)], SEED, "negative targets")
        # the header rejections of the full decode (tests/test_parity_gpu.py, test_decode_header_rejections), nothing written
        fr, _ = frame(blocks[1:2], 8, [1000])
        res, out, lay = _device_call(engine, fr, [0], [500], 8, framed_len=len(fr) - 1)          # data runs past the buffer
        assert res.view.cpu().tolist() == [BLK_E_TRUNCATED]
        G.assert_confined(out, [], SEED, "truncated")
        bad = bytearray(fr)
        bad[0:4] = (0).to_bytes(4, "little")
        res, out, lay = _device_call(engine, bytes(bad), [0], [500], 8)                          # compLen <= 0
        assert res.view.cpu().tolist() == [BLK_E_COMPLEN]
        G.assert_confined(out, [], SEED, "compLen")
        bad = bytearray(fr)
        bad[4:8] = (-7).to_bytes(4, "little", signed=True)
        res, out, lay = _device_call(engine, bytes(bad), [0], [500], 8)                          # uncompLen < 0
        assert res.view.cpu().tolist() == [BLK_E_UNCOMPLEN]
        G.assert_confined(out, [], SEED, "uncompLen")
        res, out, lay = _device_call(engine, fr, [len(fr) - 3], [500], 8)                        # the header itself runs past the buffer
        assert res.view.cpu().tolist() == [BLK_E_TRUNCATED]
    finally:
        engine.set_decoder(0)


@pytest.mark.parametrize("decoder", VARIANTS)
def test_block_checksums(engine, slz4, oracle, decoder):
    """the trailer covers the whole compressed block, whatever the target"""
    datas = [oracle.gen("text", 1, 2000, first_block=i).tobytes() for i in range(3)]
    blocks = [oracle.compress_block(d) for d in datas]
    blob, offs = frame(blocks, 8, [2000] * 3, trailer=slz4.xxh32)
    engine.set_decoder(decoder)
    engine.set_block_checksum(True)
    try:
        res, out, lay = _device_call(engine, blob, offs, [10, 500, 3000], 8, room=[10, 500, 2000])
        assert res.view.cpu().tolist() == [10, 500, 2000]
        flipped = bytearray(blob)
        flipped[offs[2] - 1] ^= 0x01                      # block 1's trailer
        res, out, lay = _device_call(engine, bytes(flipped), offs, [10, 500, 3000], 8, room=[10, 500, 2000])
        assert res.view.cpu().tolist() == [10, BLK_E_CHECKSUM, 2000]
        G.assert_confined(out, [(lay.starts[0], lay.starts[0] + 10), (lay.starts[2], lay.starts[2] + 2000)], SEED, "bad trailer")
        res, out, lay = _device_call(engine, blob, offs, [10, 500, 100], 8, framed_len=len(blob) - 2)   # the last trailer past the buffer
        assert res.view.cpu().tolist() == [10, 500, BLK_E_TRUNCATED]
    finally:
        engine.set_block_checksum(False)
        engine.set_decoder(0)


def test_argument_errors(engine, slz4, oracle):
    f = slz4.lib.mi355lz4_decompress_partial_device
    d = torch.zeros(64, dtype=torch.int64, device=DEV)
    p = d.data_ptr()
    ctx = engine.ctx
    assert f(ctx, None, 0, None, 0, 8, 0, None, None, None, None, None) == 0                     # nBlocks == 0
    assert f(None, p, 8, p, 1, 8, 0, p, p, None, p, p) == E_ARG                                  # null ctx
    assert f(ctx, p, 8, p, -1, 8, 0, p, p, None, p, p) == E_ARG                                  # nBlocks < 0
    assert f(ctx, p, 8, p, 1, 5, 0, p, p, None, p, p) == E_ARG                                   # headerKind
    for hole in (1, 3, 8, 10, 11):                                                               # framed, blockOff, outOff, target, result
        args = [ctx, p, 8, p, 1, 8, 0, p, p, None, p, p]
        args[hole] = None
        assert f(*args) == E_ARG, hole
    assert b"decompress_partial_device" in slz4.lib.mi355lz4_last_error()
    # while a range begun with _linked_begin is open, the call is refused as the other decodes are
    n, bl = 8, 65536
    raw = oracle.gen("text", n, bl).tobytes()
    framed = oracle.frame_compress(raw, bl, 1, 8, True)
    offs, _ = slz4.index_host(framed, 8, 0)
    fr, boff = _t(framed), _t(offs, np.int64)
    ooff = (torch.arange(n + 1, dtype=torch.int64) * bl).to(DEV)
    out = torch.zeros(n * bl, dtype=torch.uint8, device=DEV)
    res = torch.zeros(n, dtype=torch.int32, device=DEV)
    tgt = torch.full((n,), 100, dtype=torch.int32, device=DEV)
    engine.decompress_linked_begin(fr, len(framed), boff, n, out, ooff, res, 0)
    try:
        with pytest.raises(slz4.LZ4Error):
            engine.decompress_partial_device(fr, len(framed), boff, n, out, ooff, tgt, res)
        with pytest.raises(slz4.LZ4Error):
            engine.decompress_partial(framed, 100)
    finally:
        engine.decompress_linked_end()
        engine.synchronize()
    assert res.cpu().tolist() == [bl] * n and out.cpu().numpy().tobytes() == raw


# ---- 5. the host form -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hk", [8, 4])
def test_host_form(engine, slz4, oracle, hk):
    sizes = [65536, 1000, 0, 13, 65536, 30000]
    datas = [oracle.gen("lzsynth", 1, 65536, first_block=i)[:n].tobytes() for i, n in enumerate(sizes)]
    blocks = [oracle.compress_block(d) for d in datas]
    framed, offs = frame(blocks, hk, sizes)
    fixed = 65536 if hk == 4 else 0
    caps = [fixed] * len(sizes) if hk == 4 else sizes
    # one target for all
    for t in (0, 1, 100, 1024, 40000, 70000):
        got, blen = engine.decompress_partial(framed, t, header_kind=hk, fixed_uncomp=fixed)
        assert blen == [min(t, n) for n in sizes]
        assert got == b"".join(d[:t] for d in datas)
    # one per block, and what the device call gives for the same arguments
    per = [5, 2000, 7, 12, 65536, 29999]
    got, blen = engine.decompress_partial(framed, per, header_kind=hk, fixed_uncomp=fixed)
    res, out, lay = _device_call(engine, framed, offs, per, hk, fixed=fixed, room=[min(t, c) for t, c in zip(per, caps)])
    assert blen == res.view.cpu().tolist() == [min(t, n) for t, n in zip(per, sizes)]
    assert got == b"".join(out[s:s + r].cpu().numpy().tobytes() for s, r in zip(lay.starts, blen))
    # a buffer too small: MI355LZ4_E_CAPACITY, nothing at or past out + cap (nothing at all)
    src = np.frombuffer(framed, dtype=np.uint8)
    need = sum(blen)
    lay = G.layout([need - 1])
    buf = G.new_numpy(lay.total, SEED)
    import ctypes as C
    u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    tarr = np.array(per, dtype=np.int32)
    bl = np.zeros(16, dtype=np.int32)
    out_len, nb = C.c_size_t(), C.c_int()
    rc = slz4.lib.mi355lz4_decompress_partial(engine.ctx, src.ctypes.data_as(u8p), src.size, hk, fixed, tarr.ctypes.data_as(i32p), 0,
                                              buf[lay.starts[0]:].ctypes.data_as(u8p), need - 1, C.byref(out_len),
                                              bl.ctypes.data_as(i32p), 16, C.byref(nb))
    assert rc == E_CAPACITY and nb.value == len(sizes) and bl[:nb.value].tolist() == blen
    G.assert_confined(buf, [], SEED, "host form, capacity too small")
    # a failed block: MI355LZ4_E_BLOCK and its code in blockLen
    got, blen = engine.decompress_partial(framed, [5, -1, 7, 12, 9, 9], header_kind=hk, fixed_uncomp=fixed, raise_on_block_error=False)
    assert blen == [5, BLK_E_UNCOMPLEN, 0, 12, 9, 9]


def test_host_form_checksums_and_short_blocks(engine, slz4, oracle):
    """The host form over a chain with trailers (mi355lz4_index_host_ex's trailer path), and blocks that give fewer bytes than
    min(target, capacity) -- their headers promise more than they hold -- so that the prefixes come back block by block."""
    sizes = [3000, 1000, 20000, 64]
    claimed = [3000, 4096, 65536, 64]                     # blocks 1 and 2 decode to less than their header says
    datas = [oracle.gen("text", 1, 20000, first_block=i)[:n].tobytes() for i, n in enumerate(sizes)]
    blocks = [oracle.compress_block(d) for d in datas]
    for ck in (False, True):
        framed, offs = frame(blocks, 8, claimed, trailer=slz4.xxh32 if ck else None)
        engine.set_block_checksum(ck)
        try:
            for t in (500, 2000, 30000):
                got, blen = engine.decompress_partial(framed, t)
                assert blen == [min(t, n) for n in sizes], (ck, t)
                assert got == b"".join(d[:t] for d in datas), (ck, t)
            per = [2999, 4000, 1, 100]
            got, blen = engine.decompress_partial(framed, per)
            assert blen == [2999, 1000, 1, 64] and got == b"".join(d[:r] for d, r in zip(datas, blen))
            if ck:
                bad = bytearray(framed)
                bad[offs[1] + 8 + 3] ^= 0x40              # a data byte of block 1: its trailer no longer matches
                got, blen = engine.decompress_partial(bytes(bad), 10, raise_on_block_error=False)
                assert blen == [10, BLK_E_CHECKSUM, 10, 10]
                with pytest.raises(slz4.LZ4Error):
                    engine.decompress_partial(bytes(bad), 10)
        finally:
            engine.set_block_checksum(False)


def test_cpp_mirror(engine, slz4, oracle, tmp_path):
    """streamly_lz4::Engine::decompressPartial from a program of its own, with and without trailers; its buffer is sized from the
    chain (a chain of many small blocks asked for a large target must not ask for blocks x target bytes)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sizes = [65536, 1000, 0, 13, 30000] + [40] * 3000
    datas = [oracle.gen("lzsynth", 1, 65536, first_block=i % 7)[:n].tobytes() for i, n in enumerate(sizes)]
    blocks = [oracle.compress_block(d) for d in datas]
    exe = str(tmp_path / "decompress_partial")
    libdir = os.path.join(root, "streamly-lz4_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "native", "decompress_partial_main.cpp"), "-L", libdir, "-lmi355lz4",
                           "-Wl,-rpath," + libdir, "-o", exe])
    for ck in (0, 1):
        path, outp = tmp_path / ("stream%d.bin" % ck), tmp_path / ("out%d.bin" % ck)
        path.write_bytes(frame(blocks, 8, sizes, trailer=slz4.xxh32 if ck else None)[0])
        for t in (1000, 1 << 30):                         # (blocks x 2^30 would be terabytes)
            r = subprocess.run([exe, str(path), str(ck), str(t), str(outp)], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (r.stdout[-300:], r.stderr)
            assert [int(x) for x in r.stdout.split()] == [min(t, n) for n in sizes], (ck, t)
            assert outp.read_bytes() == b"".join(d[:t] for d in datas), (ck, t)


# ---- 6. the early exit happens --------------------------------------------------------------------------------------------------------------

def test_early_exit(engine, oracle, record):
    """1024 lzsynth blocks of 64 KiB, lane-parallel decoder: asking for 1 KiB of each is faster than decoding them (a call that
    copies a sixty-fourth of the bytes and is not faster has not left its blocks early)"""
    n, bl, target, reps = 1024, 65536, 1024, 7
    src = torch.empty(n * bl, dtype=torch.uint8, device=DEV)
    engine.generate("lzsynth", src, bl, n)
    import streamly_lz4_amd as S
    stride = S.slot_stride(bl, 8)
    slots = torch.empty(n * stride, dtype=torch.uint8, device=DEV)
    flen = torch.zeros(n, dtype=torch.int32, device=DEV)
    engine.compress_batch_device(src, n, bl, slots, stride, flen)
    boff = (torch.arange(n, dtype=torch.int64, device=DEV) * stride)
    ooff = (torch.arange(n + 1, dtype=torch.int64, device=DEV) * bl)
    poff = (torch.arange(n + 1, dtype=torch.int64, device=DEV) * target)
    out = torch.zeros(n * bl, dtype=torch.uint8, device=DEV)
    pout = torch.zeros(n * target, dtype=torch.uint8, device=DEV)
    res = torch.zeros(n, dtype=torch.int32, device=DEV)
    pres = torch.zeros(n, dtype=torch.int32, device=DEV)
    tgt = torch.full((n,), target, dtype=torch.int32, device=DEV)
    engine.set_decoder(2)
    try:
        def timed(fn):
            ts = []
            for _ in range(reps + 2):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            return statistics.median(ts[2:])
        full = timed(lambda: engine.decompress_batch_device(slots, n * stride, boff, n, out, ooff, res))
        part = timed(lambda: engine.decompress_partial_device(slots, n * stride, boff, n, pout, poff, tgt, pres))
    finally:
        engine.set_decoder(0)
    engine.synchronize()
    assert res.cpu().tolist() == [bl] * n and pres.cpu().tolist() == [target] * n
    assert torch.equal(pout.view(n, target), src.view(n, bl)[:, :target])
    rec = {"test": "partial_early_exit", "blocks": n, "block_len": bl, "target": target, "full_ms": full, "partial_ms": part,
           "ratio": full / part}
    print(rec)
    record("partial_decode", rec)
    assert part < full, rec
