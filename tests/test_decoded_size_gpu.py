"""mi355lz4_decoded_size_device on the GPU: size[] equals the acceptance rule's model (tests/size_model.py, held to the oracle
by tests/test_decoded_size_host.py) on blocks of every encoder, on hand-built edges and on malformed blocks; decoding into
exactly size[i] bytes gives what decoding at fixedUncomp stride gives, for every decoder; the call writes size[] and outOff[]
and nothing else; and the host-buffer decode that is built on it returns what it returned before."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import guarded as G
import lz4_synth as Z
import size_model as M
from conftest import DECODERS

import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_BLOCK, E_CAPACITY = -3, -5, -4
BIG = 4 << 20
LENGTHS = (0, 1, 12, 13, 14, 4095, 65535, 65536, 256 << 10, 1 << 20, 4 << 20)


def _t(a, dtype=None):
    a = np.frombuffer(bytes(a), dtype=np.uint8).copy() if isinstance(a, (bytes, bytearray)) else np.asarray(a, dtype=dtype)
    return torch.from_numpy(a).to(DEV)


def gpu_sizes(engine, blob, offs, header_kind, max_uncomp, framed_len=None):
    """(size[], outOff[]) of the blocks at offs in blob"""
    n = len(offs)
    src = _t(blob if len(blob) else b"\0")
    size = torch.full((max(n, 1),), 77, dtype=torch.int32, device=DEV)
    ooff = torch.full((n + 1,), 77, dtype=torch.int64, device=DEV)
    engine.decoded_size_device(src, len(blob) if framed_len is None else framed_len, _t(offs, np.int64) if n else None, n, size, ooff,
                               header_kind, max_uncomp)
    engine.synchronize()
    return size.cpu().numpy()[:n], ooff.cpu().numpy()


def frame8(blocks, trailer=None, gap=0, seed=6):
    """headerKind 8 framing with an uncompLen that is deliberately not the block's (the size pass does not read it)"""
    rng = random.Random(seed)
    buf, offs = bytearray(), []
    for b in blocks:
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(1, gap + 1))) if gap else b""
        offs.append(len(buf))
        buf += len(b).to_bytes(4, "little") + rng.randrange(1 << 20).to_bytes(4, "little") + bytes(b)
        if trailer:
            buf += int(trailer(bytes(b))).to_bytes(4, "little")
    buf += bytes(rng.randrange(256) for _ in range(gap))
    return bytes(buf), offs


def check_against_model(engine, slz4, blocks, max_uncomp, combos, what):
    want = np.array([M.model_size(b, max_uncomp) for b in blocks], dtype=np.int64)
    scan = np.concatenate([[0], np.cumsum(np.maximum(want, 0))])
    for hk, ck, gap in combos:
        engine.set_block_checksum(ck)
        try:
            blob, offs = (M.frame4 if hk == 4 else frame8)(blocks, slz4.xxh32 if ck else None, gap)
            size, ooff = gpu_sizes(engine, blob, offs, hk, max_uncomp)
        finally:
            engine.set_block_checksum(False)
        bad = np.nonzero(size != want)[0]
        assert bad.size == 0, "%s (kind %d, checksums %s, gap %d): block %d of %d bytes: GPU %d, model %d" % (
            what, hk, ck, gap, bad[0], len(blocks[bad[0]]), size[bad[0]], want[bad[0]])
        assert np.array_equal(ooff, scan), (what, hk, ck, gap)
    return want


def split4(framed, flen):
    """the LZ4 blocks of a dense headerKind-4 stream (no trailers)"""
    out, pos = [], 0
    for f in flen:
        assert int.from_bytes(framed[pos:pos + 4], "little") == f - 4
        out.append(framed[pos + 4:pos + f])
        pos += f
    assert pos == len(framed)
    return out


@pytest.fixture(scope="module")
def raw_inputs(oracle):
    """[(kind, bytes)] for every length x kind"""
    return [(k, M.gen(oracle, k, n, n)) for n in LENGTHS for k in M.FUZZ_KINDS]


ALL_COMBOS = [(hk, ck, gap) for hk in (4, 8) for ck in (False, True) for gap in (0, 37)]


@pytest.mark.parametrize("encoder", ["oracle", "fast", "level9", "exact", "linked"])
def test_valid_blocks(engine, slz4, oracle, raw_inputs, encoder):
    raws = [r for _, r in raw_inputs]
    if encoder == "oracle":
        blocks = [oracle.compress_block(r) for r in raws]
        combos = ALL_COMBOS
    else:
        if encoder != "fast":
            # the slow encoders: every kind up to 1 MiB, and one block of 4 MiB
            raws = [r for k, r in raw_inputs if len(r) <= 1 << 20 or k == "lzsynth"]
        try:
            if encoder == "level9":
                engine.set_compression_level(9)
            elif encoder == "exact":
                engine.set_compress_exact(True)
            elif encoder == "linked":
                engine.set_linked_compress(True)
            framed, flen = engine.compress_batch(raws, accel=1, header_kind=4)
        finally:
            engine.set_compression_level(0)
            engine.set_compress_exact(False)
            engine.set_linked_compress(False)
        blocks = split4(framed, flen)
        combos = ALL_COMBOS
    want = check_against_model(engine, slz4, blocks, BIG, combos, encoder)
    if encoder in ("oracle", "fast", "level9"):
        # independent blocks of a conforming encoder: every size is known and is the input's length
        assert want.tolist() == [len(r) for r in raws]
    else:
        # blocks of a linked stream reach into their dictionary: offsets are not judged, so the sizes are known all the same.
        # The one exception is the rule's last clause, and a block without a size must be one it names: its chain gives the
        # input's length, and it has a match with extension bytes that ends in the last 64 bytes and reaches in front of
        # the block
        for b, r, w in zip(blocks, raws, want):
            if w >= 0:
                assert w == len(r)
                continue
            seqs = Z.parse(bytes(b))
            assert seqs[-1][5] + seqs[-1][2] == len(r)
            assert any((b[tp] & 15) == 15 and off > op + lit and op + lit + ml >= len(r) - M.TAIL
                       for tp, _, lit, off, ml, op in seqs[:-1]), len(r)
        assert (want < 0).sum() <= len(raws) // 8


def _edge_blocks():
    rng = random.Random(31)
    out = []

    def body(mid, name, last=12):
        b = Z.Builder(rng).fill(out_bytes=300)
        mid(b)
        b.fill(out_bytes=200)
        blk, n = b.block(last)
        out.append((name, blk, n))

    xs = [14, 15, 15 + 254, 15 + 255] + [15 + 255 * k + d for k in range(1, 261) for d in (0, 1)]
    for x in xs:
        body(lambda b: b.add(b"q" * x, rng.randint(1, 300), 6), "literals %d" % x)
        body(lambda b: b.add(3, rng.randint(1, 300), x + 4), "match field %d" % x)
    body(lambda b: b.add(b"q" * (15 + 255 * 40 + 3), 7, 15 + 255 * 50 + 4), "both long")
    # fields at compressed positions W - 2 .. W + 1 of the kernel's window (1024) and its multiples
    for W in (1024, 2048, 3072, 7168, 16384):
        for d in (-2, -1, 0, 1):
            at = W + d
            for name, back, seq in (("token", 0, (3, 20)), ("literal extension run", 3, (15 + 255 * 4 + 7, 8)),
                                    ("offset byte 0", 3, (2, 9)), ("offset byte 1", 4, (2, 9)),
                                    ("match extension run", 5, (0, 19 + 255 * 4 + 9))):
                b = Z.Builder(rng).fill(in_bytes=at - back - 60).pad_in(at - back)
                b.add(seq[0], rng.randint(1, 900), seq[1]).fill(out_bytes=400)
                blk, n = b.block(12)
                out.append(("%s at %d" % (name, at), blk, n))
    # extension runs of exactly 31, 32 and 33 bytes (the ballot over "byte != 255" works on 32-bit words), literal and match
    for k in (30, 31, 32, 33, 63, 64, 65):
        for d in (0, 1, 254):
            body(lambda b: b.add(b"q" * (15 + 255 * (k - 1) + d), rng.randint(1, 300), 6), "literal run of %d extension bytes" % k)
            body(lambda b: b.add(3, rng.randint(1, 300), 19 + 255 * (k - 1) + d), "match run of %d extension bytes" % k)
    for count in (63, 64, 65, 513):
        b = Z.Builder(rng).add(16, 16, 4)
        for _ in range(count):
            b.add(0, rng.randint(1, 16), 4)
        blk, n = b.block(12)
        out.append(("%d minimum sequences" % count, blk, n))
        b.fill(out_bytes=300)
        for _ in range(count):
            b.add(0, rng.randint(1, 16), 4)
        blk, n = b.block(8)
        out.append(("%d minimum sequences, twice" % count, blk, n))
    for last in (b"", b"a", b"abcdefghijklmno", bytes(range(1, 255)), bytes(70000)):
        out.append(("one token, %d literals" % len(last), Z.write_block([], last), len(last)))
    return out


def test_hand_built_edges(engine, slz4):
    cases = _edge_blocks()
    blocks = [c[1] for c in cases]
    want = check_against_model(engine, slz4, blocks, BIG, [(4, False, 0), (4, False, 37), (8, True, 0)], "edges")
    for (name, _, n), w in zip(cases, want):
        assert w == n, (name, w, n)                              # every one of them is a valid block, so a known size
    # the bound: s == maxUncomp is known, s == maxUncomp + 1 is not
    name, blk, n = cases[5]
    blob, offs = M.frame4([blk, blk])
    assert gpu_sizes(engine, blob, offs, 4, n)[0].tolist() == [n, n]
    assert gpu_sizes(engine, blob, offs, 4, n - 1)[0].tolist() == [M.UNKNOWN, M.UNKNOWN]
    assert M.model_size(blk, n) == n and M.model_size(blk, n - 1) == M.UNKNOWN


def test_window_edges(engine):
    """Fields at the edges the walk really has.  Its window starts at the 16-byte-aligned address of the token it is at, is 1024
    bytes long, and takes token candidates in its first 512 bytes only.  Every block here has its data at a 16-byte-aligned
    address and opens with one literal run of L bytes, which the walk steps over as one sequence: the next window then starts
    at compressed position ip & ~15 of the block.  From there plain sequences lead up to the field under test, placed at that
    window's bytes 510 .. 513 (the last candidates, the first token of the window after it) or, for a sequence that starts
    in front of byte 512, so that it ends at bytes 1022 .. 1026 (the last that lies entirely inside, the first that leaves)."""
    rng = random.Random(77)
    cases = []
    for L in (3000, 5003, 70001):
        def start():
            b = Z.Builder(rng).add(bytes(rng.randrange(256) for _ in range(L)), rng.randint(1, min(L, 65535)), 4)
            return b, b.ip & ~15
        for d in (-2, -1, 0, 1):
            for name, back, seq in (("token", 0, (3, 20)), ("literal extension run", 3, (15 + 255 * 4 + 7, 8)),
                                    ("offset byte 0", 3, (2, 9)), ("offset byte 1", 4, (2, 9)),
                                    ("match extension run", 5, (0, 19 + 255 * 4 + 9))):
                b, w0 = start()
                b.pad_in(w0 + 512 + d - back)
                b.add(seq[0], rng.randint(1, 900), seq[1]).fill(out_bytes=400)
                cases.append(("%s at window byte %d, L %d" % (name, 512 + d, L),) + b.block(12))
        for end in (1022, 1023, 1024, 1025, 1026):
            for ml in (8, 19 + 255 * 2):                       # the sequence's last bytes: its offset, or a match extension run
                b, w0 = start()
                b.pad_in(w0 + 500)
                lit = next(n for n in range(300, 700) if Z.seq_size(n, ml) == w0 + end - b.ip)
                b.add(lit, rng.randint(1, 900), ml).fill(out_bytes=400)
                cases.append(("sequence ends at window byte %d, L %d, match %d" % (end, L, ml),) + b.block(12))
    blob, offs = bytearray(), []
    for _, blk, _ in cases:
        blob += bytes(rng.randrange(256) for _ in range((12 - len(blob)) % 16))
        offs.append(len(blob))
        blob += len(blk).to_bytes(4, "little") + blk
    assert all((o + 4) % 16 == 0 for o in offs)
    size, _ = gpu_sizes(engine, bytes(blob), offs, 4, BIG)
    for (name, blk, n), got in zip(cases, size):
        assert M.model_size(blk, BIG) == n and got == n, (name, got, n)


@pytest.fixture(scope="module")
def fuzz(oracle):
    return M.fuzz_blocks(oracle)


def test_malformed_blocks(engine, slz4, fuzz):
    muts = [m for _, _, m in fuzz]
    want = check_against_model(engine, slz4, muts, 65536, [(4, False, 0), (8, False, 37)], "mutated")
    assert 50 < (want >= 0).sum() < 550
    synth = Z.independent_cases()
    blocks = [c.block for c in synth]
    want = check_against_model(engine, slz4, blocks, BIG, [(4, False, 0)], "lz4_synth")
    for c, w in zip(synth, want):
        if c.family == "ends" and (not c.valid or c.name.startswith("offset 0")):
            assert w == M.UNKNOWN, c
    # the block the capacity-dependent code was found on, and its harmless twin (test_decoded_size_host.py)
    near = Z.write_block([(b"abcdefgh", 9, 40)], b"0123456789ab")
    far = Z.write_block([(b"abcdefgh", 9, 40)], bytes(range(32, 132)))
    check_against_model(engine, slz4, [near, far, b"\x05", b"\x00"], BIG, [(4, False, 0)], "rule 4")


def test_header_codes(engine, oracle):
    good = oracle.compress_block(M.gen(oracle, "text", 3000))
    blob = bytearray()
    offs = []
    for comp_len, data in ((len(good), good), (0, b""), (-5, b""), (len(good), good), (len(good) + 1, good)):
        offs.append(len(blob))
        blob += int(comp_len).to_bytes(4, "little", signed=True) + data
    offs.append(len(blob) - 2)                                    # a header cut short by the buffer's end
    size, ooff = gpu_sizes(engine, bytes(blob), offs, 4, 65536)
    assert size.tolist() == [3000, M.E_COMPLEN, M.E_COMPLEN, 3000, M.E_TRUNCATED, M.E_TRUNCATED]
    assert ooff.tolist() == [0, 3000, 3000, 3000, 6000, 6000, 6000]
    # framedLen bounds the reads, whatever lies behind it
    size, _ = gpu_sizes(engine, bytes(blob) + bytes(64), offs[:4], 4, 65536, framed_len=offs[3] + 4 + len(good) - 1)
    assert size.tolist() == [3000, M.E_COMPLEN, M.E_COMPLEN, M.E_TRUNCATED]
    # block checksums on: the trailer must lie inside the buffer
    engine.set_block_checksum(True)
    try:
        blob4, o4 = M.frame4([good, good], lambda b: 0)
        size, _ = gpu_sizes(engine, blob4, o4, 4, 65536, framed_len=len(blob4) - 1)
    finally:
        engine.set_block_checksum(False)
    assert size.tolist() == [3000, M.E_TRUNCATED]
    # no blocks: fine, and the scan is one zero
    size, ooff = gpu_sizes(engine, b"", [], 4, 65536)
    assert ooff.tolist() == [0]


@pytest.mark.parametrize("decoder", DECODERS)
def test_agreement_with_decoders(engine, oracle, fuzz, decoder):
    """every accepted block, decoded into exactly size[i] bytes at the dense outOff: result and bytes of the decode at
    fixedUncomp stride"""
    F = 1 << 17
    blocks = [m for _, _, m in fuzz] + [c for _, c, _ in fuzz[:60]] + [c.block for c in Z.independent_cases() + Z.end_family()]
    blob, offs = M.frame4(blocks)
    size, ooff = gpu_sizes(engine, blob, offs, 4, F)
    keep = [i for i in range(len(blocks)) if size[i] >= 0]
    assert len(keep) > 300
    n = len(keep)
    src = _t(blob)
    boff = _t([offs[i] for i in keep], np.int64)
    caps = _t([size[i] for i in keep], np.int32)
    dense_off = np.concatenate([[0], np.cumsum([size[i] for i in keep])]).astype(np.int64)
    engine.set_decoder(decoder)
    try:
        out_f = torch.zeros(n * F, dtype=torch.uint8, device=DEV)
        res_f = torch.zeros(n, dtype=torch.int32, device=DEV)
        engine.decompress_batch_device(src, len(blob), boff, n, out_f, _t(np.arange(n, dtype=np.int64) * F), res_f, 4, F)
        out_d = torch.zeros(int(dense_off[-1]) + 16, dtype=torch.uint8, device=DEV)
        res_d = torch.zeros(n, dtype=torch.int32, device=DEV)
        engine.decompress_batch_device(src, len(blob), boff, n, out_d, _t(dense_off), res_d, 4, F, out_cap=caps)
        engine.synchronize()
    finally:
        engine.set_decoder(0)
    res_f, res_d = res_f.cpu().numpy(), res_d.cpu().numpy()
    assert np.array_equal(res_f, res_d), np.nonzero(res_f != res_d)[0][:8]
    out_f, out_d = out_f.cpu().numpy(), out_d.cpu().numpy()
    for k in range(n):
        if res_f[k] >= 0:
            assert res_f[k] == size[keep[k]]
            assert np.array_equal(out_f[k * F:k * F + res_f[k]], out_d[dense_off[k]:dense_off[k] + res_f[k]]), k


def test_confinement(engine, fuzz):
    """size[] and outOff[] between guards; the inputs bit-identical afterwards; without outOff only size[] is written"""
    blocks = [m for _, _, m in fuzz[:200]]
    blob, offs = M.frame4(blocks, gap=37)
    n = len(blocks)
    src, boff = _t(blob), _t(offs, np.int64)
    src0, boff0 = src.clone(), boff.clone()
    size = G.GuardedArray(n, torch.int32, 41, DEV)
    ooff = G.GuardedArray(n + 1, torch.int64, 42, DEV)
    engine.decoded_size_device(src, len(blob), boff, n, size.view, ooff.view, 4, 65536)
    engine.synchronize()
    size.check(what="size[]")
    ooff.check(what="outOff[]")
    want = [M.model_size(b, 65536) for b in blocks]
    assert size.view.cpu().tolist() == want
    size2 = G.GuardedArray(n, torch.int32, 43, DEV)
    ooff2 = G.GuardedArray(n + 1, torch.int64, 44, DEV)
    engine.decoded_size_device(src, len(blob), boff, n, size2.view, None, 4, 65536)
    engine.synchronize()
    size2.check(what="size[] without outOff")
    ooff2.check(0, 0, what="an outOff that was not handed in")
    assert size2.view.cpu().tolist() == want
    assert torch.equal(src, src0) and torch.equal(boff, boff0)


def test_python_mirror(engine, oracle):
    raws = [M.gen(oracle, k, n, 3) for k in M.FUZZ_KINDS for n in (1, 13, 700, 65536)]
    framed, _ = engine.compress_batch(raws, header_kind=4)
    got = engine.decoded_sizes(framed, header_kind=4, max_uncomp=65536)
    assert got.dtype == np.int32 and got.tolist() == [len(r) for r in raws]
    assert engine.decoded_sizes(framed, header_kind=4, max_uncomp=699).tolist() == [len(r) if len(r) <= 699 else M.UNKNOWN for r in raws]
    framed8, _ = engine.compress_batch(raws, header_kind=8)
    assert engine.decoded_sizes(framed8, header_kind=8, max_uncomp=65536).tolist() == [len(r) for r in raws]
    assert engine.decoded_sizes(b"", header_kind=4, max_uncomp=65536).size == 0


def test_cxx_engine_decoded_sizes(engine, slz4, oracle, tmp_path):
    """streamly_lz4::Engine::decodedSizes (include/streamly_lz4.hpp) and the C call under it, mi355lz4_decoded_sizes_host:
    a C++ program built against the public header answers what the device call answers, with and without block checksums"""
    raws = [M.gen(oracle, k, n, 5) for k in M.FUZZ_KINDS for n in (1, 13, 700, 65536, 200000)]
    blocks = [oracle.compress_block(r) for r in raws]
    blocks[3] = blocks[3][:-1]                                   # one block without a size
    want = [M.model_size(b, 1 << 17) for b in blocks]
    assert want[3] == M.UNKNOWN and want.count(M.UNKNOWN) == 5   # and the four of 200 000 bytes, over the bound
    # the C call, from here
    blob, offs = M.frame4(blocks)
    arr = np.frombuffer(blob, dtype=np.uint8)
    off = np.asarray(offs, dtype=np.uint64)
    got = np.full(len(blocks), 77, dtype=np.int32)
    u8p, u64p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    rc = slz4.lib.mi355lz4_decoded_sizes_host(engine.ctx, arr.ctypes.data_as(u8p), arr.size, off.ctypes.data_as(u64p),
                                              len(blocks), 4, 1 << 17, got.ctypes.data_as(i32p))
    assert rc == 0 and got.tolist() == want
    assert slz4.lib.mi355lz4_decoded_sizes_host(engine.ctx, arr.ctypes.data_as(u8p), arr.size, off.ctypes.data_as(u64p),
                                                len(blocks), 4, -1, got.ctypes.data_as(i32p)) == E_ARG
    # the C++ wrapper, from a program of its own
    exe = str(tmp_path / "decoded_sizes")
    libdir = os.path.join(ROOT, "streamly-lz4_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "decoded_sizes_main.cpp"), "-L", libdir, "-lmi355lz4",
                           "-Wl,-rpath," + libdir, "-o", exe])
    for ck in (0, 1):
        path = tmp_path / ("stream%d.bin" % ck)
        path.write_bytes(M.frame4(blocks, slz4.xxh32 if ck else None)[0])
        r = subprocess.run([exe, str(path), str(ck), str(1 << 17)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert [int(x) for x in r.stdout.split()] == want, ck


# ---- the host-buffer decode built on the size pass ---------------------------------------------------------------------------

def _ragged(oracle, count, lo, hi, seed):
    rng = random.Random(seed)
    return [M.gen(oracle, rng.choice(M.FUZZ_KINDS), rng.randint(lo, hi), i) for i in range(count)]


def _expected(oracle, blocks, F, cap):
    """what mi355lz4_decompress_batch answers, from the oracle's decode of every block at capacity F: (return code, bytes,
    blockLen) -- a failed block beats a short buffer, and either leaves no output"""
    res = [oracle.decompress_block(b, F) for b in blocks]
    codes = [c for c, _ in res]
    if any(c < 0 for c in codes):
        return E_BLOCK, b"", codes
    if sum(codes) > cap:
        return E_CAPACITY, b"", codes
    return 0, b"".join(d for _, d in res), codes


def _host_call(engine, slz4, framed, F, cap, **kw):
    try:
        out, blen = engine.decompress_batch(framed, header_kind=4, fixed_uncomp=F, cap=cap, raise_on_block_error=False, **kw)
    except slz4.LZ4Error as e:
        assert "(%d)" % E_CAPACITY in str(e), e
        return E_CAPACITY, b"", None
    return (E_BLOCK if any(b < 0 for b in blen) else 0), out, blen


@pytest.mark.parametrize("count,lo,hi,F", [(300, 1, 65536, 65536), (64, 1, 4096, BIG)])
def test_host_path_dense(engine, slz4, oracle, count, lo, hi, F):
    raws = _ragged(oracle, count, lo, hi, count)
    blocks = [oracle.compress_block(r) for r in raws]
    framed, _ = M.frame4(blocks)
    total = sum(len(r) for r in raws)
    rc, out, blen = _host_call(engine, slz4, framed, F, total)
    assert rc == 0 and blen == [len(r) for r in raws] and out == b"".join(raws)
    assert _host_call(engine, slz4, framed, F, total - 1)[0] == E_CAPACITY
    # one mutated block in the middle: what the call answered before the size pass existed, taken from the oracle
    rng = random.Random(count)
    seen = set()
    for trial in range(6):
        mut = list(blocks)
        k = count // 2
        m = bytearray(mut[k])
        if trial == 0:
            m[-1:] = b""                                     # the chain no longer ends at the block's end
        elif trial == 1:
            m = bytearray(Z.write_block([(b"abcdefgh", 9, 40)], b"0123456789ab"))     # known to the rule's last clause
        else:
            m[rng.randrange(len(m))] ^= 1 << rng.randrange(8)
        mut[k] = bytes(m)
        want = _expected(oracle, mut, F, total)
        got = _host_call(engine, slz4, M.frame4(mut)[0], F, total)
        assert got[0] == want[0] and got[1] == want[1], (trial, got[0], want[0])
        if got[2] is not None:
            assert got[2] == want[2], trial
        seen.add(want[0])
    assert E_BLOCK in seen


def test_host_path_streams(engine, slz4, oracle):
    """ragged blocks through the streams call and through a linked call (both take the same host path)"""
    raws = _ragged(oracle, 90, 1, 65536, 7)
    framed, _ = M.frame4([oracle.compress_block(r) for r in raws])
    out, blen = engine.decompress_streams(framed, [0, 30, 31, 90], header_kind=4, fixed_uncomp=65536)
    assert blen == [len(r) for r in raws] and out == b"".join(raws)
    engine.set_linked_compress(True)
    try:
        linked, _ = engine.compress_batch(raws, header_kind=4)
    finally:
        engine.set_linked_compress(False)
    out, blen = engine.decompress_streams(linked, [0, 90], header_kind=4, fixed_uncomp=65536)
    assert blen == [len(r) for r in raws] and out == b"".join(raws)
    total = sum(len(r) for r in raws)
    out, blen = engine.decompress_batch(linked, header_kind=4, fixed_uncomp=65536, linked=True, cap=total)
    assert blen == [len(r) for r in raws] and out == b"".join(raws)
