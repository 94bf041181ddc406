"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded
inputs, against the committed golden fixtures, and through the round-trip properties of the
reference's own suite (reference test/Main.hs:57-306).  Bar: bit-exact (u8 work)."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

from conftest import DECODERS

pytestmark = pytest.mark.gpu


def sha(b):
    return hashlib.sha256(b).hexdigest()


def split_blocks(fr, meta=8):
    out, pos = [], 0
    while pos < len(fr):
        c = int.from_bytes(fr[pos:pos + 4], "little")
        out.append(fr[pos:pos + meta + c])
        pos += meta + c
    return out


# --------------------------------------------------------------------------------------------
# decode: bit-exact vs oracle / golden
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder", DECODERS)
@pytest.mark.parametrize("kind", ["lzsynth", "text", "random"])
def test_decode_matches_oracle(engine, oracle, kind, decoder):
    engine.set_decoder(decoder)
    try:
        for bl in (1, 5, 12, 13, 63, 64, 65, 300, 4096, 65536, 100001, 262144):
            for accel in (1, 5, 400):
                n = 5
                data = oracle.gen(kind, n, bl, first_block=bl).tobytes()
                fr = oracle.frame_compress(data, bl, accel, 8, False)          # independent blocks
                out, blen = engine.decompress_batch(fr)
                assert blen == [bl] * n and out == data, (kind, bl, accel)
                out, blen = engine.decompress_batch(fr, linked=True)
                assert out == data
    finally:
        engine.set_decoder(0)


def test_decode_golden_streams(engine, oracle, golden):
    for s in golden["streams"]:
        data = oracle.gen(s["kind"], s["n_blocks"], s["block_len"]).tobytes()
        fr = oracle.frame_compress(data, s["block_len"], s["accel"], 8, s["linked"])
        assert sha(fr) == s["framed_sha256"]                                   # the reference's own bytes
        out, blen = engine.decompress_batch(fr, linked=True)
        assert sha(out) == s["raw_sha256"], s
        if not s["linked"]:
            out, _ = engine.decompress_batch(fr, linked=False)
            assert sha(out) == s["raw_sha256"], s


def test_decode_linked_fixture(engine, linked_golden):
    """Reference-produced linked stream: blocks 1-3 fail standalone with the reference's codes and
    decode through stream semantics (cbits/lz4.c:2347-2355)."""
    fr = bytes.fromhex(linked_golden["framed_hex"])
    out, blen = engine.decompress_batch(fr, linked=False, raise_on_block_error=False)
    assert blen == linked_golden["standalone_codes"]
    out, blen = engine.decompress_batch(fr, linked=True)
    assert blen == [linked_golden["block_len"]] * 4 and sha(out) == linked_golden["raw_sha256"]


@pytest.mark.parametrize("decoder", DECODERS)
def test_decode_malformed_codes(engine, golden, decoder):
    """Negative codes -(ip-src)-1 (cbits/lz4.c:2163) equal the reference's, for both decoder kernels."""
    engine.set_decoder(decoder)
    try:
        for m in golden["malformed"]:
            payload = bytes.fromhex(m["payload_hex"])
            if len(payload) == 0:
                continue                                                        # compLen 0 is rejected at the header
            fr = len(payload).to_bytes(4, "little") + payload
            out, blen = engine.decompress_batch(fr, header_kind=4, fixed_uncomp=m["cap"], raise_on_block_error=False)
            assert blen == [m["code"]], (m["name"], blen)
            if m["code"] >= 0:
                assert sha(out) == m["out_sha256"]
    finally:
        engine.set_decoder(0)


@pytest.mark.parametrize("decoder", DECODERS)
def test_decode_fuzz_vs_oracle(engine, oracle, decoder):
    """Mutated / truncated blocks, batched: every status and every decoded byte equals the oracle's."""
    engine.set_decoder(decoder)
    rng = random.Random(2024 + decoder)
    payloads, caps = [], []
    for it in range(600):
        kind = rng.choice(["lzsynth", "text", "random"])
        n = rng.choice([1, 12, 13, 20, 64, 65, 100, 300, 2000, 9000])
        data = oracle.gen(kind, 1, n, first_block=it).tobytes()
        comp = bytearray(oracle.compress_block(data, rng.choice([1, 1, 9])))
        mode = rng.randrange(5)
        if mode == 1:
            comp = comp[: rng.randrange(1, len(comp) + 1)]
        elif mode == 2:
            for _ in range(rng.randrange(1, 4)):
                comp[rng.randrange(len(comp))] = rng.randrange(256)
        elif mode == 3:
            comp += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 6)))
        cap = n if mode != 4 else max(0, n + rng.randrange(-20, 20))
        payloads.append(bytes(comp))
        caps.append(cap)
    try:
        # headerKind 8 lets every block carry its own capacity; pad the tail so the out-of-block reads
        # the reference performs on malformed input see zeros in both implementations
        for i in range(0, len(payloads), 50):
            for p, cap in zip(payloads[i:i + 50], caps[i:i + 50]):
                fr = len(p).to_bytes(4, "little") + cap.to_bytes(4, "little") + p
                want_code, want = oracle.decompress_block(p, cap)
                out, blen = engine.decompress_batch(fr, raise_on_block_error=False)
                assert blen == [want_code], (len(p), cap, blen, want_code)
                if want_code >= 0:
                    assert out == want
    finally:
        engine.set_decoder(0)


@pytest.mark.parametrize("decoder", DECODERS)
def test_decode_huge_length_fields(engine, oracle, decoder):
    """Length fields that are multi-megabyte runs of 0xFF (lengths >= 2^31): same code as the oracle, and
    nothing is written outside the block's output (cbits/lz4.c:1811-1818, 1854-1858, 2064-2065)."""
    import torch
    import guarded as G
    from reference_cases import huge_length_blocks
    dev = torch.device("cuda:0")
    cases = huge_length_blocks()
    lay = G.layout([cap for _, _, cap in cases])                                 # every block's output between guards
    blob, boff = b"", []
    for _, payload, cap in cases:
        boff.append(len(blob))
        blob += len(payload).to_bytes(4, "little") + cap.to_bytes(4, "little") + payload
    buf = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    out = G.new_torch(lay.total, 1, dev)
    res = G.GuardedArray(len(cases), torch.int32, 2, dev)
    engine.set_decoder(decoder)
    try:
        for name, payload, cap in cases:                                         # the host-buffer call, a block a call
            fr = len(payload).to_bytes(4, "little") + cap.to_bytes(4, "little") + payload
            want_code, want = oracle.decompress_block(payload, cap)
            host_out, blen = engine.decompress_batch(fr, raise_on_block_error=False)
            assert blen == [want_code], (name, blen, want_code)
            if want_code >= 0:
                assert host_out == want
        engine.decompress_batch_device(buf, len(blob), torch.tensor(boff, dtype=torch.int64, device=dev), len(cases), out,
                                       torch.tensor(lay.starts, dtype=torch.int64, device=dev), res.view)
        engine.synchronize()
    finally:
        engine.set_decoder(0)
    got = res.view.cpu().tolist()
    for i, (name, payload, cap) in enumerate(cases):
        want_code, want = oracle.decompress_block(payload, cap)
        assert got[i] == want_code, (name, got[i], want_code)
        if want_code >= 0:
            assert out[lay.starts[i]:lay.starts[i] + want_code].cpu().numpy().tobytes() == want
    G.assert_confined(out, lay.ranges(), 1, "huge length fields, decoder %d" % decoder)   # whatever the blocks' results
    res.check(what="result[]")


def test_decode_header_rejections(engine, oracle):
    """decompressChunk's header checks (Internal/LZ4.hs:309-318) + the short-array case it misses."""
    data = oracle.gen("text", 1, 1000).tobytes()
    fr = oracle.frame_compress(data, 1000, 1, 8, False)
    import torch
    dev = torch.device("cuda:0")
    buf = torch.from_numpy(np.frombuffer(fr, dtype=np.uint8).copy()).to(dev)
    off = torch.zeros(1, dtype=torch.int64, device=dev)
    out = torch.zeros(2000, dtype=torch.uint8, device=dev)
    res = torch.zeros(1, dtype=torch.int32, device=dev)
    engine.decompress_batch_device(buf, len(fr), off, 1, out, off, res)
    engine.synchronize()
    assert res.item() == 1000
    engine.decompress_batch_device(buf, len(fr) - 1, off, 1, out, off, res)    # data runs past the buffer
    engine.synchronize()
    assert res.item() == -0x7F000002
    bad = bytearray(fr)
    bad[0:4] = (0).to_bytes(4, "little")
    buf2 = torch.from_numpy(np.frombuffer(bytes(bad), dtype=np.uint8).copy()).to(dev)
    engine.decompress_batch_device(buf2, len(fr), off, 1, out, off, res)       # compLen <= 0
    engine.synchronize()
    assert res.item() == -0x7F000001


# --------------------------------------------------------------------------------------------
# encode: valid LZ4 that the oracle (reference algorithm) decodes bit-exact; sizes vs reference
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lzsynth", "text", "random"])
def test_encode_roundtrips_through_oracle(engine, oracle, kind):
    for bl in (0, 1, 12, 13, 14, 63, 64, 65, 1000, 65535, 65536, 65537, 100000, 262144):
        for accel in (-1, 1, 5, 400, 65537, 10 ** 6):
            n = 4
            data = oracle.gen(kind, n, max(bl, 1), first_block=7 * bl + 1)[: n * bl].tobytes() if bl else b""
            blocks = [data[i * bl:(i + 1) * bl] for i in range(n)]
            fr, flen = engine.compress_batch(blocks, accel=accel)
            assert len(fr) == sum(flen)
            pos = 0
            for i, f in enumerate(flen):                                        # header layout, Internal/LZ4.hs:261-262
                assert int.from_bytes(fr[pos:pos + 4], "little") == f - 8
                assert int.from_bytes(fr[pos + 4:pos + 8], "little") == bl
                assert f - 8 <= oracle.compress_bound(bl)
                code, out = oracle.decompress_block(fr[pos + 8:pos + f], bl)    # standalone: independent blocks
                assert code == bl and out == blocks[i], (kind, bl, accel, i)
                pos += f
            assert oracle.frame_decompress(fr, n * bl, 8, 0, True) == data      # and through the linked decoder


def test_encode_size_vs_reference(engine, oracle):
    """Compressed size is reported against the reference's _continue (LINKED) stream at the same acceleration (north
    star).  Tolerances are what scripts/size_vs_ref.py measured on these inputs plus 1 %: one wave per block (big
    batches) lzsynth <= 1.024, text <= 1.052 (accel 5, 64 KiB; 1.020 at accel 1); segmented (small batches) lzsynth
    <= 1.022, text <= 1.036.  Against the reference compressing the same blocks INDEPENDENTLY, as this engine does,
    text is 0.97-1.00."""
    try:
        for segs, tols in ((0, (("lzsynth", 1.034), ("text", 1.062), ("random", 1.001))),
                           (-1, (("lzsynth", 1.033), ("text", 1.046), ("random", 1.001)))):
            engine.set_segments(segs)
            for kind, tol in tols:
                for bl in (65536, 262144):
                    for accel in (1, 5):
                        n = 8
                        data = oracle.gen(kind, n, bl).tobytes()
                        ours = len(engine.compress_batch([data[i * bl:(i + 1) * bl] for i in range(n)], accel=accel)[0])
                        ref = len(oracle.frame_compress(data, bl, accel, 8, True))
                        assert ours <= ref * tol, (segs, kind, bl, accel, ours, ref)
    finally:
        engine.set_segments(-1)


def test_linked_compress(engine, oracle):
    """Linked compression (mi355lz4_set_linked_compress: block i-1 is block i's dictionary, what the reference's
    LZ4_compress_fast_continue does with the previous chunk, cbits/lz4.c:1608-1636): the stream decodes through the
    oracle's LINKED decoder and through the GPU's (linked = 1) to the input, its blocks really reach into their
    predecessors, and its size is the reference's linked size within the tolerance of the independent case --
    i.e. the +6 % an independent-block stream gives away on text is gone."""
    rng = random.Random(31)
    try:
        for kind, tol in (("text", 1.06), ("lzsynth", 1.04)):
            for bl, n in ((65536, 12), (16384, 9), (262144, 3)):
                data = oracle.gen(kind, n, bl, first_block=77).tobytes()
                blocks = [data[i * bl:(i + 1) * bl] for i in range(n)]
                engine.set_linked_compress(False)
                indep = engine.compress_batch(blocks)[0]
                engine.set_linked_compress(True)
                fr, flen = engine.compress_batch(blocks)
                assert oracle.frame_decompress(fr, n * bl, 8, 0, True) == data
                out, blen = engine.decompress_batch(fr, linked=True)
                assert out == data and blen == [bl] * n
                ref = len(oracle.frame_compress(data, bl, 1, 8, True))
                assert len(fr) <= ref * tol, (kind, bl, len(fr), ref)
                if kind == "text":
                    # the dictionary pays (less so when a block is four windows long)
                    assert len(fr) < len(indep) * (0.985 if bl <= 65536 else 1.0), (bl, len(fr), len(indep))
                    print("linked compress, text, %d-byte blocks: %d bytes; independent %d; reference linked %d"
                          % (bl, len(fr), len(indep), ref))
                    _, standalone = engine.decompress_batch(fr, linked=False, raise_on_block_error=False)
                    assert standalone[0] == bl and sum(1 for r in standalone[1:] if r < 0) >= n // 2
        # the stream combinators over the same switch: compressChunks writes the linked stream, decompressChunks reads it
        import streamly_lz4_amd as S
        data = oracle.gen("text", 40, 32768, first_block=3).tobytes()
        arrays = [data[i * 32768:(i + 1) * 32768] for i in range(40)]
        cfg = S.defaultBlockConfig
        linked_arrays = S.compressChunks(cfg, 1, arrays, engine)
        assert b"".join(S.decompressChunks(cfg, linked_arrays, engine)) == data
        engine.set_linked_compress(False)
        indep_arrays = S.compressChunks(cfg, 1, arrays, engine)
        engine.set_linked_compress(True)
        assert sum(map(len, linked_arrays)) < 0.95 * sum(map(len, indep_arrays))
        # ragged blocks (a short block is a short dictionary; an empty one is none), and a block above 64 KiB
        sizes = [65536, 1000, 65536, 0, 13, 12, 40000, 70000, 65536, 5]
        data = oracle.gen("text", 8, 65536, first_block=5).tobytes()
        blocks, pos = [], 0
        for sz in sizes:
            blocks.append(data[pos:pos + sz])
            pos += sz
        fr, flen = engine.compress_batch(blocks)
        out, blen = engine.decompress_batch(fr, linked=True)
        assert blen == sizes and out == data[:pos]
        # the oracle's linked decoder, block by block, with the previous non-empty block as dictionary
        dict_bytes, o = None, 0
        for b, sz in zip(split_blocks(fr), sizes):
            code, dec = oracle.decompress_block(b[8:], sz, dict_bytes)
            assert code == sz and dec == data[o:o + sz]
            o += sz
            if code > 0:
                dict_bytes = dec
    finally:
        engine.set_linked_compress(False)


def test_compact_honours_dense_cap(engine, slz4, oracle):
    """mi355lz4_compact_device never writes at or past denseCap: blocks that do not fit are skipped and
    denseOff[nBlocks] still reports the bytes the whole stream needs."""
    import torch
    dev = torch.device("cuda:0")
    bl, n = 4096, 16
    raw = oracle.gen("random", n, bl).tobytes()
    src = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dev)
    stride = slz4.slot_stride(bl, 8)
    slots = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    flen = torch.empty(n, dtype=torch.int32, device=dev)
    engine.compress_batch_device(src, n, bl, slots, stride, flen)
    engine.synchronize()
    need = int(flen.sum().item())
    cap = need // 2                                             # undersized on purpose
    dense = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev)
    doff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    engine.compact_device(slots, stride, flen, n, dense, cap, doff)
    engine.synchronize()
    assert int(doff[-1].item()) == need                          # the caller can see it did not fit
    assert bool((dense[cap:] == 0xA5).all().item())              # nothing at or past denseCap was touched
    fitted = [i for i in range(n) if int(doff[i + 1].item()) <= cap]
    assert fitted and len(fitted) < n
    for i in fitted:
        a, b = int(doff[i].item()), int(doff[i + 1].item())
        assert torch.equal(dense[a:b], slots[i * stride:i * stride + (b - a)])


def test_encode_special_inputs(engine, oracle):
    cases = [bytes(65536), bytes(262144), b"a" * 13, b"a" * 64, b"ab" * 5000, bytes(range(256)) * 300,
             bytes(((i * 7 + (i >> 8)) & 255) for i in range(65536))]
    fr, flen = engine.compress_batch(cases)
    assert oracle.frame_decompress(fr, sum(map(len, cases)), 8, 0, True) == b"".join(cases)
    assert flen[0] - 8 <= 400 and flen[1] - 8 <= 1300                          # zeros stay tiny (ref: 267 / 1038)
    # determinism
    assert engine.compress_batch(cases)[0] == fr


def test_header_kind_4(engine, oracle):
    bl = 65536
    data = oracle.gen("lzsynth", 3, bl).tobytes()
    blocks = [data[i * bl:(i + 1) * bl] for i in range(3)]
    fr, flen = engine.compress_batch(blocks, header_kind=4)
    assert oracle.frame_decompress(fr, 3 * bl, 4, bl, True) == data
    out, blen = engine.decompress_batch(fr, header_kind=4, fixed_uncomp=bl)
    assert out == data and blen == [bl] * 3


# --------------------------------------------------------------------------------------------
# the reference's own properties (test/Main.hs), restated over the mirror API
# --------------------------------------------------------------------------------------------
def gen_01(rng, lo, hi, p_one=0.5):
    n = rng.randint(lo, hi)
    return bytes(np.frombuffer(rng.randbytes(n), dtype=np.uint8) < int(256 * p_one))   # {0,1} bytes


@pytest.mark.parametrize("accel", [-1, 0, 1, 5, 12])
def test_decompressCompressChunk(slz4, engine, accel):                         # test/Main.hs:57-65
    rng = random.Random(accel + 100)
    arr = gen_01(rng, 10 * 1024, 100 * 1024)
    comp = slz4.compressChunks(slz4.defaultBlockConfig, accel, [arr], engine)
    assert slz4.decompressChunksRaw(slz4.defaultBlockConfig, comp, engine) == [arr]


def test_decompressCompressChunk2_legacy_ctx(slz4, engine, oracle):            # test/Main.hs:67-78
    """Two consecutive blocks through the SAME legacy contexts (the exact 7-symbol face)."""
    rng = random.Random(3)
    L = slz4.lib
    u8p = C.POINTER(C.c_uint8)
    arrs = [gen_01(rng, 10 * 1024, 100 * 1024), gen_01(rng, 10 * 1024, 100 * 1024), b"", b"x" * 5]
    cctx, dctx = L.LZ4_createStream(), L.LZ4_createStreamDecode()
    try:
        for arr in arrs:
            src = np.frombuffer(arr, dtype=np.uint8).copy() if arr else np.zeros(1, np.uint8)
            bound = L.LZ4_compressBound(len(arr))
            dst = np.zeros(bound, dtype=np.uint8)
            c = L.LZ4_compress_fast_continue(cctx, src.ctypes.data_as(u8p), dst.ctypes.data_as(u8p), len(arr), bound, 1)
            assert c > 0
            assert oracle.decompress_block(dst[:c].tobytes(), len(arr)) == (len(arr), arr)
            back = np.zeros(max(len(arr), 1), dtype=np.uint8)
            d = L.LZ4_decompress_safe_continue(dctx, dst.ctypes.data_as(u8p), back.ctypes.data_as(u8p), c, len(arr))
            assert d == len(arr) and back[:d].tobytes() == arr
    finally:
        L.LZ4_freeStream(cctx)
        L.LZ4_freeStreamDecode(dctx)


def test_legacy_decoder_accepts_reference_linked_stream(slz4, engine, linked_golden):
    """The legacy face is a drop-in for streams the REFERENCE compressor wrote (blocks linked)."""
    L = slz4.lib
    u8p = C.POINTER(C.c_uint8)
    fr = bytes.fromhex(linked_golden["framed_hex"])
    bl = linked_golden["block_len"]
    dctx = L.LZ4_createStreamDecode()
    out = b""
    try:
        for blk in split_blocks(fr):
            src = np.frombuffer(blk[8:], dtype=np.uint8).copy()
            back = np.zeros(bl, dtype=np.uint8)
            d = L.LZ4_decompress_safe_continue(dctx, src.ctypes.data_as(u8p), back.ctypes.data_as(u8p), src.size, bl)
            assert d == bl
            out += back.tobytes()
    finally:
        L.LZ4_freeStreamDecode(dctx)
    assert sha(out) == linked_golden["raw_sha256"]


@pytest.mark.parametrize("batch", [1, 3, 4096])
def test_decompressResizedcompress(slz4, engine, batch):                       # test/Main.hs:80-89, 271-285
    rng = random.Random(batch)
    engine.set_batch_blocks(batch)
    try:
        arrays = [gen_01(rng, 0, 3000) for _ in range(60)] + [b"", b"\x01"]
        comp = slz4.compressChunks(slz4.defaultBlockConfig, 5, arrays, engine)
        assert len(comp) == len(arrays)
        assert slz4.decompressChunksRaw(slz4.defaultBlockConfig, comp, engine) == arrays
    finally:
        engine.set_batch_blocks(4096)


@pytest.mark.parametrize("bufsize", [1, 512, 32 * 1024, 256 * 1024])
@pytest.mark.parametrize("accel", [-1, 5, 12, 100])
def test_decompressCompress_rechunked(slz4, engine, bufsize, accel):           # test/Main.hs:91-103, 217-224
    rng = random.Random(bufsize + accel)
    n_arr = 3 if bufsize == 1 else 20
    arrays = [gen_01(rng, 0, 2000 if bufsize == 1 else 40000) for _ in range(n_arr)]
    comp = b"".join(slz4.compressChunks(slz4.defaultBlockConfig, accel, arrays, engine))
    chunks = [comp[i:i + bufsize] for i in range(0, len(comp), bufsize)]       # readChunksWithBufferOf bufsize
    assert slz4.decompressChunks(slz4.defaultBlockConfig, chunks, engine) == arrays


@pytest.mark.parametrize("bs", ["BlockHasSize", "BlockMax256KB"])
def test_decompressCompressFrame_end_mark(slz4, engine, bs):                   # test/Main.hs:105-139, 234-243
    rng = random.Random(17)
    cfg = slz4.BlockConfig(getattr(slz4.BlockSize, bs))
    arrays = [gen_01(rng, 1, 50000, 0.1) for _ in range(12)]
    comp = b"".join(slz4.compressChunks(cfg, 1, arrays, engine)) + bytes(4)    # endMarkArr
    chunks = [comp[i:i + 4096] for i in range(0, len(comp), 4096)]
    got = slz4.decompressChunks(cfg, chunks, engine, slz4.FrameConfig(True))
    assert got == arrays


def test_decompressWithCompress_frame_header(slz4, engine):                    # test/Main.hs:141-187
    rng = random.Random(23)
    cfg = slz4.BlockConfig(slz4.BlockSize.BlockMax64KB)
    arrays = [gen_01(rng, 10 * 1024, 64 * 1024, 0.1) for _ in range(10)]
    hdr = bytes([0x04, 0x22, 0x4D, 0x18, 0x40, 0x40, 0x00])
    stream = hdr + b"".join(slz4.compressChunks(cfg, 1, arrays, engine)) + bytes(4)
    chunks = [stream[i:i + 1000] for i in range(0, len(stream), 1000)]
    assert slz4.decompressChunksWith(chunks, engine) == arrays


def test_mirror_errors(slz4, engine):
    cfg = slz4.BlockConfig(slz4.BlockSize.BlockMax64KB)
    with pytest.raises(slz4.LZ4Error, match="exceeds the maximum block size of 65536"):   # Internal/LZ4.hs:237-241
        slz4.compressChunks(cfg, 1, [bytes(65537)], engine)
    with pytest.raises(slz4.LZ4Error, match="compressed data length > 2GB"):              # Internal/LZ4.hs:309-310
        slz4.decompressChunksRaw(slz4.defaultBlockConfig, [bytes(12)], engine)
    good = slz4.compressChunks(slz4.defaultBlockConfig, 1, [b"hello world, hello world"], engine)[0]
    with pytest.raises(slz4.LZ4Error, match="input array data length"):                   # Internal/LZ4.hs:311-315
        slz4.decompressChunksRaw(slz4.defaultBlockConfig, [good + b"x"], engine)
    with pytest.raises(slz4.LZ4Error, match="input array data length"):                   # the case the reference misses
        slz4.decompressChunksRaw(slz4.defaultBlockConfig, [good[:-1]], engine)
    bad = bytearray(good)
    bad[8] = 0x1F                                                                           # corrupt the first token
    with pytest.raises(slz4.LZ4Error, match="c_decompressSafeContinue failed"):            # Internal/LZ4.hs:325-330
        slz4.decompressChunksRaw(slz4.defaultBlockConfig, [bytes(bad)], engine)


# --------------------------------------------------------------------------------------------
# device-resident path at BASELINE sizes: size-independent properties
# --------------------------------------------------------------------------------------------
def _roundtrip_device(slz4, engine, kind, nb, bl, accel):
    import torch
    dev = torch.device("cuda:0")
    src = torch.empty(nb * bl, dtype=torch.uint8, device=dev)
    engine.generate(kind, src, bl, nb)
    stride = slz4.slot_stride(bl, 8)
    slots = torch.empty(nb * stride, dtype=torch.uint8, device=dev)
    flen = torch.empty(nb, dtype=torch.int32, device=dev)
    doff = torch.empty(nb + 1, dtype=torch.int64, device=dev)
    engine.compress_batch_device(src, nb, bl, slots, stride, flen, accel=accel)
    engine.synchronize()
    total = int(flen.to(torch.int64).sum().item())
    dense = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    engine.compact_device(slots, stride, flen, nb, dense, total, doff)
    del slots
    ooff = torch.empty(nb + 1, dtype=torch.int64, device=dev)
    engine.index_device(dense, total, doff, nb, ooff)
    out = torch.empty(nb * bl, dtype=torch.uint8, device=dev)
    res = torch.empty(nb, dtype=torch.int32, device=dev)
    engine.decompress_batch_device(dense, total, doff, nb, out, ooff, res)
    engine.synchronize()
    assert int(doff[-1].item()) == total
    assert int(ooff[-1].item()) == nb * bl                                       # header chain self-consistent
    assert bool((res == bl).all().item())
    assert torch.equal(out, src)                                                 # encode -> decode identity
    return total, dense, doff


def test_roundtrip_config2_full_size(slz4, engine, oracle):
    """BASELINE config 2: 4 GiB lzsynth, 64 KiB blocks; identity round trip + spot checks vs the oracle."""
    nb, bl = 65536, 65536
    total, dense, doff = _roundtrip_device(slz4, engine, "lzsynth", nb, bl, 1)
    assert 2.7 < nb * bl / total < 3.1                                           # oracle-measured ratio 2.957
    # spot-check a few blocks of the GPU-written stream with the CPU oracle
    host_off = doff.cpu().numpy()
    for i in (0, 1, 777, 65535):
        blk = dense[int(host_off[i]):int(host_off[i + 1])].cpu().numpy().tobytes()
        code, out = oracle.decompress_block(blk[8:], bl)
        assert code == bl and out == oracle.gen("lzsynth", 1, bl, first_block=i).tobytes()


def test_roundtrip_config4_share_one_call_8GiB(slz4, engine, oracle):
    """BASELINE config 4's per-GPU share is 64 GiB / 8 = 8 GiB: 131 072 blocks of 64 KiB compressed, compacted and decoded
    in ONE call each -- more than 2^32 bytes of output behind one launch, which is also what the root's verification of
    the gathered stream decodes at N = 8 (bench.py).  Identity round trip + oracle spot checks either side of 2^32."""
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    if free < 40 * (1 << 30):
        pytest.skip("needs 40 GiB of free device memory")
    nb, bl = 131072, 65536
    total, dense, doff = _roundtrip_device(slz4, engine, "lzsynth", nb, bl, 1)
    assert 2.7 < nb * bl / total < 3.1
    host_off = doff.cpu().numpy()
    assert int(host_off[-1]) == total and nb * bl > (1 << 32)
    for i in (0, 65535, 65536, 131071):                                          # output offsets 0, 2^32 - 64 Ki, 2^32, 2^33 - 64 Ki
        blk = dense[int(host_off[i]):int(host_off[i + 1])].cpu().numpy().tobytes()
        code, out = oracle.decompress_block(blk[8:], bl)
        assert code == bl and out == oracle.gen("lzsynth", 1, bl, first_block=i).tobytes()


@pytest.mark.parametrize("kind", ["lzsynth", "text"])
def test_decode_config2_reference_written_256MiB(engine, oracle, kind):
    """BASELINE config 2 says "bit-exact vs ref": 256 MiB (4096 blocks of 64 KiB) of INDEPENDENT blocks written by the
    CPU oracle's compressor (byte-identical to the reference's, tests/test_oracle.py) go through both decoder kernels --
    the sequence-at-a-time one and the lane-parallel one -- and must give the generator's bytes back."""
    nb, bl = 4096, 65536
    data = oracle.gen(kind, nb, bl, first_block=1 << 20).tobytes()
    fr = oracle.frame_compress(data, bl, 1, 8, False)
    want = sha(data)
    try:
        for decoder in (1, 2, 4):
            engine.set_decoder(decoder)
            out, blen = engine.decompress_batch(fr)
            assert blen == [bl] * nb, (kind, decoder)
            assert sha(out) == want and out == data, (kind, decoder)
            del out
    finally:
        engine.set_decoder(0)


def test_roundtrip_config5_random_256k(slz4, engine):
    """BASELINE config 5: accel 400, incompressible input, 256 KiB blocks (4 GiB)."""
    nb, bl = 16384, 262144
    total, _, _ = _roundtrip_device(slz4, engine, "random", nb, bl, 400)
    assert total == nb * (263173 + 8)                                            # 263173 B per block


def test_roundtrip_text(slz4, engine):
    _roundtrip_device(slz4, engine, "text", 8192, 65536, 1)


# --------------------------------------------------------------------------------------------
# ragged batches and large blocks (reference edge cases: empty / ragged arrays, BlockMax4MB)
# --------------------------------------------------------------------------------------------
def test_ragged_batch_roundtrip(engine, oracle):
    rng = random.Random(77)
    blocks = []
    for i in range(120):
        kind = rng.choice(["lzsynth", "text", "random"])
        n = rng.choice([0, 1, 2, 11, 12, 13, 14, 100, 127, 128, 129, 1000, 4095, 4096, 65535, 65536, 65537, 200000])
        n = max(0, n + rng.randrange(-3, 4)) if n > 20 else n
        blocks.append(oracle.gen(kind, 1, max(n, 1), first_block=1000 + i)[:n].tobytes())
    fr, flen = engine.compress_batch(blocks, accel=1)
    # every block decodes standalone with the oracle, bit-exact
    pos = 0
    for b, f in zip(blocks, flen):
        assert int.from_bytes(fr[pos + 4:pos + 8], "little") == len(b)
        assert oracle.decompress_block(fr[pos + 8:pos + f], len(b)) == (len(b), b)
        pos += f
    # and the GPU decodes the whole ragged stream, every kernel
    for dec in (1, 2, 4):
        engine.set_decoder(dec)
        out, blen = engine.decompress_batch(fr)
        assert blen == [len(b) for b in blocks] and out == b"".join(blocks)
    engine.set_decoder(0)
    # GPU decodes the oracle's (reference algorithm's) stream of the same ragged blocks
    ofr = b"".join(len(c).to_bytes(4, "little") + len(b).to_bytes(4, "little") + c
                   for b, c in ((b, oracle.compress_block(b, 1)) for b in blocks))
    out, blen = engine.decompress_batch(ofr)
    assert out == b"".join(blocks)


@pytest.mark.parametrize("n,kind", [(4 << 20, "text"), (4 << 20, "lzsynth"), (16 << 20, "random"), ((16 << 20) + 5, "text")])
def test_large_blocks(slz4, engine, oracle, n, kind):
    """BlockMax4MB-sized and larger blocks (u32 hash table path, offsets capped at 65535)."""
    data = oracle.gen(kind, 1, n, first_block=5).tobytes()
    fr, flen = engine.compress_batch([data], accel=1)
    code, out = oracle.decompress_block(fr[8:], n)
    assert code == n and out == data
    out2, blen = engine.decompress_batch(fr)
    assert blen == [n] and out2 == data
    if n <= (4 << 20):
        cfg = slz4.BlockConfig(slz4.BlockSize.BlockMax4MB)
        comp = slz4.compressChunks(cfg, 1, [data], engine)
        assert slz4.decompressChunksRaw(cfg, comp, engine) == [data]
        with pytest.raises(slz4.LZ4Error, match="exceeds the maximum block size"):
            slz4.compressChunks(cfg, 1, [data + b"x"], engine)


def test_round_robin_generation_composes(engine):
    """Block k of the global stream lives on rank k % G: the per-rank generators (first=rank, step=G)
    interleave to exactly the single-GPU stream (what bench.py relies on for N > 1)."""
    import torch
    dev = torch.device("cuda:0")
    bl, nb, G = 4096, 24, 4
    whole = torch.empty(nb * bl, dtype=torch.uint8, device=dev)
    engine.generate("lzsynth", whole, bl, nb)
    parts = []
    for r in range(G):
        p = torch.empty(nb // G * bl, dtype=torch.uint8, device=dev)
        engine.generate("lzsynth", p, bl, nb // G, first_block=r, block_step=G)
        parts.append(p.view(nb // G, bl))
    engine.synchronize()
    inter = torch.stack(parts, dim=1).reshape(-1)          # local block j of rank g -> global block j*G+g
    assert torch.equal(inter, whole)


# --------------------------------------------------------------------------------------------
# many linked streams in one call: each stream is the reference compressor's
# own output (blocks linked to their predecessor), streams are independent of each other
# --------------------------------------------------------------------------------------------
def _stream_layout(frs, meta=8):
    """frs: framed bytes per stream -> (concatenated bytes, blockOff, streamFirst, uncompressed lengths)."""
    blob, boff, first, ulen = b"", [], [0], []
    for fr in frs:
        pos = 0
        while pos < len(fr):
            c = int.from_bytes(fr[pos:pos + 4], "little")
            boff.append(len(blob) + pos)
            ulen.append(int.from_bytes(fr[pos + 4:pos + 8], "little"))
            pos += meta + c
        blob += fr
        first.append(len(boff))
    return blob, boff, first, ulen


def _decode_streams(engine, frs, linked_mode):
    import torch
    dev = torch.device("cuda:0")
    blob, boff, first, ulen = _stream_layout(frs)
    nb = len(boff)
    buf = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    off = torch.tensor(boff, dtype=torch.int64, device=dev)
    ooff_h = np.concatenate([[0], np.cumsum(ulen)]).astype(np.int64)
    ooff = torch.from_numpy(ooff_h).to(dev)
    import guarded as G
    total = int(ooff_h[-1])
    out = G.new_torch(total + G.END_GUARD, 5, dev)                                # the tail holds tests/guarded.py's pattern ...
    out[:total] = 0
    res = torch.zeros(nb, dtype=torch.int32, device=dev)
    if linked_mode == "streams":
        sf = torch.tensor(first, dtype=torch.int32, device=dev)
        engine.decompress_streams_device(buf, len(blob), off, nb, sf, len(frs), out, ooff, res)
    else:
        engine.decompress_batch_device(buf, len(blob), off, nb, out, ooff, res, linked=(linked_mode == "one"))
    engine.synchronize()
    G.assert_confined(out, [(0, total)], 5, "_decode_streams(%s)" % linked_mode)  # ... and still does: nothing past the last block
    return out[:total].cpu().numpy().tobytes(), res.cpu().tolist(), ulen, first


# The second pass of a linked decode has three implementations behind one contract: byte source pointers +
# pointer jumping (csrc/linked_ptr.hpp), the in-order replay of deferred lists (csrc/linked_replay.hpp) and the
# exact decoder block after block.  The environment picks which ones a call may use and how many dependent
# blocks a segment holds, so that every path and every segment seam sees the same tests.
LINKED_VARIANTS = {
    "default": {},                                                 # runs of up to 4 dependent blocks: one wave per run (k_decode_fixup_runs)
    "runs_forced": {"MI355LZ4_LINKED_RUNS": "100000"},             # every run, however long, through the run walker
    "no_runs": {"MI355LZ4_LINKED_RUNS": "0"},                      # ... and never: short streams through the pointer pass
    "segments_of_3": {"MI355LZ4_LINKED_PTR": "1", "MI355LZ4_LINKED_POOL_BLOCKS": "3"},
    "pointer_pass_forced": {"MI355LZ4_LINKED_PTR": "1"},          # (many short streams would be walked otherwise)
    "pointer_segments_of_2": {"MI355LZ4_LINKED_PTR": "1", "MI355LZ4_LINKED_PTR_BLOCKS": "2"},
    "replay_only": {"MI355LZ4_LINKED_PTR": "0"},
    "replay_segments_of_2": {"MI355LZ4_LINKED_PTR": "0", "MI355LZ4_LINKED_POOL_BLOCKS": "2"},
    "serial_only": {"MI355LZ4_LINKED_POOL_BLOCKS": "0"},
    # no host wait: the second pass is enqueued over all blocks, gated on the device (mi355lz4_set_linked_async)
    "async": {"MI355LZ4_LINKED_ASYNC": "4194304"},
    "async_segments_of_3": {"MI355LZ4_LINKED_ASYNC": "4194304", "MI355LZ4_LINKED_PTR": "1", "MI355LZ4_LINKED_POOL_BLOCKS": "3"},
    # run-in decode (round 5; by default only for spans of 576 MiB and more): the default run-in (every piece starts at the
    # stream's first block in these short streams), and run-ins too short to arrive at the true dictionary -- pieces redone,
    # chained, with and without the wait inside a launch, calls given up for the pointer pass
    "runin": {"MI355LZ4_LINKED_RUNIN": "1", "MI355LZ4_LINKED_RUNS": "0"},
    "runin_1_pieces_of_1": {"MI355LZ4_LINKED_RUNIN": "1", "MI355LZ4_LINKED_RUNIN_BLOCKS": "1", "MI355LZ4_LINKED_RUNIN_PIECE": "1",
                            "MI355LZ4_LINKED_RUNS": "0"},
    "runin_2_pieces_of_2_no_wait": {"MI355LZ4_LINKED_RUNIN": "1", "MI355LZ4_LINKED_RUNIN_BLOCKS": "2", "MI355LZ4_LINKED_RUNIN_PIECE": "2",
                                    "MI355LZ4_LINKED_RUNIN_SPIN": "0", "MI355LZ4_LINKED_RUNS": "0"},
    "runin_1_pieces_of_3": {"MI355LZ4_LINKED_RUNIN": "1", "MI355LZ4_LINKED_RUNIN_BLOCKS": "1", "MI355LZ4_LINKED_RUNIN_PIECE": "3",
                            "MI355LZ4_LINKED_RUNS": "0"},
}


@pytest.fixture(params=list(LINKED_VARIANTS))
def linked_variant(request, monkeypatch):
    for k, v in LINKED_VARIANTS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def test_engine_written_linked_stream_all_linked_paths(engine, oracle, linked_variant):
    """A linked stream written by the ENGINE's linked compressor (deeper into its predecessors than the reference's: half of
    a text block's bytes derive from the block before it) through every linked decode path of LINKED_VARIANTS -- among them
    the run-in decode with run-ins too short for it -- and through the oracle's linked decoder: the input every time.
    Ragged and empty blocks included."""
    engine.set_linked_compress(True)
    try:
        for kind, bl, n in (("text", 65536, 30), ("text", 16384, 23), ("lzsynth", 65536, 14)):
            data = oracle.gen(kind, n, bl, first_block=41).tobytes()
            blocks = [data[i * bl:(i + 1) * bl] for i in range(n)]
            fr, flen = engine.compress_batch(blocks)
            assert oracle.frame_decompress(fr, n * bl, 8, 0, True) == data
            out, res, ulen, _ = _decode_streams(engine, [fr], "one")
            assert res == ulen == [bl] * n and out == data, (kind, bl)
        sizes = [65536, 1000, 65536, 0, 13, 12, 40000, 65536, 65536, 5, 65536, 30000]
        data = oracle.gen("text", 9, 65536, first_block=6).tobytes()
        blocks, pos = [], 0
        for sz in sizes:
            blocks.append(data[pos:pos + sz])
            pos += sz
        fr, flen = engine.compress_batch(blocks)
        out, blen = engine.decompress_batch(fr, linked=True)
        assert blen == sizes and out == data[:pos]
    finally:
        engine.set_linked_compress(False)


@pytest.mark.parametrize("decoder", [1, 2])
def test_linked_streams_many(engine, oracle, decoder, linked_variant):
    engine.set_decoder(decoder)
    try:
        rng = random.Random(7)
        datas, frs = [], []
        for s in range(24):
            bl = rng.choice([4096, 20000, 65536])
            nb = rng.randint(1, 6)
            kind = "text" if s % 3 else "lzsynth"
            d = oracle.gen(kind, nb, bl, first_block=100 * s).tobytes()
            if s % 4 == 1:                                   # periodic: matches that straddle the seam (:1883-1911)
                pat = d[:3001]
                d = (pat * (len(d) // len(pat) + 1))[: len(d)]
            datas.append(d)
            frs.append(oracle.frame_compress(d, bl, 1, 8, True))
        out, res, ulen, first = _decode_streams(engine, frs, "streams")
        assert res == ulen
        assert out == b"".join(datas)
        # the streams really are linked: decoded block by block they fail with the reference's codes ...
        out0, res0, _, _ = _decode_streams(engine, frs, "none")
        failing = [i for i, r in enumerate(res0) if r < 0]
        assert len(failing) > 10
        blocks = split_blocks(b"".join(frs))
        for i in failing[:20]:
            code, _ = oracle.decompress_block(blocks[i][8:], ulen[i])
            assert code == res0[i]
        # ... and treated as ONE stream, the first block of stream s > 0 that reaches back sees the wrong
        # predecessor, so the per-stream table is what keeps streams apart
        heads = set(first[:-1])
        assert all(i not in heads for i in failing)          # a stream's first block never needs a dictionary
    finally:
        engine.set_decoder(0)


def test_linked_streams_error_is_local(engine, oracle):
    """A corrupt block poisons only the rest of its own stream, with the reference's codes."""
    frs, datas = [], []
    for s in range(6):
        d = oracle.gen("text", 4, 16384, first_block=10 * s).tobytes()
        datas.append(d)
        frs.append(oracle.frame_compress(d, 16384, 1, 8, True))
    bad = bytearray(frs[2])
    blk = split_blocks(frs[2])
    pos = len(blk[0]) + 8                                    # first token of block 1 of stream 2
    bad[pos] = 0x1F                                          # 1 literal, then an offset that is almost surely wrong
    bad[pos + 2], bad[pos + 3] = 0xFF, 0xFF
    frs2 = list(frs)
    frs2[2] = bytes(bad)
    out, res, ulen, first = _decode_streams(engine, frs2, "streams")
    for s in range(6):
        lo, hi = first[s], first[s + 1]
        if s != 2:
            assert res[lo:hi] == ulen[lo:hi]
            o = sum(ulen[:lo])
            assert out[o:o + len(datas[s])] == datas[s]
    # reference behaviour for stream 2, block by block with the previous GOOD output as dictionary
    lo = first[2]
    dict_bytes = None
    for j, b in enumerate(split_blocks(frs2[2])):
        code, dec = oracle.decompress_block(b[8:], ulen[lo + j], dict_bytes)
        assert res[lo + j] == code, (j, res[lo + j], code)
        if code > 0:
            dict_bytes = dec


def test_linked_streams_fuzz_codes(engine, oracle, linked_variant):
    """Random single-byte corruptions anywhere in reference-linked streams: every block's result (size or
    negative code) and every decoded byte equals the oracle's linked decode of the same bytes."""
    rng = random.Random(2024)
    base = []
    for s in range(4):
        kind = ["text", "lzsynth", "text", "lzsynth"][s]
        bl = [8192, 16384, 65536, 4096][s]
        d = oracle.gen(kind, 3, bl, first_block=500 + 10 * s).tobytes()
        if s == 2:
            pat = d[:2500]
            d = (pat * (len(d) // len(pat) + 1))[: len(d)]
        base.append(oracle.frame_compress(d, bl, 1, 8, True))
    frs, expect = [], []
    for trial in range(120):
        fr = bytearray(base[trial % 4])
        blocks = split_blocks(bytes(fr))
        # corrupt one payload byte of block 1 or 2 (never a header: header errors are a separate test)
        bi = rng.choice([1, 2])
        start = sum(len(b) for b in blocks[:bi]) + 8
        pos = start + rng.randrange(len(blocks[bi]) - 8)
        fr[pos] ^= 1 << rng.randrange(8)
        frs.append(bytes(fr))
        # oracle: the reference's linked semantics, block by block
        dict_bytes, res, outs = None, [], []
        for b in split_blocks(bytes(fr)):
            cap = int.from_bytes(b[4:8], "little")
            code, dec = oracle.decompress_block(b[8:], cap, dict_bytes)
            res.append(code)
            outs.append(dec if code >= 0 else None)
            if code > 0:
                dict_bytes = dec
        expect.append((res, outs))
    out, res, ulen, first = _decode_streams(engine, frs, "streams")
    for t, (eres, eouts) in enumerate(expect):
        lo = first[t]
        assert res[lo:lo + 3] == eres, (t, res[lo:lo + 3], eres)
        for j in range(3):
            if eouts[j] is not None:
                o = sum(ulen[:lo + j])
                assert out[o:o + len(eouts[j])] == eouts[j], (t, j)


def test_single_linked_stream_fuzz_codes(engine, oracle, linked_variant):
    """ONE reference-linked stream per call (linked = 1: tolerant parallel pass + in-order replay,
    csrc/linked_replay.hpp) with corruptions of payload bytes: every block's result (size or the reference's
    negative code, cbits/lz4.c:2163) and every decoded byte equals the oracle's linked decode, block by block
    -- whether a block was replayed from its deferred list or went back to the exact serial decoder."""
    rng = random.Random(77)
    for trial in range(40):
        kind = ["text", "lzsynth", "text"][trial % 3]
        bl = [65536, 65536, 16384, 4096][trial % 4]
        nblk = rng.randint(3, 9)
        d = oracle.gen(kind, nblk, bl, first_block=900 + 13 * trial).tobytes()
        if trial % 5 == 2:                                   # periodic: matches that straddle the block seam
            pat = d[:2711]
            d = (pat * (len(d) // len(pat) + 1))[: len(d)]
        if trial % 7 == 3:                                   # shared vocabulary shifted by whole blocks: long far matches
            d = d[:bl] * nblk
        fr = bytearray(oracle.frame_compress(d, bl, 1, 8, True))
        blocks = split_blocks(bytes(fr))
        for _ in range(rng.choice([0, 1, 1, 2, 4])):
            bi = rng.randrange(1, len(blocks))
            start = sum(len(b) for b in blocks[:bi]) + 8
            pos = start + rng.randrange(len(blocks[bi]) - 8)
            fr[pos] = rng.randrange(256) if rng.random() < 0.5 else fr[pos] ^ (1 << rng.randrange(8))
        dict_bytes, eres, eouts = None, [], []
        for b in split_blocks(bytes(fr)):
            cap = int.from_bytes(b[4:8], "little")
            code, dec = oracle.decompress_block(b[8:], cap, dict_bytes)
            eres.append(code)
            eouts.append(dec if code >= 0 else None)
            if code > 0:
                dict_bytes = dec
        out, res, ulen, first = _decode_streams(engine, [bytes(fr)], "one")
        assert res == eres, (trial, res, eres)
        o = 0
        for j, e in enumerate(eouts):
            if e is not None:
                assert out[o:o + len(e)] == e, (trial, j)
            o += ulen[j]


@pytest.mark.parametrize("bl", [262144, 1 << 20, 4 << 20, (4 << 20) + 65536])
def test_single_linked_stream_large_blocks(engine, oracle, linked_variant, bl):
    """Linked streams with blocks above 64 KiB (BlockMax256KB .. BlockMax4MB, or big arrays under BlockHasSize): a
    block of up to 4 MiB takes as many list regions and pointers as it has 64 KiB pieces; beyond that it is walked.
    Clean and corrupted, against the oracle's linked decode."""
    rng = random.Random(bl)
    nblk = 5 if bl <= (1 << 20) else 3
    raw = oracle.gen("text", (nblk * bl + 65535) // 65536, 65536, first_block=21).tobytes()[: nblk * bl]
    for trial in range(3):
        fr = bytearray(oracle.frame_compress(raw, bl, 1, 8, True))
        blocks = split_blocks(bytes(fr))
        if trial:
            bi = rng.randrange(1, len(blocks))
            start = sum(len(b) for b in blocks[:bi]) + 8
            pos = start + rng.randrange(len(blocks[bi]) - 8)
            fr[pos] ^= 1 << rng.randrange(8)
        dict_bytes, eres, eouts = None, [], []
        for b in split_blocks(bytes(fr)):
            code, dec = oracle.decompress_block(b[8:], int.from_bytes(b[4:8], "little"), dict_bytes)
            eres.append(code)
            eouts.append(dec if code >= 0 else None)
            if code > 0:
                dict_bytes = dec
        out, res, ulen, _ = _decode_streams(engine, [bytes(fr)], "one")
        assert res == eres, (bl, trial, res, eres)
        o = 0
        for j, e in enumerate(eouts):
            if e is not None:
                assert out[o:o + len(e)] == e, (bl, trial, j)
            o += ulen[j]


def test_single_linked_stream_deep_chains(engine, oracle, linked_variant):
    """Streams in which a byte's origin lies arbitrarily far back: runs (every byte copies the one before it, across
    every block seam: a chain as deep as the stream is long), short and long periods, a period longer than a block.
    The pointer pass resolves a chain of depth d in log(d) passes; the other paths walk it."""
    bl = 65536
    cases = {
        "zeros": bytes(40 * bl),
        "period 3": (b"abc" * (14 * bl // 3 + 1))[: 14 * bl],
        "period 70001": (oracle.gen("text", 2, bl, first_block=9).tobytes()[:70001] * 12)[: 11 * bl],
        # every block is made of the block before it, noise otherwise: a run-in never arrives at the true dictionary, every
        # piece would have to be redone behind the one in front (the run-in decode gives such a call up: k_runin_fix)
        "period 60000 of noise": (random.Random(5).randbytes(60000) * 45)[: 40 * bl],
        "runs in text": b"".join(oracle.gen("text", 1, bl, first_block=i).tobytes()[:3000] + bytes([65 + i]) * 20000 for i in range(30)),
    }
    for name, d in cases.items():
        d = d[: len(d) // bl * bl]
        fr = oracle.frame_compress(d, bl, 1, 8, True)
        out, res, ulen, _ = _decode_streams(engine, [fr], "one")
        assert res == ulen and out == d, name
        # the same stream as two streams of a multi-stream call (the second starts without a dictionary)
        out, res, ulen, _ = _decode_streams(engine, [fr, fr], "streams")
        assert res == ulen and out == d + d, name


def test_streams_call_without_streams_decodes_every_block(engine, oracle):
    """nStreams = 0: every block lies outside every stream and is decoded on its own."""
    import torch
    dev = torch.device("cuda:0")
    d = oracle.gen("lzsynth", 5, 16384, first_block=2).tobytes()
    fr = oracle.frame_compress(d, 16384, 1, 8, False)
    blob, boff, first, ulen = _stream_layout([fr])
    buf = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    off = torch.tensor(boff, dtype=torch.int64, device=dev)
    ooff = torch.arange(6, dtype=torch.int64, device=dev) * 16384
    out = torch.zeros(5 * 16384, dtype=torch.uint8, device=dev)
    res = torch.zeros(5, dtype=torch.int32, device=dev)
    sf = torch.zeros(1, dtype=torch.int32, device=dev)
    engine.decompress_streams_device(buf, len(blob), off, 5, sf, 0, out, ooff, res)
    engine.synchronize()
    assert res.cpu().tolist() == [16384] * 5 and out.cpu().numpy().tobytes() == d


def test_linked_streams_host_api(engine, oracle):
    """mi355lz4_decompress_streams (host buffers) == the device entry point == the raw data."""
    datas, frs = [], []
    for s in range(9):
        d = oracle.gen("text", 1 + s % 4, 16384, first_block=40 * s).tobytes()
        datas.append(d)
        frs.append(oracle.frame_compress(d, 16384, 1, 8, True))
    blob, boff, first, ulen = _stream_layout(frs)
    out, blen = engine.decompress_streams(blob, first)
    assert blen == ulen and out == b"".join(datas)
    # the table is checked
    import streamly_lz4_amd as S
    with pytest.raises(S.LZ4Error):
        engine.decompress_streams(blob, [0, 5, 3])
    with pytest.raises(S.LZ4Error):
        engine.decompress_streams(blob, [0, len(boff) + 1])


def test_decompress_chunks_batch_form(engine, oracle, slz4):
    """decompressChunks over arrays that lie back to back takes one index walk and one GPU call (decompressChunksBatch,
    include/streamly_lz4.hpp); its results -- as bytes or as views into one buffer -- and its errors are those of the
    array-at-a-time combinators (resizeChunksD + decompressChunksRawD, Internal/LZ4.hs:432-567)."""
    S = slz4
    cfg = S.defaultBlockConfig
    raw = oracle.gen("text", 37, 65536).tobytes() + oracle.gen("lzsynth", 1, 1234).tobytes()
    framed = oracle.frame_compress(raw, 65536, 1, 8, True)                     # the reference's linked stream
    for split in (1 << 30, 65536, 5000, 7):
        chunks = [framed[i:i + split] for i in range(0, len(framed), split)] if split < len(framed) else [framed]
        if split == 7:
            chunks = chunks[:2000] + [b"".join(chunks[2000:])]
        out_b = S.decompressChunks(cfg, chunks, engine)
        out_v = S.decompressChunks(cfg, chunks, engine, views=True)
        assert b"".join(out_b) == raw and [len(a) for a in out_b] == [65536] * 37 + [1234]
        assert [bytes(v) for v in out_v] == out_b
    two_step = S.decompressChunksRaw(cfg, S.resizeChunks(cfg, S.defaultFrameConfig, [framed]), engine)
    assert two_step == S.decompressChunks(cfg, [framed], engine)
    assert S.decompressChunks(cfg, [], engine) == []
    # errors: whatever the batch form cannot take goes through the combinators and raises what they raise
    def err(arrays):
        try:
            S.decompressChunks(cfg, arrays, engine)
        except S.LZ4Error as e:
            return str(e)
        return None
    def err2(arrays):
        try:
            S.decompressChunksRaw(cfg, S.resizeChunks(cfg, S.defaultFrameConfig, arrays), engine)
        except S.LZ4Error as e:
            return str(e)
        return None
    damaged = bytearray(framed); damaged[20000] ^= 0xFF; damaged[20001] ^= 0xFF; damaged[20002] ^= 0x55
    for bad in ([framed[:-5]], [framed + b"\x01"], [framed[:8]]):             # one thing wrong: the same message
        assert err(bad) == err2(bad) and err(bad) is not None
    # several things wrong: the fused stream reports the first in stream order (err2 resizes everything first)
    for bad in ([bytes(damaged)], [b"\x00\x00\x00\x00" + framed], [bytes(damaged[:-3])]):
        assert err(bad) is not None
