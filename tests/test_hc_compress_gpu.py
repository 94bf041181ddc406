"""Compression levels 1..12 on the GPU (mi355lz4_set_compression_level; csrc/encode_hc.hpp): round trips through the
oracle, the reference and every GPU decoder; the LZ4 format rules of every block written; linked compression; ratios
against level 0 and liblz4's LZ4_compress_HC; determinism; level 0 left byte-identical; frames and the mirrors."""
import ctypes as C
import ctypes.util
import glob
import os
import struct
import sys
import sysconfig

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from conftest import DECODERS  # noqa: E402
import lz4f  # noqa: E402
from lz4_check import check_block  # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG = -3
LENGTHS = [0, 1, 12, 13, 14, 4095, 65535, 65536, 256 << 10, 1 << 20, 4 << 20]
KINDS = ["text", "lzsynth", "random", "zero"]


@pytest.fixture(scope="module")
def ref_codec():
    """The reference codec built under oracle/_ref, or None where it was not built."""
    from oracle.oracle import Reference
    try:
        return Reference()
    except (OSError, FileNotFoundError):
        return None


@pytest.fixture
def hc(slz4):
    eng = slz4.Engine(0)
    yield eng
    eng.close()


def _data(oracle, kind, n, seed=0):
    if n == 0:
        return b""
    if kind == "zero":
        return bytes(n)
    bl = min(n, 65536)
    nb = (n + bl - 1) // bl
    return oracle.gen(kind, nb, bl, first_block=seed).tobytes()[:n]


def _split(framed, hk, ck):
    """[(compressed data, uncompLen or None)] of a dense framed stream."""
    out, pos = [], 0
    while pos < len(framed):
        cl = struct.unpack_from("<i", framed, pos)[0]
        ul = struct.unpack_from("<i", framed, pos + 4)[0] if hk == 8 else None
        out.append((framed[pos + hk:pos + hk + cl], ul))
        pos += hk + cl + (4 if ck else 0)
    assert pos == len(framed)
    return out


def _walk(block, n, dict_len=0):
    """Checks the LZ4 format rules of one block that decodes to n bytes; returns (sequences, matches reaching into the
    dictionary)."""
    i, pos, seqs, into_dict = 0, 0, 0, 0
    while True:
        tok = block[i]
        i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = block[i]
                i += 1
                lit += b
                if b != 255:
                    break
        i += lit
        pos += lit
        if i == len(block):
            break
        off = block[i] | (block[i + 1] << 8)
        i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = block[i]
                i += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        assert 1 <= off <= 65535 and off <= pos + dict_len, "offset %d at %d" % (off, pos)
        assert pos <= n - 13, "a match starts within the last 12 bytes (%d of %d)" % (pos, n)
        assert pos + ml <= n - 5, "the last 5 bytes are not literals"
        into_dict += off > pos
        pos += ml
        seqs += 1
    assert pos == n
    if n < 13:
        assert seqs == 0
    strict = check_block(block, n, dict_len)       # the strict validator too: bounds, the last token, compressBound
    assert (strict[0], strict[3]) == (seqs, into_dict)
    return seqs, into_dict


def _hc_compress(eng, blocks, level, hk=8, ck=False, linked=False):
    eng.set_compression_level(level)
    eng.set_block_checksum(ck)
    eng.set_linked_compress(linked)
    return eng.compress_batch(blocks, accel=1, header_kind=hk)


# ---- 0. the setter ------------------------------------------------------------------------------------------
def test_levels_set_and_get(hc, slz4):
    assert hc.compression_level == 0
    for lv in range(10):
        hc.set_compression_level(lv)
        assert hc.compression_level == lv
    for lv in (10, 11, 12):
        hc.set_compression_level(lv)
        assert hc.compression_level == 9
    for lv in (-1, 13, 100):
        assert slz4.lib.mi355lz4_set_compression_level(hc.ctx, lv) == E_ARG
        assert hc.compression_level == 9
    hc.set_compression_level(0)
    assert hc.compression_level == 0


# ---- 1. + 2. round trip and format rules ----------------------------------------------------------------------
@pytest.mark.parametrize("level,hk,ck", [(1, 8, False), (3, 4, True), (6, 8, True), (9, 4, False), (9, 8, False),
                                         (9, 4, True), (9, 8, True), (12, 8, False)])
@pytest.mark.parametrize("n", LENGTHS)
def test_round_trip(hc, slz4, oracle, ref_codec, level, hk, ck, n):
    blocks = [_data(oracle, k, n, seed=3) for k in KINDS]
    framed, flen = _hc_compress(hc, blocks, level, hk, ck)
    parts = _split(framed, hk, ck)
    assert len(parts) == len(blocks)
    for (comp, ul), raw in zip(parts, blocks):
        if hk == 8:
            assert ul == n
        assert len(comp) <= slz4.compress_bound(n)
        if level in (3, 9) or n <= (1 << 20):
            _walk(comp, n)
        if n == 0:
            continue
        r, got = oracle.decompress_block(comp, n)
        assert r == n and got == raw, "oracle"
        if ref_codec is not None:
            r, got = ref_codec.decompress_block(comp, n)
            assert r == n and got == raw, "reference"
    want = b"".join(blocks)
    for d in DECODERS:
        hc.set_decoder(d)
        out, blen = hc.decompress_batch(framed, header_kind=hk, fixed_uncomp=n)
        assert blen == [n] * len(blocks) and out == want, "decoder %d" % d
    hc.set_decoder(0)
    out, _ = hc.decompress_batch(framed, header_kind=hk, fixed_uncomp=n)
    assert out == want, "decoder 0"


def test_device_call_every_small_length(hc, slz4, oracle):
    """Blocks of every length 0..300 and some ragged big ones in ONE device call (srcOff / srcLen per block)."""
    import torch
    hc.set_compression_level(9)
    lens = list(range(301)) + [65537, 100_003, 131_072, 70_001]
    raw = [_data(oracle, "text", L, seed=L) for L in lens]
    offs = np.cumsum([0] + lens[:-1]).astype(np.uint64)
    src = torch.from_numpy(np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8).copy()).cuda()
    stride = slz4.slot_stride(max(lens), 8)
    slots = torch.zeros(len(lens) * stride, dtype=torch.uint8, device="cuda:0")
    flen = torch.zeros(len(lens), dtype=torch.int32, device="cuda:0")
    so = torch.from_numpy(offs.view(np.int64)).cuda()
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda:0")
    rc = slz4.lib.mi355lz4_compress_batch_device(hc.ctx, C.c_void_p(src.data_ptr()), C.c_void_p(so.data_ptr()),
                                                 C.c_void_p(sl.data_ptr()), C.c_uint64(0), max(lens), len(lens), 1, 8,
                                                 C.c_void_p(slots.data_ptr()), C.c_size_t(stride),
                                                 C.c_void_p(flen.data_ptr()))
    assert rc == 0
    hc.synchronize()
    sb, fl = slots.cpu().numpy().tobytes(), flen.cpu().numpy().tolist()
    for i, L in enumerate(lens):
        blk = sb[i * stride:i * stride + fl[i]]
        cl, ul = struct.unpack_from("<ii", blk, 0)
        assert ul == L and cl + 8 == fl[i]
        _walk(blk[8:], L)
        if L:
            r, got = oracle.decompress_block(blk[8:], L)
            assert r == L and got == raw[i]


# ---- 3. linked ------------------------------------------------------------------------------------------------
def _decode_linked_oracle(oracle, parts, blocks):
    prev = None
    for (comp, _ul), raw in zip(parts, blocks):
        r, got = oracle.decompress_block(comp, len(raw), dict_bytes=prev[-65536:] if prev else None)
        assert r == len(raw) and got == raw
        prev = raw


@pytest.mark.parametrize("bl,n", [(65536, 64), (200_000, 12), (1 << 20, 4)])
def test_linked(hc, slz4, oracle, bl, n):
    raw = _data(oracle, "text", bl * n, seed=11)
    blocks = [raw[i * bl:(i + 1) * bl] for i in range(n)]
    framed, _ = _hc_compress(hc, blocks, 9, linked=True)
    parts = _split(framed, 8, False)
    into = 0
    for i, ((comp, _ul), b) in enumerate(zip(parts, blocks)):
        into += _walk(comp, len(b), dict_len=0 if i == 0 else min(65536, bl))[1]
    assert into > 0, "no match reaches into the previous block"
    _decode_linked_oracle(oracle, parts, blocks)
    for d in DECODERS:
        hc.set_decoder(d)
        out, blen = hc.decompress_batch(framed, linked=True)
        assert out == raw and blen == [bl] * n, "decoder %d" % d
    hc.set_decoder(0)
    indep, _ = _hc_compress(hc, blocks, 9, linked=False)
    assert len(framed) < len(indep)


def test_linked_multi_group_host_call(hc, oracle):
    """More than 64 MiB in one host call: the second group's first block takes its dictionary across the seam."""
    bl, n = 65536, 1100
    raw = _data(oracle, "lzsynth", bl * n, seed=5)
    blocks = [raw[i * bl:(i + 1) * bl] for i in range(n)]
    framed, _ = _hc_compress(hc, blocks, 6, linked=True)
    parts = _split(framed, 8, False)
    _decode_linked_oracle(oracle, parts, blocks)
    seam = 1024                                   # 64 MiB / 64 KiB: the first block of the second group
    assert _walk(parts[seam][0], bl, dict_len=bl)[1] > 0
    out, _ = hc.decompress_batch(framed, linked=True)
    assert out == raw


# ---- 4. ratio ------------------------------------------------------------------------------------------------
def _liblz4_hc():
    for name in ("liblz4.so.1", ctypes.util.find_library("lz4")):
        if not name:
            continue
        try:
            L = C.CDLL(name)
        except OSError:
            continue
        if hasattr(L, "LZ4_compress_HC"):
            L.LZ4_compress_HC.restype = C.c_int
            L.LZ4_compress_HC.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
            return L
    return None


def _python_sources(limit=16 << 20):
    files = sorted(glob.glob(os.path.join(sysconfig.get_paths()["stdlib"], "**", "*.py"), recursive=True))
    out, size = [], 0
    for f in files:
        try:
            b = open(f, "rb").read()
        except OSError:
            continue
        out.append(b)
        size += len(b)
        if size >= limit:
            break
    return b"".join(out)[:limit]


def _corpus(oracle, name):
    bl = 65536
    if name == "python":
        raw = _python_sources()
        raw = raw[:len(raw) // bl * bl]
        assert len(raw) >= 4 << 20
    else:
        raw = oracle.gen(name, 256, bl).tobytes()
    return [raw[i:i + bl] for i in range(0, len(raw), bl)]


@pytest.mark.parametrize("name,vs_level0", [("text", 0.92), ("lzsynth", 0.88), ("python", 0.82)])
def test_ratio(hc, oracle, record, name, vs_level0):
    blocks = _corpus(oracle, name)
    tot = {}
    for lv in (0, 1, 5, 9):
        framed, _ = _hc_compress(hc, blocks, lv)
        tot[lv] = len(framed) - 8 * len(blocks)
    assert tot[9] <= tot[5] <= tot[1]
    assert tot[9] <= vs_level0 * tot[0], tot
    L = _liblz4_hc()
    rec = {"level%d" % k: v for k, v in tot.items()}
    if L is not None:
        dst = C.create_string_buffer(65536 + 65536 // 255 + 16)
        ref = 0
        for b in blocks:
            r = L.LZ4_compress_HC(b, dst, len(b), len(dst), 9)
            assert r > 0
            ref += r
        rec["liblz4_hc9"] = ref
        assert tot[9] <= 1.03 * ref, (tot[9], ref)
    record("hc_ratio_" + name, rec)


def test_ratio_random(hc, oracle):
    blocks = _corpus(oracle, "random")[:64]
    f0, _ = _hc_compress(hc, blocks, 0)
    f9, _ = _hc_compress(hc, blocks, 9)
    assert len(f9) <= 1.001 * len(f0)


# ---- 5. determinism ---------------------------------------------------------------------------------------------
def _dev_compress(eng, slz4, src, bl, n):
    import torch
    stride = slz4.slot_stride(bl, 8)
    slots = torch.zeros(n * stride, dtype=torch.uint8, device="cuda:0")
    flen = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    eng.compress_batch_device(src, n, bl, slots, stride, flen, header_kind=8)
    eng.synchronize()
    fl = flen.cpu().numpy().tolist()
    sb = slots.cpu().numpy().tobytes()
    return [sb[i * stride:i * stride + fl[i]] for i in range(n)]


def test_deterministic(hc, slz4):
    import torch
    bl, n = 65536, 4096
    src = torch.empty(n * bl, dtype=torch.uint8, device="cuda:0")
    hc.generate("text", src, bl, n)
    hc.synchronize()
    hc.set_compression_level(9)
    a = _dev_compress(hc, slz4, src, bl, n)
    b = _dev_compress(hc, slz4, src, bl, n)
    assert a == b
    for k in (0, 1777, n - 1):
        alone = _dev_compress(hc, slz4, src[k * bl:(k + 1) * bl], bl, 1)
        assert alone[0] == a[k]
    s = torch.cuda.Stream()
    hc.use_stream(s.cuda_stream)
    c = _dev_compress(hc, slz4, src[:256 * bl], bl, 256)
    assert c == a[:256]


# ---- 6. level 0 unchanged ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bl,n", [(65536, 16), (256 << 10, 16), (65536, 600)])
@pytest.mark.parametrize("linked", [False, True])
def test_level0_unchanged(slz4, oracle, bl, n, linked):
    raw = _data(oracle, "text", bl * n, seed=2)
    blocks = [raw[i * bl:(i + 1) * bl] for i in range(n)]
    fresh = slz4.Engine(0)
    fresh.set_linked_compress(linked)
    want = fresh.compress_batch(blocks, accel=3)
    fresh.close()
    eng = slz4.Engine(0)
    eng.set_linked_compress(linked)
    eng.set_compression_level(9)
    hc9 = eng.compress_batch(blocks, accel=3)
    eng.set_compression_level(0)
    assert eng.compress_batch(blocks, accel=3) == want
    assert hc9 != want
    eng.close()


# ---- 7. frames and mirrors -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("linked", [False, True])
def test_frame(hc, slz4, oracle, linked):
    data = _data(oracle, "text", 3_000_007, seed=9)
    hc.set_compression_level(9)
    frame = slz4.lz4FrameCompress(data, hc, blockMax=slz4.BlockSize.BlockMax256KB, linkedBlocks=linked, blockChecksum=True)
    assert slz4.lz4FrameDecompress(frame, hc) == data
    hc.set_compression_level(0)
    fast = slz4.lz4FrameCompress(data, hc, blockMax=slz4.BlockSize.BlockMax256KB, linkedBlocks=linked, blockChecksum=True)
    assert frame[:7] == fast[:7] and len(frame) < len(fast)
    L = lz4f.load()
    if L is None:
        pytest.skip("liblz4 with LZ4F_* not found")
    assert lz4f.decompress(L, frame, len(data) + 16) == data


def test_compress_chunks(hc, slz4, oracle):
    bl, n = 65536, 40
    raw = _data(oracle, "lzsynth", bl * n, seed=4)
    cfg = slz4.BlockConfig(slz4.BlockSize.BlockMax64KB)
    hc.set_compression_level(0)
    fast = slz4.compressChunks(cfg, 1, [raw[i * bl:(i + 1) * bl] for i in range(n)], hc)
    hc.set_compression_level(7)
    chunks = slz4.compressChunks(cfg, 1, [raw[i * bl:(i + 1) * bl] for i in range(n)], hc)
    assert b"".join(slz4.decompressChunks(cfg, chunks, hc)) == raw
    assert sum(len(c) for c in chunks) < sum(len(c) for c in fast)


def test_multi_engine_levels_must_agree(slz4, oracle):
    m = slz4.MultiEngine([0, 0])
    blocks = [_data(oracle, "text", 65536, seed=i) for i in range(8)]
    fast, _ = m.compress_batch(blocks)
    m.set_compression_level(9)
    framed, _ = m.compress_batch(blocks)
    assert len(framed) < len(fast)
    out, _ = m.decompress_batch(framed)
    assert out == b"".join(blocks)
    slz4.lib.mi355lz4_multi_engine.restype = C.c_void_p
    e1 = C.c_void_p(slz4.lib.mi355lz4_multi_engine(m._h, 1))
    assert slz4.lib.mi355lz4_set_compression_level(e1, 3) == 0
    with pytest.raises(slz4.LZ4Error, match="compression level"):
        m.compress_batch(blocks)
    m.close()
