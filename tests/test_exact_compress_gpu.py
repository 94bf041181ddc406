"""Reference-exact compression (mi355lz4_set_compress_exact): the engine's compress calls continue ONE stream whose bytes
are LZ4_compress_fast_continue's over separately allocated arrays.  The reference here is the oracle's compress stream
(orc_cstream_init once, orc_compress_fast_continue per array, each array its own allocation), driven through ctypes, and
-- where oracle/_ref was built -- the reference's own framing (Reference.frame_compress, linked)."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from conftest import DECODERS  # noqa: E402
from oracle.oracle import Oracle, build as oracle_build  # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG = -3
_u8p = C.POINTER(C.c_uint8)
HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "liblz4ref.so"))


class OracleStream:
    """orc_cstream over separately allocated arrays: the reference's compressChunksD call sequence."""

    def __init__(self):
        self.lib = C.CDLL(oracle_build(), mode=os.RTLD_LOCAL)
        self.lib.orc_compress_fast_continue.restype = C.c_int
        self.lib.orc_compress_fast_continue.argtypes = [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int]
        self.lib.orc_compress_bound.restype = C.c_int
        self.lib.orc_compress_bound.argtypes = [C.c_int]
        self.lib.orc_debug_renorms.restype = C.c_long
        self.reset()

    def reset(self):
        self.st = C.create_string_buffer(16384 + 256)
        self.lib.orc_cstream_init(self.st)
        self.keep = []

    def compress(self, arrays, accel=1):
        if accel < 0:
            accel = 0                                  # speed = max speed0 0 (Internal/LZ4.hs:364)
        out = []
        for a in arrays:
            src = np.zeros(len(a) + 64, dtype=np.uint8)  # its own allocation, readable slack behind it
            src[: len(a)] = np.frombuffer(bytes(a), dtype=np.uint8)
            cap = self.lib.orc_compress_bound(len(a))
            dst = np.zeros(cap + 64, dtype=np.uint8)
            r = self.lib.orc_compress_fast_continue(self.st, src.ctypes.data_as(_u8p), dst.ctypes.data_as(_u8p), len(a),
                                                    cap, int(accel))
            assert r > 0
            out.append(dst[:r].tobytes())
            self.keep = self.keep[-1:] + [src]      # the previous array stays alive: it is the dictionary
        return out


def frame(comps, arrays, kind, checksum=False):
    """The engine's framing of the blocks: | compLen | uncompLen (kind 8) | data | xxh32 (checksums) |."""
    import streamly_lz4_amd as S
    out = bytearray()
    for c, a in zip(comps, arrays):
        out += len(c).to_bytes(4, "little")
        if kind == 8:
            out += len(a).to_bytes(4, "little")
        out += c
        if checksum:
            out += int(S.lib.slz4_xxh32(np.frombuffer(c, dtype=np.uint8).ctypes.data_as(_u8p), len(c), 0)).to_bytes(4, "little")
    return bytes(out)


_ORC = None


def orc():
    global _ORC
    if _ORC is None:
        _ORC = Oracle()
    return _ORC


def data(kind, n_blocks, block_len, first=0):
    if kind == "zeros":
        return bytes(n_blocks * block_len)
    if kind == "pysrc":
        files = sorted(glob.glob(os.path.join(os.path.dirname(os.__file__), "*.py")))
        buf = bytearray()
        for f in files:
            buf += open(f, "rb").read()
            if len(buf) >= n_blocks * block_len:
                break
        while len(buf) < n_blocks * block_len:
            buf = buf + buf
        return bytes(buf[: n_blocks * block_len])
    return orc().gen(kind, n_blocks, block_len, first_block=first).tobytes()


def split(raw, block_len):
    return [raw[i:i + block_len] for i in range(0, len(raw), block_len)]


def ragged(seed=7):
    rng = np.random.default_rng(seed)
    lens = [0, 1, 3, 4, 5, 12, 13, 4095, 65535, 65536, 65537, 200000]
    lens = lens + [int(x) for x in rng.permutation(lens)] + [0, 0, 2, 65536]
    raw = data("text", 1, sum(lens) + 16, first=seed) if seed % 2 else data("pysrc", 1, sum(lens) + 16)
    out, p = [], 0
    for n in lens:
        out.append(raw[p:p + n])
        p += n
    return out


def gpu_host(eng, arrays, accel=1, kind=8):
    framed, flen = eng.compress_batch(arrays, accel=accel, header_kind=kind)
    return framed, flen


def gpu_device(eng, arrays, accel=1, kind=8, gap=37):
    """compress_batch_device with the arrays NOT back to back (gap bytes between them): placement must not matter."""
    import torch
    import streamly_lz4_amd as S
    offs, p = [], 0
    for a in arrays:
        offs.append(p)
        p += len(a) + gap
    buf = np.zeros(p + 16, dtype=np.uint8)
    for o, a in zip(offs, arrays):
        buf[o:o + len(a)] = np.frombuffer(bytes(a), dtype=np.uint8)
    n = len(arrays)
    mx = max(len(a) for a in arrays)
    stride = S.slot_stride_ex(mx, kind, eng._block_checksum)
    src = torch.from_numpy(buf).cuda()
    off = torch.tensor(offs, dtype=torch.int64).cuda()
    ln = torch.tensor([len(a) for a in arrays], dtype=torch.int32).cuda()
    slots = torch.zeros(n * stride, dtype=torch.uint8).cuda()
    flen = torch.zeros(n, dtype=torch.int32).cuda()
    eng.compress_batch_device(src, n, mx, slots, stride, flen, accel=accel, header_kind=kind, src_off=off, src_len=ln,
                              block_stride=0)
    torch.cuda.synchronize()
    sl = slots.cpu().numpy()
    fl = flen.cpu().tolist()
    return b"".join(sl[i * stride:i * stride + fl[i]].tobytes() for i in range(n)), fl


@pytest.fixture
def engine():
    import streamly_lz4_amd as S
    e = S.Engine(0)
    e.set_compress_exact(True)
    yield e
    e.close()


def expect(arrays, accel=1, kind=8, checksum=False):
    return frame(OracleStream().compress(arrays, accel), arrays, kind, checksum)


# ---- 1. byte equality ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["text", "lzsynth", "random", "zeros", "pysrc"])
@pytest.mark.parametrize("block_len,n", [(65536, 24), (262144, 6), (1 << 20, 3), (4 << 20, 2)])
def test_uniform_blocks_equal_oracle(engine, kind, block_len, n):
    arrays = split(data(kind, n, block_len), block_len)
    want = expect(arrays)
    got, _ = gpu_host(engine, arrays)
    assert got == want
    engine.reset_compress_stream()
    got, _ = gpu_device(engine, arrays)
    assert got == want


@pytest.mark.parametrize("accel", [-3, 0, 1, 2, 9, 65537, 10 ** 6])
def test_accel_and_ragged_lengths(engine, accel):
    arrays = ragged(accel & 7 | 1)
    want = expect(arrays, accel)
    got, _ = gpu_host(engine, arrays, accel=accel)
    assert got == want
    engine.reset_compress_stream()
    got, _ = gpu_device(engine, arrays, accel=accel)
    assert got == want


@pytest.mark.parametrize("hk", [4, 8])
@pytest.mark.parametrize("checksum", [False, True])
def test_header_kinds_and_checksums(engine, hk, checksum):
    arrays = split(data("text", 12, 65536, first=5), 65536) if hk == 4 else ragged(3)
    engine.set_block_checksum(checksum)
    want = expect(arrays, 1, hk, checksum)
    got, _ = gpu_host(engine, arrays, kind=hk)
    assert got == want
    engine.reset_compress_stream()
    got, _ = gpu_device(engine, arrays, kind=hk)
    assert got == want


def test_compress_chunks_equals_reference(engine):
    import streamly_lz4_amd as S
    arrays = ragged(5)
    want = OracleStream().compress(arrays)
    for _ in range(2):                         # compressChunks starts a new stream each time
        got = S.compressChunks(S.BlockConfig(), 1, arrays, engine)
        assert [bytes(g)[8:] for g in got] == want
    engine.set_batch_blocks(5)                 # the stream continues across compressChunks' batches
    got = S.compressChunks(S.BlockConfig(), 1, arrays, engine)
    assert [bytes(g)[8:] for g in got] == want
    if HAVE_REF:
        from oracle.oracle import Reference
        raw = data("text", 20, 65536, first=9)
        arrays = split(raw, 65536)
        ref = Reference().frame_compress(raw, 65536, 1, 8, True)
        assert b"".join(bytes(g) for g in S.compressChunks(S.BlockConfig(), 1, arrays, engine)) == ref


# ---- 2. continuation --------------------------------------------------------------------------------------------------
def test_calls_continue_one_stream(engine):
    arrays = split(data("pysrc", 64, 16384), 16384) + ragged(9)
    want = expect(arrays)
    one, _ = gpu_host(engine, arrays)
    assert one == want
    for cut in (1, 7, 4096):
        engine.reset_compress_stream()
        parts = []
        for i in range(0, len(arrays), cut):
            f = gpu_device if (i // cut) % 2 else gpu_host
            parts.append(f(engine, arrays[i:i + cut])[0])
        assert b"".join(parts) == want, cut
    engine.reset_compress_stream()
    assert gpu_host(engine, arrays)[0] == want
    engine.set_compress_exact(True)            # switching on again starts a new stream too
    assert gpu_host(engine, arrays)[0] == want


def test_host_call_over_several_groups(engine):
    arrays = split(data("text", 200, 1 << 20, first=3), 1 << 20)     # 200 MiB: four 64 MiB groups
    want = expect(arrays)
    got, _ = gpu_host(engine, arrays)
    assert got == want


# ---- 3. speculation ---------------------------------------------------------------------------------------------------
def _with_env(monkeypatch, **kw):
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


@pytest.mark.parametrize("runin,piece", [(0, 0), (12, 0), (12, 3), (4, 5), (2, 1), (12, 64)])
def test_speculation_settings(engine, monkeypatch, runin, piece):
    _with_env(monkeypatch, MI355LZ4_EXACT_RUNIN=runin, MI355LZ4_EXACT_PIECE=piece)
    arrays = split(data("pysrc", 96, 65536), 65536)
    want = expect(arrays)
    got, _ = gpu_host(engine, arrays)
    assert got == want
    pieces, spec, kept, redone = engine.exact_state()
    assert kept + redone == spec
    if runin == 0:
        assert pieces == 1 and spec == 0


def test_runin_1_on_text_redoes_every_piece(engine, monkeypatch):
    _with_env(monkeypatch, MI355LZ4_EXACT_RUNIN=1, MI355LZ4_EXACT_PIECE=4)
    arrays = split(data("text", 48, 65536, first=11), 65536)
    want = expect(arrays)
    got, _ = gpu_device(engine, arrays)
    assert got == want
    pieces, spec, kept, redone = engine.exact_state()
    assert pieces == 12 and spec == 11 and redone == 11 and kept == 0


def test_runin_3_on_python_sources_mixes(engine, monkeypatch):
    _with_env(monkeypatch, MI355LZ4_EXACT_RUNIN=3, MI355LZ4_EXACT_PIECE=2)
    arrays = split(data("pysrc", 160, 65536), 65536)
    want = expect(arrays)
    got, _ = gpu_host(engine, arrays)
    assert got == want
    pieces, spec, kept, redone = engine.exact_state()
    assert kept > 0 and redone > 0, (pieces, spec, kept, redone)


# ---- 4. renorm --------------------------------------------------------------------------------------------------------
def test_stream_across_2gib_renorm(engine):
    os_ = OracleStream()
    r0 = os_.lib.orc_debug_renorms()
    big = 4 << 20
    text = data("text", 4, 65536, first=21)
    total = 0
    call = 0
    while total < (2 << 30) + (64 << 20):
        arrays = [bytes(big)] * 15 + [text[call % 3 * 65536:(call % 3 + 1) * 65536] * 64]   # zeros, then 4 MiB of text
        want = frame(os_.compress(arrays), arrays, 8)
        got, _ = gpu_device(engine, arrays, gap=0)
        assert got == want, call
        total += sum(len(a) for a in arrays)
        call += 1
    assert os_.lib.orc_debug_renorms() > r0


def test_renorm_block_starting_a_redone_piece(engine, monkeypatch):
    """The 2 GiB renorm falls on the first block of a speculated piece that fails its check and is redone: the redo
    starts from its predecessor's final table, which already has that block's renorm applied -- applying it again
    would zero the table and change the bytes."""
    os_ = OracleStream()
    big = 4 << 20
    prior = [bytes(big)] * 511 + [bytes((1 << 31) - 294912 - 511 * big)]    # currentOffset 2^31 - 4.5 * 64 KiB
    for i in range(0, len(prior), 128):
        part = prior[i:i + 128]
        want = frame(os_.compress(part), part, 8)
        assert gpu_device(engine, part, gap=0)[0] == want, i
    r0 = os_.lib.orc_debug_renorms()
    # 16 blocks of text: block 4 renorms (2^31 - 4.5 * 64 KiB + 5 * 64 KiB > 2^31) and starts piece 1 of 4-block pieces
    _with_env(monkeypatch, MI355LZ4_EXACT_RUNIN=1, MI355LZ4_EXACT_PIECE=4)
    arrays = split(data("text", 16, 65536, first=31), 65536)
    want = frame(os_.compress(arrays), arrays, 8)
    assert os_.lib.orc_debug_renorms() == r0 + 1
    got, _ = gpu_device(engine, arrays)
    assert got == want
    pieces, spec, kept, redone = engine.exact_state()
    assert (pieces, spec, redone) == (4, 3, 3)
    monkeypatch.delenv("MI355LZ4_EXACT_RUNIN")         # the stream goes on past the renorm, at the default speculation
    more = split(data("text", 40, 65536, first=47), 65536)
    assert gpu_host(engine, more)[0] == frame(os_.compress(more), more, 8)


# ---- 5. decoding ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoder", DECODERS)
def test_output_decodes_linked(engine, decoder):
    import streamly_lz4_amd as S
    raw = data("pysrc", 40, 65536)
    arrays = split(raw, 65536)
    framed, _ = gpu_host(engine, arrays)
    dec = S.Engine(0)
    dec.set_decoder(decoder)
    out, lens = dec.decompress_batch(framed, header_kind=8, linked=True)
    assert out == raw
    dec.close()
    assert orc().frame_decompress(framed, len(raw), 8, 65536, True) == raw


# ---- 6. determinism, default mode, refusals ---------------------------------------------------------------------------
def test_deterministic_and_other_stream(engine):
    import torch
    arrays = split(data("lzsynth", 32, 65536, first=2), 65536)
    a, _ = gpu_device(engine, arrays)
    engine.reset_compress_stream()
    b, _ = gpu_device(engine, arrays)
    s = torch.cuda.Stream()
    engine.reset_compress_stream()
    with torch.cuda.stream(s):
        c, _ = gpu_device(engine, arrays)
    assert a == b == c == expect(arrays)


def test_default_mode_unchanged_by_toggle():
    import streamly_lz4_amd as S
    arrays = split(data("text", 16, 65536, first=4), 65536)
    e = S.Engine(0)
    before = e.compress_batch(arrays)[0]
    e.set_compress_exact(True)
    exact = e.compress_batch(arrays)[0]
    e.set_compress_exact(False)
    assert e.compress_exact is False
    after = e.compress_batch(arrays)[0]
    e.close()
    assert before == after and exact != before


def test_refused_combinations(engine):
    import streamly_lz4_amd as S
    arrays = [b"abc" * 100]
    engine.set_compression_level(9)
    with pytest.raises(S.LZ4Error, match="compress_exact"):
        engine.compress_batch(arrays)
    engine.set_compression_level(0)
    engine.set_segments(4)
    with pytest.raises(S.LZ4Error, match="segments"):
        engine.compress_batch(arrays)
    engine.set_segments(-1)
    m = S.MultiEngine([0])
    S.lib.mi355lz4_multi_engine.restype = C.c_void_p
    S.lib.mi355lz4_multi_engine.argtypes = [C.c_void_p, C.c_int]
    assert S.lib.mi355lz4_set_compress_exact(C.c_void_p(S.lib.mi355lz4_multi_engine(m._h, 0)), 1) == 0
    with pytest.raises(S.LZ4Error, match="exact"):
        m.compress_batch(arrays)
    m.close()
    engine.set_linked_compress(True)          # ignored while the mode is on
    assert gpu_host(engine, arrays)[0] == expect(arrays)
