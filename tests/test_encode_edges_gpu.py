"""Every GPU encoder on the edge inputs of tests/encode_cases.py, held to the strict block validator of tests/lz4_check.py.

One ragged device call (srcOff / srcLen, hundreds of blocks) per row of the matrix below and per acceleration: level 0 in its
small form (16-bit positions), its big form (32-bit positions: every case, the tiny ones too), cut into 2 and into up to 64
segments, with the library choosing the segments, linked; levels 1 and 9, and 9 linked.  Every block of every call must
  - carry a consistent framedLen, header and checksum trailer,
  - pass check_block -- the format's rules, the end rules included, which the reference's decoder does not enforce,
  - decode through the oracle to its input (with the block in front as dictionary in the linked rows),
  - hold a match where any working match finder finds one (must_match, at acceleration 1),
  - come out byte-identical from a second call,
and every GPU decoder must decode the call's slots back to the inputs.  The segment rows also get blocks whose lengths put
0..13 bytes behind a seam (a non-last segment must then stop short of it) and a block whose only repeat straddles a seam; the
segment length is computed here the way api.cpp computes it, so a change of that formula is a deliberate edit of this file.

The byte-pinned encoders (set_compress_exact, compress_streams_device) take the same list as the consecutive arrays of one
stream, and reversed as a second one: their bytes must be OracleStream's, array by array, and pass check_block with the stream's
window (the array in front, 64 KiB at the most) as dictionary.  No case is left out of that part: OracleStream expresses
every case, the empty arrays included.

Sizes are recorded next to the oracle's (measurements/encode_edges.jsonl), not asserted.

What this file found when it was written: every encoder kept every format rule on every case, and level 0 left period-3 blocks
of 64..75 bytes (and, linked, runs of that length) and the forced 5-byte match in 82 bytes without a single match -- a window of
encode_wave.hpp never finds its own repeats, and those blocks are one window or two.  Short blocks now enter 8 positions per
fruitless window (encode_wave.hpp, ENC_SHORT_STEP); must_match holds that."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from conftest import DECODERS  # noqa: E402
import encode_cases as EC  # noqa: E402
import lz4_check as LC  # noqa: E402

pytestmark = pytest.mark.gpu

ACCELS = [1, 2, 9, 400, 65537]
ENCODERS = {
    "noseg": dict(segments=0), "seg2": dict(segments=2), "seg64": dict(segments=64), "auto": dict(segments=-1),
    "linked": dict(linked=True), "level1": dict(level=1), "level9": dict(level=9), "level9_linked": dict(level=9, linked=True),
}
# (encoder, maxBlockLen, header kind, block checksums)
LEVEL0_ROWS = [
    ("noseg", 65536, 8, False),                                        # the small form: cases of up to 64 KiB
    ("noseg", 65537, 4, False), ("noseg", 262144, 8, False),           # the big form: all cases
    ("seg2", 8192, 8, False), ("seg2", 65536, 8, True), ("seg2", 262144, 4, False),
    ("seg64", 8192, 4, False), ("seg64", 65536, 8, False), ("seg64", 262144, 8, False),
    ("auto", 65536, 8, False),                                         # a few hundred blocks: the library cuts them into 16
    ("linked", 65536, 8, False), ("linked", 262144, 4, False),
]
LEVEL_ROWS = [
    ("level1", 65536, 8, False), ("level1", 262144, 4, False), ("level9", 65536, 4, False), ("level9", 262144, 8, False),
    ("level9_linked", 65536, 8, False), ("level9_linked", 262144, 8, False),
]
SEAM_ROWS = [(segs, M) for segs in (2, 64) for M in (8192, 65536, 262144)]
MAX_CALL = 8 << 20


@pytest.fixture(scope="module")
def cases():
    return EC.cases()


_oracle_sizes = {}


def oracle_size(oracle, data, accel):
    key = (data, accel)
    if key not in _oracle_sizes:
        _oracle_sizes[key] = len(oracle.compress_block(data, accel))
    return _oracle_sizes[key]


class configured:
    """the session's engine set up as one encoder, and back to its defaults afterwards"""

    def __init__(self, engine, segments=-1, linked=False, level=0, checksum=False):
        self.engine, self.set = engine, (segments, linked, level, checksum)

    def __enter__(self):
        self._apply(*self.set)
        return self.engine

    def __exit__(self, *exc):
        self._apply(-1, False, 0, False)
        self.engine.set_decoder(0)

    def _apply(self, segments, linked, level, checksum):
        self.engine.set_segments(segments)
        self.engine.set_linked_compress(linked)
        self.engine.set_compression_level(level)
        self.engine.set_block_checksum(checksum)


def device_call(engine, slz4, blocks, M, hk, ck, call, gap=0):
    """one compress call over `blocks` laid out gap bytes apart: call(src, n, M, slots, stride, flen, srcOff, srcLen); returns the
    device tensors and the layout"""
    import torch
    lens = [len(b) for b in blocks]
    assert sum(lens) <= MAX_CALL and max(lens) <= M
    offs = np.cumsum([0] + [L + gap for L in lens[:-1]]).astype(np.int64)
    host = np.zeros(int(offs[-1]) + lens[-1] + 64, dtype=np.uint8)          # (64 bytes of readable slack behind the last block)
    for o, b in zip(offs, blocks):
        host[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    n = len(blocks)
    stride = slz4.slot_stride_ex(M, hk, ck)
    t = dict(src=torch.from_numpy(host).cuda(), so=torch.from_numpy(offs).cuda(),
             sl=torch.tensor(lens, dtype=torch.int32, device="cuda:0"),
             slots=torch.zeros(n * stride, dtype=torch.uint8, device="cuda:0"),
             flen=torch.zeros(n, dtype=torch.int32, device="cuda:0"), stride=stride, n=n, lens=lens, offs=offs.tolist())
    call(t["src"], n, M, t["slots"], stride, t["flen"], t["so"], t["sl"])
    engine.synchronize()
    return t


def split_slots(slz4, t, blocks, hk, ck, what):
    """the compressed data of every slot, after the checks of framedLen, header and trailer"""
    sb = t["slots"].cpu().numpy()
    fl = t["flen"].cpu().tolist()
    comps = []
    for i, b in enumerate(blocks):
        fr = sb[i * t["stride"]:i * t["stride"] + fl[i]].tobytes()
        c = int.from_bytes(fr[:4], "little")
        assert c > 0 and fl[i] == hk + c + (4 if ck else 0), (what, i, len(b), fl[i], c)
        if hk == 8:
            assert int.from_bytes(fr[4:8], "little") == len(b), (what, i, "uncompLen")
        comp = fr[hk:hk + c]
        if ck:
            assert int.from_bytes(fr[hk + c:], "little") == slz4.xxh32(comp), (what, i, "trailer")
        comps.append(comp)
    return comps


def check_call(engine, slz4, oracle, record, enc, M, hk, ck, accel, blocks, names, flags, what):
    """the whole contract of one call (module docstring); blocks lie back to back"""
    import torch
    linked = bool(ENCODERS[enc].get("linked"))

    def call(src, n, mx, slots, stride, flen, so, sl):
        engine.compress_batch_device(src, n, mx, slots, stride, flen, accel=accel, header_kind=hk, src_off=so, src_len=sl,
                                     block_stride=0)

    with configured(engine, checksum=ck, **{k: v for k, v in ENCODERS[enc].items()}):
        t = device_call(engine, slz4, blocks, M, hk, ck, call)
        comps = split_slots(slz4, t, blocks, hk, ck, what)
        prev, unmatched = None, []                   # the last non-empty block in front: the linked rows' dictionary
        for i, (b, comp) in enumerate(zip(blocks, comps)):
            d = prev[-65536:] if (linked and prev) else None
            try:
                seqs, max_off, _, _ = LC.check_block(comp, len(b), len(d) if d else 0)
            except AssertionError as e:
                raise AssertionError("%r block %d (%s, %d bytes): %s" % (what, i, names[i], len(b), e))
            assert max_off <= 65535
            assert oracle.decompress_block(comp, len(b), d) == (len(b), b), (what, i, names[i], "the oracle does not decode it")
            if flags[i] and accel == 1 and seqs == 0:
                unmatched.append(names[i])
            if len(b):
                prev = b
        # a second identical call: identical bytes (the slots were zeroed, so the whole buffers compare)
        t2 = device_call(engine, slz4, blocks, M, hk, ck, call)
        assert torch.equal(t["flen"], t2["flen"]) and torch.equal(t["slots"], t2["slots"]), (what, "two calls, two results")
        del t2
        # every GPU decoder takes the slots back to the inputs
        n, total = t["n"], t["offs"][-1] + t["lens"][-1]
        boff = torch.arange(n, dtype=torch.int64, device="cuda:0") * t["stride"]
        for dec in list(DECODERS) + [0]:
            engine.set_decoder(dec)
            out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda:0")
            res = torch.full((n,), -99, dtype=torch.int32, device="cuda:0")
            engine.decompress_batch_device(t["slots"], t["slots"].numel(), boff, n, out, t["so"], res, header_kind=hk,
                                           fixed_uncomp=M if hk == 4 else 0, linked=linked, out_cap=t["sl"])
            engine.synchronize()
            assert res.cpu().tolist() == t["lens"], (what, "decoder %d" % dec)
            assert torch.equal(out[:total], t["src"][:total]), (what, "decoder %d" % dec)
        assert not unmatched, (what, "no match at all in", unmatched)
    return comps


def run_row(engine, slz4, oracle, record, cases, enc, M, hk, ck, accel):
    mine = [c for c in cases if len(c.data) <= M]
    assert len(mine) >= 300
    what = (enc, M, hk, ck, accel)
    comps = check_call(engine, slz4, oracle, record, enc, M, hk, ck, accel, [c.data for c in mine],
                       ["%s/%s" % (c.family, c.name) for c in mine], [c.must_match for c in mine], what)
    for family in EC.FAMILIES:
        got = sum(len(x) for c, x in zip(mine, comps) if c.family == family)
        ref = sum(oracle_size(oracle, c.data, accel) for c in mine if c.family == family)
        record("encode_edges", dict(encoder=enc, max_block_len=M, header_kind=hk, checksum=ck, accel=accel, family=family,
                                    engine_bytes=got, oracle_bytes=ref))


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("enc,M,hk,ck", LEVEL0_ROWS, ids=["%s-%d-hk%d%s" % (e, m, h, "-ck" if c else "") for e, m, h, c in LEVEL0_ROWS])
def test_level0_rows(engine, slz4, oracle, record, cases, enc, M, hk, ck, accel):
    run_row(engine, slz4, oracle, record, cases, enc, M, hk, ck, accel)


@pytest.mark.parametrize("enc,M,hk,ck", LEVEL_ROWS, ids=["%s-%d-hk%d" % (e, m, h) for e, m, h, _ in LEVEL_ROWS])
def test_level_rows(engine, slz4, oracle, record, cases, enc, M, hk, ck):
    run_row(engine, slz4, oracle, record, cases, enc, M, hk, ck, 1)


# ---- segment seams ------------------------------------------------------------------------------------------------------------

def seam_blocks(segs, M):
    """(segments the library cuts a block of a call with this maxBlockLen into, their length, {kind: blocks}): lengths
    k * segLen + t for k in {1, segments - 1} and t in 0..13, and one block whose only repeat straddles the first seam"""
    cut = min(segs, M // 4096, 64)                   # api.cpp: segments of 4 KiB at least, 64 at the most
    seg_len = (((M + cut - 1) // cut) + 63) & ~63    # api.cpp, EncodeSegArgs::segLen
    rng = random.Random(4242 + segs + M)
    text = EC._text(rng, M)
    full = {"zeros": bytes(M), "period 5": (b"abcde" * (M // 5 + 1))[:M], "text": text}
    out = {}
    for kind, src in full.items():
        out[kind] = [src[:k * seg_len + t] for k in sorted({1, cut - 1}) for t in range(14)]
        assert all(len(b) >= seg_len and len(b) <= M for b in out[kind])
    s = EC._rand(rng, 256)
    straddle = EC._rand(rng, seg_len - 428) + s + EC._rand(rng, 44) + s + EC._rand(rng, 200)
    assert straddle[seg_len - 128:seg_len + 128] == s and len(straddle) <= M
    out["zeros"].append(straddle)
    return cut, seg_len, out


def test_seam_blocks_follow_the_library():
    assert seam_blocks(2, 8192)[:2] == (2, 4096) and seam_blocks(64, 8192)[:2] == (2, 4096)
    assert seam_blocks(2, 65536)[:2] == (2, 32768) and seam_blocks(64, 65536)[:2] == (16, 4096)
    assert seam_blocks(2, 262144)[:2] == (2, 131072) and seam_blocks(64, 262144)[:2] == (64, 4096)


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("segs,M", SEAM_ROWS)
def test_segment_seams(engine, slz4, oracle, record, segs, M, accel):
    cut, seg_len, kinds = seam_blocks(segs, M)
    for kind, blocks in kinds.items():
        names = ["%s %d = %d * %d + %d" % (kind, len(b), len(b) // seg_len, seg_len, len(b) % seg_len) for b in blocks]
        flags = [kind != "text"] * len(blocks)
        if kind == "zeros":
            names[-1], flags[-1] = "the only repeat straddles the seam at %d" % seg_len, False
        comps = check_call(engine, slz4, oracle, record, "seg%d" % segs, M, 8, False, accel, blocks, names, flags,
                           ("seams", segs, M, accel, kind))
        record("encode_edges", dict(encoder="seg%d" % segs, max_block_len=M, accel=accel, family="seams " + kind,
                                    engine_bytes=sum(len(x) for x in comps),
                                    oracle_bytes=sum(oracle_size(oracle, b, accel) for b in blocks)))


# ---- the byte-pinned encoders ----------------------------------------------------------------------------------------------------

def check_stream(oracle, arrays, comps, want, what):
    prev = b""
    for i, (a, comp, w) in enumerate(zip(arrays, comps, want)):
        assert comp == w, (what, i, len(a), "not the reference's bytes")
        d = prev[-65536:]
        try:
            LC.check_block(comp, len(a), len(d))
        except AssertionError as e:
            raise AssertionError("%r array %d (%d bytes): %s" % (what, i, len(a), e))
        assert oracle.decompress_block(comp, len(a), d or None) == (len(a), a), (what, i)
        prev = a


@pytest.mark.parametrize("accel", [1, 9])
def test_exact_stream(engine, slz4, oracle, cases, accel):
    from test_exact_compress_gpu import OracleStream
    fwd = [c.data for c in cases]
    M = max(len(a) for a in fwd)

    def call(src, n, mx, slots, stride, flen, so, sl):
        engine.compress_batch_device(src, n, mx, slots, stride, flen, accel=accel, header_kind=8, src_off=so, src_len=sl,
                                     block_stride=0)

    engine.set_compress_exact(True)
    try:
        for name, arrays in (("forward", fwd), ("reversed", fwd[::-1])):
            engine.reset_compress_stream()
            t = device_call(engine, slz4, arrays, M, 8, False, call, gap=37)
            comps = split_slots(slz4, t, arrays, 8, False, ("exact", name, accel))
            check_stream(oracle, arrays, comps, OracleStream().compress(arrays, accel), ("exact", name, accel))
    finally:
        engine.set_compress_exact(False)


@pytest.mark.parametrize("accel", [1, 9])
def test_compress_streams(engine, slz4, oracle, cases, accel):
    from test_exact_compress_gpu import OracleStream
    fwd = [c.data for c in cases]
    M, n = max(len(a) for a in fwd), len(fwd)
    arrays = fwd + fwd[::-1]
    cs = slz4.CompressStreams(engine, 2)
    try:
        def call(src, nb, mx, slots, stride, flen, so, sl):
            engine.compress_streams_device(cs, src, nb, mx, [0, n, 2 * n], [0, 1], slots, stride, flen, accel=accel,
                                           header_kind=8, src_off=so, src_len=sl, block_stride=0)

        t = device_call(engine, slz4, arrays, M, 8, False, call, gap=37)
        comps = split_slots(slz4, t, arrays, 8, False, ("streams", accel))
    finally:
        cs.close()
    for name, lo in (("forward", 0), ("reversed", n)):
        part = arrays[lo:lo + n]
        check_stream(oracle, part, comps[lo:lo + n], OracleStream().compress(part, accel), ("streams", name, accel))
