"""Batches of standard LZ4 frames on the GPU (include/mi355lz4.h, "batches of standard LZ4 frames"): mi355lz4_frames_load's
sizes, mi355lz4_frames_decode's results and the output bytes are held to tests/frames_model.py for every golden frame liblz4
wrote, every hand-built frame and every corruption -- each on its own, all in one call in shuffled order at all 16 residues of
inOff, and with both skip flags; the host form; equality with lz4FrameDecompress; a second load; a ragged 300-input call; an
input beyond 4 GiB."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import frames_cases as FC  # noqa: E402
import frames_model as M  # noqa: E402
import lz4f  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 32
FILL = 0xA7
L = lz4f.load()


@pytest.fixture(scope="module")
def eng():
    import streamly_lz4_amd as S
    e = S.Engine(0)
    yield e
    e.close()


_INPUTS = None
_EXPECT = {}


def inputs(oracle):
    """[(name, bytes)]: golden, hand-built, corrupt"""
    global _INPUTS
    if _INPUTS is None:
        _INPUTS = ([("golden/" + i, f) for i, f, _ in FC.golden()] + [("valid/" + n, f) for n, f, _ in FC.valid_cases(oracle)] +
                   [("corrupt/" + n, f) for n, f, _ in FC.corrupt_cases(oracle)])
    return _INPUTS


def expect(oracle, name, data, flags=0):
    """the model's answer, computed once per input and flag set and left unchanged"""
    key = (name, flags)
    if key not in _EXPECT:
        _EXPECT[key] = M.model(data, oracle, flags)
    return _EXPECT[key]


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)


def run(eng, datas, flags=0, residues=False, fr=None):
    """one load and one decode of the inputs: (sizes, results, [output bytes or None]); every output range lies between guard
    bytes, which must come back untouched, as must the range of an input whose size is a code"""
    import torch
    import streamly_lz4_amd as S
    n = len(datas)
    offs, pos = [], 5
    for i, d in enumerate(datas):
        if residues:
            pos += (i % 16 - pos) % 16
        offs.append(pos)
        pos += len(d) + 3
    buf = np.full(pos + 16, 0xEE, dtype=np.uint8)
    for o, d in zip(offs, datas):
        buf[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    dbuf, doff, dlen = _t(buf), _t(np.array(offs + [0], dtype=np.int64)), _t(np.array([len(d) for d in datas] + [0], dtype=np.int64))
    own = fr is None
    fr = fr or S.Frames(eng)
    sizes = fr.load(dbuf, doff, dlen, n_inputs=n, flags=flags)
    assert len(sizes) == n and fr.total() == sum(s for s in sizes if s > 0)
    assert n == 0 or fr.sizes_device_ptr()
    outs, at = [], GUARD
    for i, s in enumerate(sizes):
        at += (i * 7) % 16 if residues else 0
        outs.append(at)
        at += max(s, 0) + GUARD
    out = torch.full((at + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    result = torch.full((n + 2,), -77, dtype=torch.int64, device=DEV)
    fr.decode(out, _t(np.array(outs + [0], dtype=np.int64)), result[1:])
    torch.cuda.synchronize()
    res = result.cpu().numpy()
    assert res[0] == -77 and res[n + 1] == -77, "result[] written outside [0, nInputs)"
    got = out.cpu().numpy()
    mask = np.ones(got.size, dtype=bool)
    parts = []
    for o, s, r in zip(outs, sizes, res[1:n + 1]):
        if s >= 0:
            mask[o:o + s] = False
        parts.append(got[o:o + s].tobytes() if s >= 0 and r >= 0 else None)
    assert bool((got[mask] == FILL).all()), "bytes outside the inputs' output ranges were written"
    if own:
        fr.close()
    return sizes, [int(r) for r in res[1:n + 1]], parts


def check(oracle, named, got, flags=0):
    sizes, results, parts = got
    for (name, data), s, r, p in zip(named, sizes, results, parts):
        ws, wr, wp = expect(oracle, name, data, flags)
        assert (s, r) == (ws, wr), "%s: sizes %s result %s, the model says %s / %s" % (
            name, M.NAMES.get(s, s), M.NAMES.get(r, r), M.NAMES.get(ws, ws), M.NAMES.get(wr, wr))
        assert p == wp, "%s: the output bytes differ from the model's" % name


def test_every_input_on_its_own(eng, oracle):
    import streamly_lz4_amd as S
    fr = S.Frames(eng)                                   # (one object: every load replaces the one before)
    for name, data in inputs(oracle):
        check(oracle, [(name, data)], run(eng, [data], fr=fr))
    fr.close()


def test_all_in_one_call_shuffled_at_every_residue(eng, oracle):
    named = list(inputs(oracle))
    random.Random(5).shuffle(named)
    check(oracle, named, run(eng, [d for _, d in named], residues=True))


def test_skip_flags(eng, oracle):
    import streamly_lz4_amd as S
    named = [x for x in inputs(oracle) if not x[0].startswith("golden/") or "65537" in x[0] or "random" in x[0]]
    random.Random(6).shuffle(named)
    flags = S.FRAMES_SKIP_CONTENT_CHECKSUM | S.FRAMES_SKIP_BLOCK_CHECKSUM
    got = run(eng, [d for _, d in named], flags=flags, residues=True)
    check(oracle, named, got, flags)
    by = dict(zip([n for n, _ in named], got[1]))
    assert by["corrupt/block-checksum-flipped"] >= 0 and by["corrupt/content-checksum-flipped"] >= 0
    assert by["corrupt/header-checksum"] == M.E_HEADER_CHECKSUM and by["corrupt/cut-in-content-checksum"] == M.E_TRUNCATED


def test_unknown_flags_and_order_of_calls(eng):
    import streamly_lz4_amd as S
    fr = S.Frames(eng)
    z = _t(np.zeros(4, dtype=np.int64))
    with pytest.raises(S.LZ4Error):
        fr.decode(_t(np.zeros(8, dtype=np.uint8)), z, z)            # decode before any load
    with pytest.raises(S.LZ4Error):
        fr.load(_t(np.zeros(8, dtype=np.uint8)), z, z, n_inputs=1, flags=4)
    assert fr.load(None, None, None, n_inputs=0) == [] and fr.total() == 0 and fr.blocks() == 0
    fr.decode(None, None, None)                                      # nInputs == 0 is MI355LZ4_OK
    fr.close()


def test_host_form(eng, oracle):
    import ctypes as C
    import streamly_lz4_amd as S
    named = [x for x in inputs(oracle) if "-b7-" not in x[0]]
    random.Random(7).shuffle(named)
    parts, res = eng.decompress_frames([d for _, d in named], raise_on_error=False)
    for (name, data), p, r in zip(named, parts, res):
        _, wr, wp = expect(oracle, name, data)
        assert r == wr and p == (wp or b""), name
    with pytest.raises(S.LZ4Error):
        eng.decompress_frames([d for _, d in named])                 # MI355LZ4_E_BLOCK: some input failed
    # the capacity answer: one failed call sizes the buffer
    good = [d for n, d in named if n.startswith("valid/")]
    want = [expect(oracle, n, d)[2] for n, d in named if n.startswith("valid/")]
    total = sum(len(w) for w in want)
    arrs = [np.frombuffer(d, dtype=np.uint8) for d in good]
    ptrs = (S._u8p * len(good))(*[a.ctypes.data_as(S._u8p) if a.size else None for a in arrs])
    lens = (C.c_size_t * len(good))(*[a.size for a in arrs])
    result = (C.c_int64 * len(good))()
    out_len = C.c_size_t(12345)
    small = np.full(total, 0x5A, dtype=np.uint8)
    rc = S.lib.mi355lz4_decompress_frames(eng.ctx, ptrs, lens, len(good), 0, small.ctypes.data_as(S._u8p), total - 1, C.byref(out_len), result)
    assert rc == -4 and out_len.value == total and bool((small == 0x5A).all())
    rc = S.lib.mi355lz4_decompress_frames(eng.ctx, ptrs, lens, len(good), 0, small.ctypes.data_as(S._u8p), total, C.byref(out_len), result)
    assert rc == 0 and out_len.value == total and small.tobytes() == b"".join(want)
    assert eng.decompress_frames([]) == ([], [])


def test_equals_lz4FrameDecompress(eng, oracle):
    import streamly_lz4_amd as S
    for name, data in inputs(oracle):
        _, wr, wp = expect(oracle, name, data)
        if wr >= 0:
            assert S.lz4FrameDecompress(data, eng) == wp, name
        elif name != "corrupt/offset-zero":             # (the reference's decoder, v1.9.3, writes zeros for offset 0; the size rule refuses it)

            with pytest.raises(Exception):
                S.lz4FrameDecompress(data, eng)


def test_second_load_replaces_the_first(eng, oracle):
    import streamly_lz4_amd as S
    named = list(inputs(oracle))
    random.Random(8).shuffle(named)
    fr = S.Frames(eng)
    for k in (40, 7, 120):
        part = named[:k]
        check(oracle, part, run(eng, [d for _, d in part], fr=fr))
        named = named[k:] + named[:k]
    fr.close()


def test_three_hundred_ragged_inputs(eng):
    """frames the engine's own writer makes of 0 .. 200 KB of text, every option in turn, in one call"""
    import streamly_lz4_amd as S
    rng = random.Random(9)
    sizes = [0, 1, 200000] + [rng.randrange(0, 200001) for _ in range(297)]
    datas = [FC.content("text" if i % 5 else "random", n, 1000 + i) for i, n in enumerate(sizes)]
    frames = [S.lz4FrameCompress(d, eng, blockChecksum=bool(i & 1), contentSize=bool(i & 2), contentChecksum=bool(i & 4),
                                 linkedBlocks=bool(i & 8)) for i, d in enumerate(datas)]
    got_sizes, results, parts = run(eng, frames)
    assert got_sizes == sizes and results == sizes
    for i, (d, p) in enumerate(zip(datas, parts)):
        assert p == d, i


def test_last_input_beyond_4_gib(eng, oracle):
    import torch
    import streamly_lz4_amd as S
    named = [x for x in inputs(oracle) if x[0].startswith("valid/") or "text65537" in x[0]][:12]
    datas = [d for _, d in named]
    far = (1 << 32) + 12345
    buf = torch.empty(far + (1 << 20), dtype=torch.uint8, device=DEV)
    offs, pos = [], 3
    for i, d in enumerate(datas):
        at = far if i == len(datas) - 1 else pos
        buf[at:at + len(d)] = _t(np.frombuffer(d, dtype=np.uint8)) if d else buf[at:at]
        offs.append(at)
        pos += len(d) + 1
    fr = S.Frames(eng)
    sizes = fr.load(buf, _t(np.array(offs, dtype=np.int64)), _t(np.array([len(d) for d in datas], dtype=np.int64)))
    want = [expect(oracle, n, d) for n, d in named]
    assert sizes == [w[0] for w in want]
    outs = np.cumsum([0] + [max(s, 0) for s in sizes])
    out = torch.zeros(int(outs[-1]) + 16, dtype=torch.uint8, device=DEV)
    result = torch.zeros(len(datas), dtype=torch.int64, device=DEV)
    fr.decode(out, _t(outs[:-1].astype(np.int64)), result)
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [w[1] for w in want]
    got = out.cpu().numpy()
    for o, w in zip(outs, want):
        assert got[o:o + len(w[2])].tobytes() == w[2]
    fr.close()
    del buf


@pytest.mark.skipif(L is None, reason="system liblz4 with LZ4F_* not found")
def test_frames_of_both_writers(eng):
    import streamly_lz4_amd as S
    data = FC.content("text", 300000, 77) + FC.content("random", 70000, 78) + FC.content("text", 50000, 79)
    frames = []
    for k in range(16):
        frames.append(S.lz4FrameCompress(data, eng, blockChecksum=bool(k & 1), contentSize=bool(k & 2), contentChecksum=bool(k & 4),
                                         linkedBlocks=bool(k & 8), blockMax=1 + k % 4))
        frames.append(lz4f.compress_frame(L, data, block_id=4 + k % 4, linked=bool(k & 8), content_checksum=bool(k & 4),
                                          block_checksum=bool(k & 1), content_size=len(data) if k & 2 else 0, level=9 if k & 1 else 0))
    frames.append(lz4f.compress_pieces(L, FC.pieces_of(data), linked=True, content_checksum=True))
    sizes, results, parts = run(eng, frames)
    assert sizes == results == [len(data)] * len(frames)
    assert all(p == data for p in parts)
