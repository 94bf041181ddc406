"""Writing batches of standard LZ4 frames on the GPU (include/mi355lz4.h, "writing batches of standard LZ4 frames").

Every frame mi355lz4_cframes_compress writes is held to two independent descriptions: tests/frames_model.py, the decode side's
contract, reads it back to the input (validity: fields, block count, the stored bit exactly where c >= n, every compressed block
through lz4_check), and tests/cframes_model.py rebuilds it byte for byte from the payloads of a per-input
mi355lz4_compress_batch_device call (pinned bytes).  Every call runs in guarded buffers (tests/guarded.py): inputs and frames
placed out of order, guards around and between the frame ranges and behind each frame's end, src and the offset arrays
compared afterwards.  Then: inputs that lie back to back in linked mode, the round trip through mi355lz4_frames and the system
liblz4, the codes, the engine switches that must not apply, and the host form across several groups."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import cframes_model as CM  # noqa: E402
import frames_cases as FC  # noqa: E402
import frames_model as M  # noqa: E402
import guarded as G  # noqa: E402
import lz4_check  # noqa: E402
import lz4f  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = lz4f.load()
LENGTHS = (0, 1, 12, 13, 65535, 65536, 65537, 3 * 65536, 3 * 65536 + 5)
KINDS = ("text", "random", "mixed")


@pytest.fixture(scope="module")
def eng():
    import streamly_lz4_amd as S
    e = S.Engine(0)
    e.set_segments(0)                       # the segment path makes the same choice in the writer's call and in the per-input ones
    yield e
    e.close()


_CONTENT = {}


def content(kind, n, seed):
    """text; random (every block is stored); mixed: text + random + text in thirds (a stored block inside a frame)"""
    key = (kind, n, seed)
    if key not in _CONTENT:
        if kind == "mixed":
            a = n // 3
            _CONTENT[key] = FC.content("text", a, seed) + FC.content("random", a, seed + 1) + FC.content("text", n - 2 * a, seed + 2)
        elif kind == "rep-mixed":
            a = n // 2
            _CONTENT[key] = FC.content("rep", a, seed) + FC.content("random", 65536, seed + 1) + FC.content("rep", n - a - 65536, seed + 2)
        else:
            _CONTENT[key] = FC.content(kind, n, seed)
    return _CONTENT[key]


def batch(kind, lengths=LENGTHS, seed=300):
    return [content(kind, n, seed + 7 * i) for i, n in enumerate(lengths)]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def level_of(flags):
    """level 0 and level 9, each with and without LINKED across the sixteen flag sets"""
    return 9 if ((flags >> 1) ^ (flags >> 3)) & 1 else 0


class Placed:
    """the inputs in one src buffer, out of order and at every alignment, `gap` bytes apart (order: where input i lies)"""

    def __init__(self, datas, gap=5, order=None, lead=3):
        n = len(datas)
        order = list(order) if order is not None else sorted(range(n), key=lambda i: (i * 7 + 3) % max(n, 1))
        self.off = [0] * n
        pos = lead
        for i in order:
            self.off[i] = pos
            pos += len(datas[i]) + gap
        self.buf = np.full(pos + 64, 0xEE, dtype=np.uint8)
        for o, d in zip(self.off, datas):
            self.buf[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
        self.len = [len(d) for d in datas]


def compress(eng, datas, bsid, flags, caps=None, placed=None, max_len=None, total_len=None, src_len=None, in_len=None, writer=None,
             accel=1):
    """one mi355lz4_cframes_compress call in guarded buffers: (frameLen list, [frame bytes or None], the device tensors for a
    round trip).  caps[i]: dstCap of input i (default: the bound).  Asserts the confinement rules of the header."""
    import torch
    import streamly_lz4_amd as S
    n = len(datas)
    placed = placed or Placed(datas)
    in_len = list(placed.len if in_len is None else in_len)
    caps = [CM.bound(len(d), bsid, flags) if c is None else c for d, c in zip(datas, caps or [None] * n)]
    # the frame ranges: guards between them, every start residue, and out of order (frame i at region perm[i])
    perm = sorted(range(n), key=lambda i: (i * 5 + 2) % max(n, 1))
    lay = G.layout([caps[i] for i in perm], first_residue=3)
    dst_off = [0] * n
    for r, i in enumerate(perm):
        dst_off[i] = lay.starts[r]
    dst = G.new_torch(lay.total, seed=91, device=DEV)
    flen = G.GuardedArray(n, torch.int64, seed=92, device=DEV)
    src_np = placed.buf
    src = _t(src_np)
    arrays = {"inOff": np.array(placed.off + [0], dtype=np.int64), "inLen": np.array(in_len + [0], dtype=np.int64),
              "dstOff": np.array(dst_off + [0], dtype=np.int64), "dstCap": np.array(caps + [0], dtype=np.int64)}
    dev = {k: _t(v) for k, v in arrays.items()}
    w = writer or S.FrameWriter(eng)
    w.compress(src, dev["inOff"], dev["inLen"], max(placed.len + [0]) if max_len is None else max_len,
               sum(placed.len) if total_len is None else total_len, dst, dev["dstOff"], dev["dstCap"], flen.view, block_size_id=bsid,
               flags=flags, accel=accel, n_inputs=n, src_len=src_np.size if src_len is None else src_len)
    torch.cuda.synchronize()
    if writer is None:
        w.close()
    lens = flen.view.cpu().numpy().tolist()
    flen.check(what="frameLen[]")
    allowed = [(dst_off[i], dst_off[i] + lens[i]) for i in range(n) if lens[i] >= 0]
    assert all(lens[i] <= caps[i] for i in range(n))
    G.assert_confined(dst, allowed, seed=91, what="dst")
    assert np.array_equal(src.cpu().numpy(), src_np), "src was written"
    for k, v in arrays.items():
        assert np.array_equal(dev[k].cpu().numpy(), v), k + " was written"
    host = dst.cpu().numpy()
    frames = [host[dst_off[i]:dst_off[i] + lens[i]].tobytes() if lens[i] >= 0 else None for i in range(n)]
    return lens, frames, dict(dst=dst, dst_off=dev["dstOff"], flen=flen.view, placed=placed, src=src)


def reference_payloads(eng, src, off, n, bsid, linked, max_block_len, accel=1):
    """the compressed bytes of the blocks of ONE input, by a mi355lz4_compress_batch_device call over those blocks alone where they
    lie in src (headerKind 4, the engine's level, the linked switch = the flag, the writer's maxBlockLen)"""
    import torch
    import streamly_lz4_amd as S
    bmax = CM.block_max(bsid)
    nb = -(-n // bmax)
    if nb == 0:
        return []
    stride = int(S.slot_stride(max_block_len, 4))
    slots = torch.zeros(nb * stride, dtype=torch.uint8, device=DEV)
    fl = torch.zeros(nb, dtype=torch.int32, device=DEV)
    eng.set_linked_compress(bool(linked))
    eng.compress_batch_device(src, nb, max_block_len, slots, stride, fl, accel=accel, header_kind=4,
                              src_off=_t(np.array([off + k * bmax for k in range(nb)], dtype=np.int64)),
                              src_len=_t(np.array([min(bmax, n - k * bmax) for k in range(nb)], dtype=np.int32)), block_stride=0)
    torch.cuda.synchronize()
    eng.set_linked_compress(False)
    host, lens = slots.cpu().numpy(), fl.cpu().numpy().tolist()
    out = []
    for k in range(nb):
        c = int.from_bytes(host[k * stride:k * stride + 4].tobytes(), "little")
        assert lens[k] == 4 + c
        out.append(host[k * stride + 4:k * stride + 4 + c].tobytes())
    return out


def check_valid(frame, data, bsid, flags, oracle, payloads=None):
    """the decode side's contract reads the frame back to the input; its fields, block count and stored bits are the writer's"""
    n = len(data)
    assert M.model(frame, oracle) == (n, n, data)
    frames, err = M.walk(frame)
    assert err is None and len(frames) == 1
    f = frames[0]
    bmax = CM.block_max(bsid)
    want_flg = 0x40 | (0 if flags & CM.LINKED else 0x20) | (0x10 if flags & CM.BLOCK_CHECKSUM else 0) | \
        (0x08 if flags & CM.CONTENT_SIZE else 0) | (0x04 if flags & CM.CONTENT_CHECKSUM else 0)
    assert f.flg == want_flg and f.bmax == bmax and frame[5] == bsid << 4
    assert f.declared == (n if flags & CM.CONTENT_SIZE else None)
    assert (f.checksum is not None) == bool(flags & CM.CONTENT_CHECKSUM)
    blocks = CM.cut(data, bsid)
    assert len(f.blocks) == len(blocks) == -(-n // bmax)
    done = 0
    for k, ((_p, stored, payload, ck), block) in enumerate(zip(f.blocks, blocks)):
        assert (ck is not None) == bool(flags & CM.BLOCK_CHECKSUM)
        if stored:
            assert payload == block
        else:
            assert len(payload) < len(block)
            lz4_check.check_block(payload, len(block), min(done, 65536) if flags & CM.LINKED else 0)
        if payloads is not None:
            assert stored == (len(payloads[k]) >= len(block)), "block %d: the stored bit is not c >= n" % k
        done += len(block)
    assert len(frame) <= CM.bound(n, bsid, flags)
    return f


def whole_check(eng, datas, bsid, flags, oracle, **kw):
    """validity and pinned bytes of every frame of one call"""
    lens, frames, ctx = compress(eng, datas, bsid, flags, **kw)
    max_block = min(CM.block_max(bsid), max([len(d) for d in datas] + [0]))
    stored = compressed = 0
    for i, (data, frame) in enumerate(zip(datas, frames)):
        assert lens[i] >= 0 and frame is not None, (i, lens[i])
        pay = reference_payloads(eng, ctx["src"], ctx["placed"].off[i], len(data), bsid, flags & CM.LINKED, max_block)
        f = check_valid(frame, data, bsid, flags, oracle, pay)
        assert frame == CM.frame(data, bsid, flags, pay), "input %d (%d bytes): not the model's bytes" % (i, len(data))
        stored += sum(1 for b in f.blocks if b[1])
        compressed += sum(1 for b in f.blocks if not b[1])
    return lens, frames, ctx, stored, compressed


@pytest.mark.parametrize("flags", range(16))
def test_every_flag_set_valid_and_pinned(eng, oracle, flags):
    """block id 4, the nine lengths, one content kind per flag set, level 0 or 9"""
    kind = KINDS[flags % 3]
    eng.set_compression_level(level_of(flags))
    try:
        _, _, _, stored, compressed = whole_check(eng, batch(kind), 4, flags, oracle)
    finally:
        eng.set_compression_level(0)
    if kind == "random":
        assert compressed == 0 and stored == sum(-(-n // 65536) for n in LENGTHS)
    elif kind == "text":
        assert (stored, compressed) == (5, 9)       # stored: 1, 12 and 13 bytes, and the tails of 1 and 5 bytes
    else:
        assert stored >= 2 and compressed >= 4      # a stored block inside a frame whose other blocks are compressed


def test_levels_and_linked_all_meet():
    seen = {(level_of(f), f & 1) for f in range(16)}
    assert seen == {(0, 0), (0, 1), (9, 0), (9, 1)}


def test_block_id_5(eng, oracle):
    bmax = 262144
    lengths = (0, 1, bmax - 1, bmax, bmax + 1, 2 * bmax + 5)
    for kind, flags, level in (("mixed", CM.LINKED | CM.CONTENT_CHECKSUM | CM.BLOCK_CHECKSUM, 0), ("text", CM.CONTENT_SIZE, 9)):
        eng.set_compression_level(level)
        try:
            whole_check(eng, batch(kind, lengths, seed=500), 5, flags, oracle)
        finally:
            eng.set_compression_level(0)


def test_block_id_7_one_input_of_4_mib_and_100(eng, oracle):
    data = content("rep-mixed", 4 * (1 << 20) + 100, 700)
    lens, frames, _, stored, compressed = whole_check(eng, [data], 7, CM.LINKED | CM.BLOCK_CHECKSUM | CM.CONTENT_SIZE, oracle)
    assert stored + compressed == 2 and compressed >= 1 and lens[0] < len(data) // 8


def test_back_to_back_linked_inputs(eng, oracle):
    """two inputs with no byte between them, the second beginning with a copy of the first's last 4 KiB: the first's last block
    must not become the dictionary of the second's first block"""
    a = content("text", 65536 + 20000, 800)
    b = a[-4096:] + content("text", 65536 + 3000, 801)
    datas = [a, b]
    placed = Placed(datas, gap=0, order=[0, 1])
    assert placed.off[1] == placed.off[0] + len(a)
    flags = CM.LINKED | CM.CONTENT_CHECKSUM
    for level in (0, 9):
        eng.set_compression_level(level)
        try:
            lens, frames, ctx, _, _ = whole_check(eng, datas, 4, flags, oracle, placed=placed)
            for d, f in zip(datas, frames):
                assert M.model(f, oracle) == (len(d), len(d), d)
            # the second input alone in a buffer of its own: its first block is the same block
            alone = Placed([b])
            first = reference_payloads(eng, _t(alone.buf), alone.off[0], len(b), 4, True, 65536)[0]
            assert M.walk(frames[1])[0][0].blocks[0][2] == first
            # ... and it holds no match that reaches in front of the frame
            lz4_check.check_block(first, 65536, 0)
        finally:
            eng.set_compression_level(0)


def test_round_trip_through_frames_and_liblz4(eng, oracle):
    import torch
    import streamly_lz4_amd as S
    datas = batch("mixed") + batch("text", (70000, 5), seed=900)
    flags = CM.LINKED | CM.BLOCK_CHECKSUM | CM.CONTENT_SIZE | CM.CONTENT_CHECKSUM
    lens, frames, ctx = compress(eng, datas, 4, flags)
    n = len(datas)
    fr = S.Frames(eng)
    sizes = fr.load(ctx["dst"], ctx["dst_off"], ctx["flen"], n_inputs=n)
    assert sizes == [len(d) for d in datas]
    out_off = np.cumsum([0] + sizes)[:-1].astype(np.int64)
    out = torch.zeros(sum(sizes) + 16, dtype=torch.uint8, device=DEV)
    result = torch.zeros(n, dtype=torch.int64, device=DEV)
    fr.decode(out, _t(out_off), result)
    torch.cuda.synchronize()
    assert result.cpu().numpy().tolist() == sizes
    assert out.cpu().numpy()[:sum(sizes)].tobytes() == b"".join(datas)
    fr.close()
    if L is None:
        pytest.skip("the system liblz4 does not load: the round trip through mi355lz4_frames stands alone")
    for d, f in zip(datas, frames):
        assert lz4f.decompress(L, f, len(d) + 16) == d


def test_codes_and_neighbours(eng, oracle):
    flags = CM.BLOCK_CHECKSUM | CM.CONTENT_CHECKSUM
    datas = [content("text", n, 1000 + i) for i, n in enumerate((70000, 3000, 65536, 200000, 12))]
    good, want, _ = compress(eng, datas, 4, flags)
    assert all(g == CM.bound(len(d), 4, flags) or g < CM.bound(len(d), 4, flags) for g, d in zip(good, datas))

    def neighbours(lens, frames, bad):
        for i in range(len(datas)):
            if i in bad:
                assert frames[i] is None
            else:
                assert lens[i] == good[i] and frames[i] == want[i], i

    # a capacity one byte short: _CAPACITY, nothing written for it (compress() checks the guards), the neighbours delivered
    caps = [None] * 5
    caps[1], caps[3] = good[1] - 1, good[3] - 1
    lens, frames, _ = compress(eng, datas, 4, flags, caps=caps)
    assert lens[1] == lens[3] == CM.E_CAPACITY
    neighbours(lens, frames, {1, 3})
    # ... and exactly the frame's length is enough
    caps[1], caps[3] = good[1], good[3]
    lens, frames, _ = compress(eng, datas, 4, flags, caps=caps)
    neighbours(lens, frames, set())
    # an input that ends past srcBufLen, and one that starts past it
    placed = Placed(datas, order=[4, 2, 1, 3, 0])                         # input 0 lies last in src
    lens, frames, _ = compress(eng, datas, 4, flags, placed=placed, src_len=placed.off[0] + len(datas[0]) - 1)
    assert lens[0] == CM.E_INPUT
    neighbours(lens, frames, {0})
    lens, frames, _ = compress(eng, datas, 4, flags, placed=placed, src_len=placed.off[0] - 1)
    assert lens[0] == CM.E_INPUT
    neighbours(lens, frames, {0})
    # an offset + length that wraps around 2^64 is outside too
    in_len = list(placed.len)
    in_len[2] = -8                                                        # 2^64 - 8 as an unsigned length
    lens, frames, _ = compress(eng, datas, 4, flags, placed=placed, in_len=in_len)
    assert lens[2] == CM.E_INPUT
    neighbours(lens, frames, {2})
    # over maxInputLen: the two longest
    lens, frames, _ = compress(eng, datas, 4, flags, max_len=65536, total_len=sum(len(d) for d in datas))
    assert lens[0] == lens[3] == CM.E_INPUT
    neighbours(lens, frames, {0, 3})
    # over the block bound: totalLen says one block, so the table holds 1 + 5; the inputs have 2 + 1 + 1 + 4 + 1 = 9.  Blocks are
    # counted in input order: inputs 0..2 fit (4 blocks), input 3 ends at 8 > 6 and input 4 behind it at 9
    lens, frames, _ = compress(eng, datas, 4, flags, total_len=65536)
    assert lens[3] == lens[4] == CM.E_INPUT
    neighbours(lens, frames, {3, 4})
    # a dstCap of the bound never fails: random data, every flag that adds bytes, both linked settings
    rnd = batch("random")
    for f in (CM.BLOCK_CHECKSUM | CM.CONTENT_SIZE | CM.CONTENT_CHECKSUM, CM.LINKED):
        lens, frames, _ = compress(eng, rnd, 4, f)
        assert lens == [CM.bound(len(d), 4, f) for d in rnd]


def test_engine_switches_that_do_not_apply(eng, oracle):
    """reference-exact mode and the engine's block checksums are off for the internal call, and all switches come back"""
    import streamly_lz4_amd as S
    datas = batch("text", (65537, 13, 100000), seed=1100)
    flags = CM.LINKED | CM.BLOCK_CHECKSUM
    _, want, _ = compress(eng, datas, 4, flags)
    eng.set_block_checksum(True)
    eng.set_compress_exact(True)
    try:
        _, got, _ = compress(eng, datas, 4, flags)
        assert eng.compress_exact
    finally:
        eng.set_compress_exact(False)
        eng.set_block_checksum(False)
    assert got == want
    for d, f in zip(datas, got):
        check_valid(f, d, 4, flags, oracle)
    # the engine's own linked switch is left as it was: an independent call behind a linked writer call is independent
    src = _t(np.frombuffer(datas[2], dtype=np.uint8).copy())
    pay = reference_payloads(eng, src, 0, len(datas[2]), 4, False, 65536)
    for k, p in enumerate(pay):
        lz4_check.check_block(p, min(65536, len(datas[2]) - k * 65536), 0)
    assert S.cframes_bound(0, 4, 0) == 11


def test_reserve_then_compress_and_a_second_call_on_one_writer(eng, oracle):
    import streamly_lz4_amd as S
    w = S.FrameWriter(eng)
    datas = batch("mixed", (65537, 0, 3 * 65536 + 5, 12), seed=1200)
    w.reserve(len(datas), max(len(d) for d in datas), sum(len(d) for d in datas), 4)
    first = compress(eng, datas, 4, CM.LINKED | CM.CONTENT_SIZE, writer=w)
    small = compress(eng, datas[:2], 4, CM.CONTENT_CHECKSUM, writer=w)
    again = compress(eng, datas, 4, CM.LINKED | CM.CONTENT_SIZE, writer=w)
    w.close()
    assert first[1] == again[1]
    for d, f in zip(datas, first[1]):
        check_valid(f, d, 4, CM.LINKED | CM.CONTENT_SIZE, oracle)
    for d, f in zip(datas[:2], small[1]):
        check_valid(f, d, 4, CM.CONTENT_CHECKSUM, oracle)
    empty = compress(eng, [], 4, 0)
    assert empty[0] == [] and empty[1] == []


def test_host_form(eng, oracle, monkeypatch):
    """the dense output is the device form's frames back to back; a small budget cuts the call into several groups; a capacity
    that is too small reports the total and writes nothing"""
    import ctypes as C
    import streamly_lz4_amd as S
    datas = batch("mixed") + batch("text", (65536, 1, 200000, 70000, 150000), seed=1300)
    flags = CM.LINKED | CM.BLOCK_CHECKSUM | CM.CONTENT_CHECKSUM
    _, want, _ = compress(eng, datas, 4, flags)
    frames, lens = eng.compress_frames(datas, 4, flags)
    assert frames == want and lens == [len(f) for f in want]
    # 1 MiB of inputs and bounds a group: the inputs above take more than two
    monkeypatch.setenv("MI355LZ4_CFRAMES_BUDGET_MB", "1")
    assert sum(len(d) + CM.bound(len(d), 4, flags) for d in datas) > 2 << 20
    frames, lens = eng.compress_frames(datas, 4, flags)
    monkeypatch.delenv("MI355LZ4_CFRAMES_BUDGET_MB")
    assert frames == want
    for d, f in zip(datas[:4], frames[:4]):
        check_valid(f, d, 4, flags, oracle)
    # the capacity answer
    total = sum(len(f) for f in want)
    n = len(datas)
    arrs = [np.frombuffer(d, dtype=np.uint8) for d in datas]
    u8p = C.POINTER(C.c_uint8)
    ptrs = (u8p * n)(*[a.ctypes.data_as(u8p) if a.size else None for a in arrs])
    sizes = (C.c_size_t * n)(*[a.size for a in arrs])
    flen = (C.c_int64 * n)()
    out = np.full(total + 64, 0xC3, dtype=np.uint8)
    out_len = C.c_size_t(5)
    rc = S.lib.mi355lz4_compress_frames(eng.ctx, ptrs, sizes, n, 4, flags, 1, out.ctypes.data_as(u8p), total - 1, C.byref(out_len), flen)
    assert rc == -4 and out_len.value == total and bool((out == 0xC3).all())
    assert [int(x) for x in flen] == [len(f) for f in want]
    rc = S.lib.mi355lz4_compress_frames(eng.ctx, ptrs, sizes, n, 4, flags, 1, out.ctypes.data_as(u8p), total, C.byref(out_len), flen)
    assert rc == 0 and out_len.value == total and out[:total].tobytes() == b"".join(want) and bool((out[total:] == 0xC3).all())
    assert eng.compress_frames([], 4, 0) == ([], [])
