"""Fast fixed-size output pages on the GPU (mi355lz4_compress_pages_fast_device, mi355lz4_compress_pages_fast): every page is what
the contract says (tests/fastpages_model.py; include/mi355lz4.h) of the block E that mi355lz4_compress_batch_device
writes for the same slice with the same accel, byte for byte.

A test runs the call, reads the positions of its pages off its own pageSrcLen, gets E for every (input, position) from ONE
compress_batch_device call (segments off, unlinked, blocks of up to 65536 bytes) and lets the model walk the chain: the model confirms every
position, length and byte, and that nothing else was written (the pages start as 0xA5, the arrays as -77)."""
import json
import os

import numpy as np
import pytest

import fastpages_model as FM
import guarded as G
import lz4_check
import pages_cases as PC
import placement as P
import test_pages_gpu as TP
from conftest import DECODERS
from dict_cases import text

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_t = TP._t
TEXT8K = text(7600000, 8192)
TEXT32K = text(7600001, 32768)          # long enough for 133 sequences at accel 8 too


@pytest.fixture(scope="module", autouse=True)
def plain_batches(engine):
    """E is the batch call's block with segments off: its bytes then do not depend on how many blocks share a call"""
    engine.set_segments(0)
    yield
    engine.set_segments(-1)


def run_fast(engine, inputs, page_sizes, max_pages, hk, accel=1, stride=None, lens=None):
    """one mi355lz4_compress_pages_fast_device call, as test_pages_gpu.run_device: (pageSrcLen, pageCompLen, nPages, consumed, pages,
    stride), all numpy; the pages start as 0xA5 and the arrays as -77"""
    import torch
    n = len(inputs)
    if stride is None:
        stride = hk + max(1, max(page_sizes))
    src, offs = TP.pack(inputs)
    lens = [len(d) for d in inputs] if lens is None else lens
    pages = torch.full((n * max_pages * stride + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    sl, cl = (torch.full((n * max_pages,), -77, dtype=torch.int32, device=DEV) for _ in range(2))
    cnt, cons = (torch.full((n,), -77, dtype=torch.int32, device=DEV) for _ in range(2))
    engine.compress_pages_fast_device(_t(src), _t(np.array(offs, dtype=np.int64)), _t(np.array(lens, dtype=np.int32)), n,
                                      _t(np.array(page_sizes, dtype=np.int32)), max_pages, pages, stride, sl, cl, cnt, cons,
                                      header_kind=hk, accel=accel)
    engine.synchronize()
    return sl.cpu().numpy(), cl.cpu().numpy(), cnt.cpu().numpy(), cons.cpu().numpy(), pages.cpu().numpy(), stride


def kid(d):
    return len(d), hash(d)


class Blocks:
    """E for slices of inputs, from compress_batch_device: {(input's length and hash, pos, accel): block}, filled a call at a time"""

    def __init__(self, engine):
        self.engine = engine
        self.have = {}

    def fetch(self, wanted, accel):
        """wanted: [(data, pos)]; one batch call for those not there yet"""
        import torch
        todo = sorted({(kid(d), pos): (d, pos) for d, pos in wanted if (kid(d), pos, accel) not in self.have and pos < len(d)}.values(),
                      key=lambda x: (kid(x[0]), x[1]))
        if not todo:
            return
        datas = list({kid(d): d for d, _ in todo}.values())
        src, offs = TP.pack(datas)
        base = {kid(d): o for d, o in zip(datas, offs)}
        off = np.array([base[kid(d)] + pos for d, pos in todo], dtype=np.int64)
        ln = np.array([min(len(d) - pos, 65536) for d, pos in todo], dtype=np.int32)
        n = len(todo)
        import streamly_lz4_amd as S
        # (maxBlockLen only bounds the lengths and the slots: up to 65536 it is the same kernel and the same bytes)
        stride = int(S.slot_stride(int(max(ln)), 8))
        slots = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
        flen = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.engine.compress_batch_device(_t(src), n, int(max(ln)), slots, stride, flen, accel=accel, header_kind=8, src_off=_t(off),
                                          src_len=_t(ln))
        self.engine.synchronize()
        slots, flen = slots.cpu().numpy(), flen.cpu().numpy()
        for k, (d, pos) in enumerate(todo):
            assert flen[k] > 8, "the batch call failed on a slice"
            self.have[(kid(d), pos, accel)] = slots[k * stride + 8: k * stride + int(flen[k])].tobytes()

    def encoder(self, data, accel):
        def encode(piece, pos):
            return self.have[(kid(data), pos, accel)]       # KeyError: the model wants a position the call did not take
        return encode


@pytest.fixture(scope="module")
def blocks(engine):
    return Blocks(engine)


def positions(got, i, max_pages):
    sl, _, cnt, _, _, _ = got
    used = [int(sl[i * max_pages + k]) for k in range(max(int(cnt[i]), 0))]
    return [int(x) for x in np.cumsum([0] + used)]


def check_call(blocks, got, inputs, sizes, max_pages, hk, accel, what, skipped=()):
    """every input of a call against the model's chain over the batch call's blocks; returns the model's chains"""
    blocks.fetch([(d, pos) for i, d in enumerate(inputs) if i not in skipped for pos in positions(got, i, max_pages)], accel)
    chains = []
    for i, (d, t) in enumerate(zip(inputs, sizes)):
        if i in skipped:
            chains.append([])
            continue
        ch = FM.chain(d, t, blocks.encoder(d, accel), max_pages)
        TP.check_input(got, i, max_pages, hk, [(p, len(p), u) for p, u, *_ in ch], sum(u for _, u, *_ in ch), (what, i, len(d), t, hk, accel))
        chains.append(ch)
    return chains


def pages_needed(n, t):
    return 1 if t <= 1 else -(-n // FM.min_progress(t)) + 1


T_GROUPS = [(1, 1), (2, 4), (5, 16), (17, 64), (65, 256), (257, 700)]


@pytest.fixture(scope="module")
def edge_sizes(engine, blocks):
    """page sizes at which the page of TEXT32K's first slice ends behind sequence 60..68 and 124..132 of its block: the edges of the
    encoder's queue of 64 sequences.  Read off E (the batch call's block), per accel."""
    out = {}
    for accel in (1, 8):
        blocks.fetch([(TEXT32K, 0)], accel)
        seqs, _ = FM.sequences(blocks.have[(kid(TEXT32K), 0, accel)], len(TEXT32K))
        assert len(seqs) > 140, "the text input has too few sequences to reach the second edge of the queue"
        out[accel] = sorted(set(range(seqs[60][2], seqs[68][2] + 12)) | set(range(seqs[124][2], seqs[132][2] + 12)))
    return out


@pytest.mark.parametrize("hk", [0, 4, 8])
@pytest.mark.parametrize("accel", [1, 8])
def test_byte_exact_against_the_model(engine, blocks, edge_sizes, accel, hk):
    """every T in 1..700 on the 8 KiB text, every seventh on the five 2048-byte inputs, chains to their end; then the page sizes that
    put the cut at the queue's edges (the grid above ends at 700 bytes: no page of it holds 62 sequences)"""
    seen = set()
    calls = []
    for lo, hi in T_GROUPS:
        ts = list(range(lo, hi + 1))
        calls.append(([TEXT8K] * len(ts), ts, pages_needed(len(TEXT8K), lo)))
        ts7 = [t for t in range(1, 701, 7) if lo <= t <= hi]
        if ts7:
            calls.append(([PC.input_bytes(name) for name in PC.GRID_SMALL for _ in ts7], ts7 * len(PC.GRID_SMALL), pages_needed(2048, ts7[0])))
    ts = edge_sizes[accel]
    calls.append(([TEXT32K] * len(ts), ts, pages_needed(len(TEXT32K), ts[0])))
    for inputs, sizes, max_pages in calls:
        got = run_fast(engine, inputs, sizes, max_pages, hk, accel)
        chains = check_call(blocks, got, inputs, sizes, max_pages, hk, accel, "grid")
        for d, t, ch in zip(inputs, sizes, chains):
            assert sum(u for _, u, *_ in ch) == (len(d) if t > 1 else 0), ("the chain ends with the input", len(d), t)
            seen |= {j for _, _, j, _, _, cut in ch if cut}
    print("cuts seen: %d kinds, largest %d" % (len(seen), max(seen)))
    assert {-1, 0} <= seen
    assert set(range(62, 67)) <= seen and set(range(126, 131)) <= seen, sorted(seen)


def test_special_inputs(engine, blocks):
    rnd = PC.input_bytes("random2048")
    zeros, txt = PC.input_bytes("zeros70000"), PC.input_bytes("text70000")
    small = [b"", b"a", text(5, 12), text(6, 13)]
    # random bytes: all-literals pages, each the progress bound long
    got = run_fast(engine, [rnd], [300], 9, 8)
    ch = check_call(blocks, got, [rnd], [300], 9, 8, 1, "random")[0]
    assert [j for _, _, j, *_ in ch[:-1]] == [-1] * (len(ch) - 1) and all(u == FM.min_progress(300) for _, u, *_ in ch[:-1])
    # the 64 KiB bound: zeros give two pages that are E whole, far from full; text falls below 65536 remaining in mid-chain
    for t in (64, 4096):
        max_pages = pages_needed(70000, t)
        got = run_fast(engine, [zeros, txt], [t, t], max_pages, 8)
        chz, cht = check_call(blocks, got, [zeros, txt], [t, t], max_pages, 8, 1, "64 KiB")
        if t == 4096:       # (a block of 65536 zeros is about 270 bytes: at T = 64 the zeros go as literals)
            assert [(u, cut) for _, u, _, _, _, cut in chz] == [(65536, False), (70000 - 65536, False)]
            assert max(len(p) for p, *_ in chz) < 400, "pages that are E whole are far from full"
        assert any(n == 65536 for *_, n, _ in cht) and any(n < 65536 for *_, n, _ in cht[:-1])
        assert sum(u for _, u, *_ in cht) == 70000
    # inputs of 0, 1, 12 and 13 bytes: literals only, as the encoder makes them
    for t in (1, 2, 5, 13, 14, 15, 100):
        got = run_fast(engine, small, [t] * 4, 16, 4)
        chains = check_call(blocks, got, small, [t] * 4, 16, 4, 1, "small")
        assert [p for p, *_ in chains[0]] == [b"\x00"]
        assert all(j in (-1, None) for ch in chains for _, _, j, *_ in ch)
    # T >= compressBound(n): one page, the batch call's block
    ins = [PC.input_bytes(name) for name in PC.GRID_SMALL] + [TEXT8K]
    sizes = [PC.compress_bound(len(d)) + k for k, d in enumerate(ins)]
    got = run_fast(engine, ins, sizes, 2, 8, accel=8)
    chains = check_call(blocks, got, ins, sizes, 2, 8, 8, "bound")
    for d, ch in zip(ins, chains):
        assert len(ch) == 1 and ch[0][0] == blocks.have[(kid(d), 0, 8)] and ch[0][1] == len(d)


ROUND_TRIP = [("text2048", 64), ("text2048", 300), ("mixed2048", 100), ("period2048", 20), ("random2048", 271), ("zeros70000", 300),
              ("text70000", 4096), ("text70000", 700), ("text0", 9), ("text13", 9), ("text2048", 1)]


@pytest.mark.parametrize("decoder", DECODERS + [0])
def test_round_trip(engine, oracle, decoder):
    """headerKind 8 pages are ordinary blocks: every decoder variant and the CPU oracle decode each on its own, the strict validator
    passes each, and an input's decoded pages concatenate to its consumed prefix"""
    import torch
    inputs = [PC.input_bytes(name) for name, _ in ROUND_TRIP]
    sizes = [t for _, t in ROUND_TRIP]
    max_pages = 130
    sl, cl, cnt, cons, pages, stride = run_fast(engine, inputs, sizes, max_pages, 8)
    boff, ooff, want, pos = [], [], [], 0
    for i, (d, t) in enumerate(zip(inputs, sizes)):
        assert cons[i] == (len(d) if t > 1 else 0), (i, "the chain ends with the input")
        at = 0
        for k in range(int(cnt[i])):
            e = i * max_pages + k
            boff.append(e * stride); ooff.append(pos)
            want.append(d[at:at + int(sl[e])])
            block = pages[e * stride + 8: e * stride + 8 + int(cl[e])].tobytes()
            assert int(cl[e]) <= t
            lz4_check.check_block(block, int(sl[e]))
            if decoder == 0:
                assert oracle.decompress_block(block, int(sl[e])) == (int(sl[e]), want[-1]), (i, k)
            at += int(sl[e]); pos += int(sl[e]) + 3
        assert at == cons[i]
    n = len(boff)
    out = torch.full((pos + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    res = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    engine.set_decoder(decoder)
    try:
        engine.decompress_batch_device(_t(pages), pages.size, _t(np.array(boff, dtype=np.int64)), n, out,
                                       _t(np.array(ooff + [pos], dtype=np.int64)), res, header_kind=8, linked=False)
        engine.synchronize()
    finally:
        engine.set_decoder(0)
    res, out = res.cpu().numpy(), out.cpu().numpy()
    for j in range(n):
        assert res[j] == len(want[j]), (decoder, "page", j, int(res[j]), len(want[j]))
        assert out[ooff[j]:ooff[j] + len(want[j])].tobytes() == want[j], (decoder, "page", j)


def test_chains_skips_and_determinism(engine, blocks):
    txt = PC.input_bytes("text2048")
    # chains one page short
    for t in (16, 64, 256):
        full = len(positions(run_fast(engine, [txt], [t], pages_needed(2048, t), 8), 0, pages_needed(2048, t))) - 1
        got = run_fast(engine, [txt], [t], full - 1, 8)
        ch = check_call(blocks, got, [txt], [t], full - 1, 8, 1, "one page short")[0]
        assert len(ch) == full - 1 and got[3][0] < 2048
    # the per-input skips: a length outside 0..MI355LZ4_MAX_INPUT_SIZE, a page that does not fit the stride
    inputs = [txt, txt, txt, txt, txt, b""]
    lens = [2048, -1, 2048, 0x7E000001, 2048, 0]
    sizes = [100, 100, 101, 100, 64, 100]
    hk, stride, max_pages = 4, 104, 3
    got = run_fast(engine, inputs, sizes, max_pages, hk, stride=stride, lens=lens)
    sl, cl, cnt, cons, pages, _ = got
    for i in (1, 2, 3):
        assert cnt[i] == 0 and cons[i] == -77, (i, "a skipped input gets nPages = 0 and nothing else")
        TP.check_input((sl, cl, cnt, np.where(cons == -77, 0, cons), pages, stride), i, max_pages, hk, [], 0, ("skipped", i))
    check_call(blocks, got, inputs, sizes, max_pages, hk, 1, "beside a skipped input", skipped=(1, 2, 3))
    # pageSize < 1: no page, nothing consumed
    got = run_fast(engine, [txt, txt], [0, -5], 2, 8, stride=16)
    assert got[2].tolist() == [0, 0] and got[3].tolist() == [0, 0] and (got[4] == 0xA5).all()
    # 300 inputs with differing page sizes in one call, twice: the same bytes
    rs = np.random.RandomState(20261021)
    many = [text(int(rs.randint(1 << 30)), int(rs.randint(0, 3001))) if i % 3 else rs.randint(0, 7, size=int(rs.randint(0, 3001))).astype(np.uint8).tobytes()
            for i in range(300)]
    ts = [int(rs.randint(-2, 900)) for _ in many]
    a = run_fast(engine, many, ts, 6, 8, accel=2)
    b = run_fast(engine, many, ts, 6, 8, accel=2)
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x, y), "the same call twice gives other bytes"
    check_call(blocks, a, many, ts, 6, 8, 2, "300 inputs")


@pytest.mark.parametrize("hk", [0, 8])
def test_call_is_confined(engine, blocks, hk):
    """guard patterns (tests/guarded.py) as tests/test_pages_confinement_gpu.py: of a page the bytes [0, headerKind + compLen) and
    nothing behind them, unwritten pages and skipped inputs not at all, the arrays only at the entries of pages written, never an
    input.  The sizes come from a first, unguarded call that the model has confirmed."""
    import torch
    cases = [("text2048", 64), ("zeros70000", 100), ("random2048", 300), ("text70000", 4096), ("text0", 50), ("text13", 9),
             ("mixed2048", 17), ("period2048", 1), ("text100", 0), ("text100", 117), ("text2048", 271), ("text12", 13), ("text2048", 90)]
    max_pages = 5
    inputs = [PC.input_bytes(name) for name, _ in cases]
    n = len(inputs)
    lens = [len(d) for d in inputs]
    sizes = [t for _, t in cases]
    lens[2], sizes[9], dead = -3, 5000, {2, 9}
    stride = hk + 4096 + 41
    stride += (1 - stride) % 2
    first = run_fast(engine, inputs, sizes, max_pages, hk, stride=stride, lens=lens)
    want = check_call(blocks, first, inputs, sizes, max_pages, hk, 1, "before the guarded call", skipped=dead)
    assert any(len(w) == max_pages and sum(u for _, u, *_ in w) < len(d) for w, d in zip(want, inputs)), "no chain runs out of pages"
    written = [hk + len(want[i][k][0]) if k < len(want[i]) else 0 for i in range(n) for k in range(max_pages)]
    lay = G.layout(written, stride=stride, first_residue=5)
    seed = 157 + hk
    buf = G.new_torch(lay.total + stride, seed, DEV)
    lay_src = G.layout([len(d) for d in inputs])
    src = _t(G.pair(lay_src, inputs)[0])
    off = _t(np.array(lay_src.starts, dtype=np.int64))
    ln = _t(np.array(lens, dtype=np.int32))
    ps = _t(np.array(sizes, dtype=np.int32))
    copies = [t.clone() for t in (src, off, ln, ps)]
    sl, cl = (G.GuardedArray(n * max_pages, torch.int32, seed + 10 + j, DEV) for j in range(2))
    cnt, cons = (G.GuardedArray(n, torch.int32, seed + 20 + j, DEV) for j in range(2))
    engine.compress_pages_fast_device(src, off, ln, n, ps, max_pages, buf[lay.starts[0]:], stride, sl.view, cl.view, cnt.view, cons.view,
                                      header_kind=hk, accel=1)
    engine.synchronize()
    torch.cuda.synchronize()
    G.assert_confined(buf, lay.ranges(), seed, "pages")
    for t, c in zip((src, off, ln, ps), copies):
        assert torch.equal(t, c), "an input was written"
    entries = [i * max_pages + k for i in range(n) for k in range(len(want[i]))]
    for arr, what in ((sl, "pageSrcLen[]"), (cl, "pageCompLen[]")):
        s = arr.lay.starts[0]
        G.assert_confined(arr.buf, [(s + 4 * e, s + 4 * e + 4) for e in entries], arr.seed, what)
    cnt.check(what="nPages[]")
    s = cons.lay.starts[0]
    G.assert_confined(cons.buf, [(s + 4 * i, s + 4 * i + 4) for i in range(n) if i not in dead], cons.seed, "consumed[]")
    hb = buf.cpu().numpy()
    slv, clv = sl.view.cpu().numpy(), cl.view.cpu().numpy()
    for i in range(n):
        for k, (page, used, *_) in enumerate(want[i]):
            at = i * max_pages + k
            assert (int(clv[at]), int(slv[at])) == (len(page), used), (i, k)
            assert hb[lay.starts[at]:lay.starts[at] + hk + len(page)].tobytes() == TP.header(hk, len(page), used) + page, (i, k)


def test_host_form(engine, blocks):
    """mi355lz4_compress_pages_fast: one upload, the device call, the pages and the four arrays back: the device call's pages"""
    inputs = [PC.input_bytes("text2048"), PC.input_bytes("zeros70000"), b"", PC.input_bytes("mixed2048")]
    for t, max_pages, hk, accel in ((64, 50, 8, 1), (300, 4, 4, 8), (4096, 2, 0, 1)):
        got = engine.compress_pages_fast(inputs, t, max_pages, header_kind=hk, accel=accel)
        dev = run_fast(engine, inputs, [t] * len(inputs), max_pages, hk, accel)
        check_call(blocks, dev, inputs, [t] * len(inputs), max_pages, hk, accel, "host form")
        sl, cl, cnt, cons, pages, stride = dev
        for i, (pl, consumed) in enumerate(got):
            assert consumed == cons[i] and len(pl) == cnt[i]
            for k, (page, used) in enumerate(pl):
                e = i * max_pages + k
                assert used == sl[e] and page == pages[e * stride: e * stride + hk + int(cl[e])].tobytes(), (t, i, k)
    engine.set_compression_level(3)
    try:
        with pytest.raises(Exception, match="level"):
            engine.compress_pages_fast(inputs, 64, 2)
    finally:
        engine.set_compression_level(0)


def test_placement_beyond_4gib(engine, blocks):
    """sources beyond 2^32 in permuted order, pages at a stride of 2^28 + 37 so that (i * maxPages + k) * pageStride passes 2^32,
    guard windows around every page and at its 32-bit aliases (tests/placement.py)"""
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(0)
    if free < P.MIN_FREE:
        pytest.skip("needs 40 GiB of free device memory")
    wide = P.Space(32, front=1 << 30)
    stride, max_pages, hk = (1 << 28) + 37, 4, 8
    cases = [("text70000", 20000), ("text2048", 256), ("zeros70000", 100), ("text13", 64), ("mixed2048", 1000)]
    inputs = [PC.input_bytes(name) for name, _ in cases]
    sizes = [t for _, t in cases]
    near = run_fast(engine, inputs, sizes, max_pages, hk, stride=hk + 20000)
    want = check_call(blocks, near, inputs, sizes, max_pages, hk, 1, "near")
    far_in, far_out = P.new_far(DEV), P.new_far(DEV)
    try:
        starts = P.place([len(d) for d in inputs], "far_permuted", first_residue=3)
        decoys = []
        for d in inputs:
            shorter = [x for x in inputs if len(x) < len(d)]
            decoys.append(max(shorter, key=len) if shorter else min((x for x in inputs if len(x) > len(d)), key=len))
        P.put_inputs(far_in, starts, inputs, decoys)
        n = len(inputs)
        pstarts = [(i * max_pages + k) * stride for i in range(n) for k in range(max_pages)]
        psizes = [hk + len(want[i][k][0]) if k < len(want[i]) else 0 for i in range(n) for k in range(max_pages)]
        assert pstarts[-1] > 1 << 32
        win = P.Windows(pstarts, psizes, space=wide, seed=190)
        win.fill(far_out)
        sl, cl = (G.GuardedArray(n * max_pages, torch.int32, 191 + j, DEV) for j in range(2))
        cnt, cons = (G.GuardedArray(n, torch.int32, 193 + j, DEV) for j in range(2))
        engine.compress_pages_fast_device(P.view(far_in), _t(np.array(starts, dtype=np.int64)), _t(np.array([len(d) for d in inputs], dtype=np.int32)),
                                          n, _t(np.array(sizes, dtype=np.int32)), max_pages, P.view(far_out, wide), stride, sl.view, cl.view,
                                          cnt.view, cons.view, header_kind=hk, accel=1)
        engine.synchronize()
        win.check(far_out, "pages")
        cnt.check(what="nPages[]"); cons.check(what="consumed[]")
        assert cnt.view.cpu().tolist() == [len(w) for w in want]
        assert cons.view.cpu().tolist() == [sum(u for _, u, *_ in w) for w in want]
        for i in range(n):
            for k, (page, used, *_) in enumerate(want[i]):
                at = i * max_pages + k
                assert P.read(far_out, at * stride, hk + len(page), wide) == TP.header(hk, len(page), used) + page, (i, k)
    finally:
        far_in = far_out = None
        torch.cuda.empty_cache()


# The bound on the page count against the exact call.  The fast encoder is documented at 1.025 times the reference's size on text,
# and a cut without the reference's shortened last match gives up less than one sequence of a 1 KiB page: about 1.05 was expected.
# The first run on an MI355X measured 1.0000 (1024 pages from either call: 256 text records of 4 KiB into 1 KiB pages, these seeds --
# both calls need four pages a record, and the slack of the fourth page hides the difference in size); the bound is that value plus
# 0.03, to cover other seeds.
PAGE_COUNT_RATIO_MEASURED = 1.0
PAGE_COUNT_RATIO_BOUND = PAGE_COUNT_RATIO_MEASURED + 0.03


def test_page_count_against_the_exact_call(engine):
    """256 text records of 4 KiB (7k's generator) into 1 KiB pages: fewer pages than the all-literals chain would take, and no more
    than the bound above times compress_pages_device's count on the same records; the ratio goes into profiles/fastpages_rate.json"""
    recs = [text(7700000 + i, 4096) for i in range(256)]
    t, max_pages = 1024, 8
    fast = run_fast(engine, recs, [t] * 256, max_pages, 8)
    exact = TP.run_device(engine, recs, [t] * 256, max_pages, 8)
    assert (fast[3] == 4096).all() and (exact[3] == 4096).all()
    n_fast, n_exact = int(fast[2].sum()), int(exact[2].sum())
    ratio = n_fast / n_exact
    print("pages: fast %d, exact %d, ratio %.4f" % (n_fast, n_exact, ratio))
    assert n_fast < 256 * -(-4096 // FM.min_progress(t)), "no fewer pages than all-literals chains"
    path = os.path.join(ROOT, "profiles", "fastpages_rate.json")
    if os.path.exists(path) and os.access(path, os.W_OK):
        with open(path) as f:
            rec = json.load(f)
        entry = {"records": 256, "record_bytes": 4096, "page_size": t, "fast_pages": n_fast, "exact_pages": n_exact,
                 "ratio": round(ratio, 4)}
        if rec.get("page_count_ratio_vs_exact") != entry:           # (the same seeds give the same counts: nothing to rewrite)
            rec["page_count_ratio_vs_exact"] = entry
            with open(path, "w") as f:
                json.dump(rec, f, indent=1)
                f.write("\n")
    assert ratio <= PAGE_COUNT_RATIO_BOUND, (ratio, PAGE_COUNT_RATIO_BOUND)
