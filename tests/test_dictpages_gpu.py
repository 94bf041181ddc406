"""Fast fixed-size output pages against a prepared dictionary on the GPU (mi355lz4_compress_pages_fastdict_device,
mi355lz4_compress_pages_fastdict): every page is what the contract says (tests/dictpages_model.py; include/mi355lz4.h)
of the block E that mi355lz4_compress_fastdict_device writes for the same slice with the same object and the same accel, byte for
byte.

A test runs the call, reads the positions of its pages off its own pageSrcLen, gets E for every (input, position) from ONE
compress_fastdict_device call and lets the model walk the chain: the model confirms every position, length and byte, and that
nothing else was written (the pages start as 0xA5, the arrays as -77)."""
import os

import numpy as np
import pytest

import dict_cases
import dictpages_cases as DC
import dictpages_model as DM
import guarded as G
import lz4_check
import pages_cases as PC
import test_pages_gpu as TP
from dict_cases import dictionary, text

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOB = "MI355LZ4_FASTDICT_WAVES"
_t = TP._t
D64K = dictionary(65536)
EDGE8K = DC.edge_input(D64K)
TEXT32K = text(7600001, 32768)


@pytest.fixture(scope="module")
def setup():
    """an engine of this module's own and one prepared dictionary object; `use(D)` loads D unless it is what the object holds"""
    import streamly_lz4_amd as S
    os.environ.pop(KNOB, None)
    eng = S.Engine(0)
    hd = S.HcDict(eng)
    state = {"D": None}

    def use(D):
        if state["D"] != D:
            hd.load(_t(np.frombuffer(bytes(D) + b"\x00", dtype=np.uint8).copy()), len(D))
            eng.synchronize()
            assert len(hd) == min(len(D), 65536)
            state["D"] = bytes(D)
            state["images"] = (hd.image(), hd.fast_image())
        return bytes(D)[-65536:]

    yield S, eng, hd, use, state
    os.environ.pop(KNOB, None)
    eng.set_compression_level(0)
    eng.set_block_checksum(False)
    hd.close()
    eng.close()


def run_dp(setup, inputs, page_sizes, max_pages, hk, accel=1, stride=None, lens=None, waves=None):
    """one mi355lz4_compress_pages_fastdict_device call against what the object holds, as test_pages_gpu.run_device: (pageSrcLen,
    pageCompLen, nPages, consumed, pages, stride), all numpy, and the pages on the device; the pages start as 0xA5 and the arrays
    as -77"""
    import torch
    _, eng, hd, _, _ = setup
    n = len(inputs)
    if stride is None:
        stride = hk + max(1, max(page_sizes))
    src, offs = TP.pack(inputs)
    lens = [len(d) for d in inputs] if lens is None else lens
    pages = torch.full((n * max_pages * stride + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    sl, cl = (torch.full((n * max_pages,), -77, dtype=torch.int32, device=DEV) for _ in range(2))
    cnt, cons = (torch.full((n,), -77, dtype=torch.int32, device=DEV) for _ in range(2))
    if waves is not None:
        os.environ[KNOB] = str(waves)
    try:
        eng.compress_pages_fastdict_device(hd, _t(src), _t(np.array(offs, dtype=np.int64)), _t(np.array(lens, dtype=np.int32)), n,
                                           _t(np.array(page_sizes, dtype=np.int32)), max_pages, pages, stride, sl, cl, cnt, cons,
                                           header_kind=hk, accel=accel)
        eng.synchronize()
    finally:
        os.environ.pop(KNOB, None)
    return sl.cpu().numpy(), cl.cpu().numpy(), cnt.cpu().numpy(), cons.cpu().numpy(), pages.cpu().numpy(), stride, pages


def kid(d):
    return len(d), hash(d)


class Blocks:
    """E for slices of inputs, from compress_fastdict_device against the loaded dictionary: {(dictionary, input, pos, accel): block},
    filled a call at a time"""

    def __init__(self, setup):
        self.setup = setup
        self.have = {}

    def fetch(self, wanted, accel):
        """wanted: [(data, pos)]; one call for those not there yet"""
        import torch
        S, eng, hd, _, state = self.setup
        dk = kid(state["D"])
        todo = sorted({(kid(d), pos): (d, pos) for d, pos in wanted if (dk, kid(d), pos, accel) not in self.have and pos < len(d)}.values(),
                      key=lambda x: (kid(x[0]), x[1]))
        if not todo:
            return
        datas = list({kid(d): d for d, _ in todo}.values())
        src, offs = TP.pack(datas)
        base = {kid(d): o for d, o in zip(datas, offs)}
        off = np.array([base[kid(d)] + pos for d, pos in todo], dtype=np.int64)
        ln = np.array([min(len(d) - pos, 65536) for d, pos in todo], dtype=np.int32)
        n = len(todo)
        # (maxBlockLen only bounds the lengths and the slots: up to 65536 it is the same kernel and the same bytes)
        stride = int(S.slot_stride(int(max(ln)), 8))
        slots = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
        flen = torch.zeros(n, dtype=torch.int32, device=DEV)
        eng.compress_fastdict_device(hd, _t(src), n, int(max(ln)), slots, stride, flen, accel=accel, header_kind=8, src_off=_t(off),
                                     src_len=_t(ln), block_stride=0)
        eng.synchronize()
        slots, flen = slots.cpu().numpy(), flen.cpu().numpy()
        for k, (d, pos) in enumerate(todo):
            assert flen[k] > 8, "the dictionary batch call failed on a slice"
            self.have[(dk, kid(d), pos, accel)] = slots[k * stride + 8: k * stride + int(flen[k])].tobytes()

    def encoder(self, data, accel):
        dk = kid(self.setup[4]["D"])

        def encode(piece, pos):
            return self.have[(dk, kid(data), pos, accel)]       # KeyError: the model wants a position the call did not take
        return encode


@pytest.fixture(scope="module")
def blocks(setup):
    return Blocks(setup)


def positions(got, i, max_pages):
    sl, cnt = got[0], got[2]
    used = [int(sl[i * max_pages + k]) for k in range(max(int(cnt[i]), 0))]
    return [int(x) for x in np.cumsum([0] + used)]


def check_call(blocks, got, inputs, sizes, max_pages, hk, accel, what, skipped=()):
    """every input of a call against the model's chain over the dictionary batch call's blocks; returns the model's chains"""
    blocks.fetch([(d, pos) for i, d in enumerate(inputs) if i not in skipped for pos in positions(got, i, max_pages)], accel)
    chains = []
    for i, (d, t) in enumerate(zip(inputs, sizes)):
        if i in skipped:
            chains.append([])
            continue
        ch = DM.chain(d, t, blocks.encoder(d, accel), max_pages)
        TP.check_input(got[:6], i, max_pages, hk, [(p, len(p), u) for p, u, *_ in ch], sum(u for _, u, *_ in ch), (what, i, len(d), t, hk, accel))
        chains.append(ch)
    return chains


_VALID = set()


def validate(oracle, kept, inputs, chains):
    """every page of the chains through the strict validator and the CPU oracle, with the dictionary; a page cut by T that leaves
    input behind is T or T - 1 bytes long and makes the progress the contract promises.  (A page seen before is not walked again.)"""
    for d, ch in zip(inputs, chains):
        for pg, used, j, pos, n, cut in ch:
            key = (len(kept), hash(kept), pg, d[pos: pos + used])
            if key in _VALID:
                continue
            _VALID.add(key)
            lz4_check.check_block(pg, used, dict_len=len(kept))
            assert oracle.decompress_block(pg, used, dict_bytes=kept or None) == (used, d[pos: pos + used]), (len(d), pos, len(pg))


def full_and_progress(chains, sizes):
    for t, ch in zip(sizes, chains):
        for pg, used, j, pos, n, cut in ch:
            if cut and used < n and t > 1:
                assert len(pg) >= t - 1 and used >= DM.min_progress(t), (t, pos, len(pg), used)


def pages_needed(n, t):
    return 1 if t <= 1 else -(-n // DM.min_progress(t)) + 1


SMALL_T_GROUPS = [(1, 1), (2, 4), (5, 16), (17, 99)]


def decode_pages_on_device(setup, got, inputs, max_pages, D):
    """headerKind 8 pages as they lie, through decompress_dict_device with the page addresses as blockOff"""
    import torch
    _, eng, _, _, _ = setup
    sl, cl, cnt, cons, hp, stride, pages = got
    boff, ooff, want, pos = [], [], [], 0
    for i, d in enumerate(inputs):
        at = 0
        for k in range(int(cnt[i])):
            e = i * max_pages + k
            if int(sl[e]) == 0:
                continue                # (a zero token, T = 1 or an empty input: nothing to decode)
            boff.append(e * stride); ooff.append(pos)
            want.append(d[at: at + int(sl[e])])
            at += int(sl[e]); pos += int(sl[e]) + 3
    n = len(boff)
    out = torch.full((pos + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    res = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    dt = _t(np.frombuffer(bytes(D) + b"\x00", dtype=np.uint8).copy())
    eng.decompress_dict_device(pages, int(pages.numel()), _t(np.array(boff, dtype=np.int64)), n, dt, len(D), out,
                               _t(np.array(ooff, dtype=np.int64)), res, header_kind=8)
    eng.synchronize()
    res, out = res.cpu().numpy(), out.cpu().numpy()
    assert res.tolist() == [len(w) for w in want]
    for j in range(n):
        assert out[ooff[j]: ooff[j] + len(want[j])].tobytes() == want[j], ("page", j)
        assert (out[ooff[j] + len(want[j]): ooff[j] + len(want[j]) + 3] == 0x5A).all()


@pytest.mark.parametrize("hk", [0, 4, 8])
@pytest.mark.parametrize("accel", [1, 8])
def test_every_page_size_byte_exact_against_the_model(setup, blocks, oracle, accel, hk):
    """every T in 1..700 in one call of 700 inputs -- the 8 KiB input that starts and ends with dictionary bytes, against the 64 KiB
    dictionary; 40 pages an input, so the chains of T >= 100 or so run to the input's end --, then the small T on the input's last
    KiB to its end"""
    kept = setup[3](D64K)
    ts = list(range(1, 701))
    got = run_dp(setup, [EDGE8K] * 700, ts, 40, hk, accel)
    chains = check_call(blocks, got, [EDGE8K] * 700, ts, 40, hk, accel, "every T")
    validate(oracle, kept, [EDGE8K] * 700, chains)
    full_and_progress(chains, ts)
    assert all(sum(u for _, u, *_ in ch) == 8192 for ch in chains[300:]), "the chains of the larger page sizes end with the input"
    seen = {j for ch in chains for _, _, j, _, _, cut in ch if cut and j is not None}
    opens = sum(1 for ch in chains for pg, used, j, _, _, cut in ch if cut and used >= 13 and pg[0] >> 4 == 0)
    print("cuts seen: %d kinds, largest %d; pages that open with a match: %d" % (len(seen), max(seen), opens))
    assert {-1, 0, 1, 2} <= seen and opens > 100
    if hk == 8:
        decode_pages_on_device(setup, got, [EDGE8K] * 700, 40, D64K)
    tail = EDGE8K[-1024:]
    for lo, hi in SMALL_T_GROUPS:
        ts = list(range(lo, hi + 1))
        max_pages = pages_needed(1024, lo)
        got = run_dp(setup, [tail] * len(ts), ts, max_pages, hk, accel)
        chains = check_call(blocks, got, [tail] * len(ts), ts, max_pages, hk, accel, "small T")
        validate(oracle, kept, [tail] * len(ts), chains)
        full_and_progress(chains, ts)
        assert all(sum(u for _, u, *_ in ch) == (1024 if t > 1 else 0) for t, ch in zip(ts, chains))
    assert setup[4]["images"] == (setup[2].image(), setup[2].fast_image()), "a page call wrote the prepared dictionary"


@pytest.mark.parametrize("d", [0, 3, 6, 7, 8, 100, 4095, 65535, 65536, 70000])
def test_dictionary_lengths(setup, blocks, oracle, d):
    D = dictionary(d)
    kept = setup[3](D)
    src = DC.edge_input(D) if d else text(77000, 8192)
    ts = [10, 12, 13, 64, 300, 1024]
    max_pages = pages_needed(8192, 10)
    for accel in (1, 8):
        got = run_dp(setup, [src] * len(ts), ts, max_pages, 8, accel)
        chains = check_call(blocks, got, [src] * len(ts), ts, max_pages, 8, accel, "dictionary of %d" % d)
        validate(oracle, kept, [src] * len(ts), chains)
        full_and_progress(chains, ts)
        assert all(sum(u for _, u, *_ in ch) == 8192 for ch in chains)
    if d:
        decode_pages_on_device(setup, got, [src] * len(ts), max_pages, D)


def test_compressible_input_and_the_64k_bound(setup, blocks, oracle):
    kept = setup[3](D64K)
    # an input that is wholly a copy of dictionary text: every page is E whole -- 65536 input bytes at the most -- and far from full
    copy = D64K[3000:63000] * 3
    got = run_dp(setup, [copy], [4096], 6, 8)
    ch = check_call(blocks, got, [copy], [4096], 6, 8, 1, "a copy of the dictionary")[0]
    validate(oracle, kept, [copy], [ch])
    assert [(u, cut) for _, u, _, _, _, cut in ch] == [(65536, False), (65536, False), (180000 - 131072, False)]
    assert max(len(p) for p, *_ in ch) < 4096 - 1, "pages that are E whole are not full"       # (a full page is T or T - 1 bytes)
    # 200000 bytes of text at T = 4096: slices of 65536 bytes until fewer remain
    txt = text(7600002, 200000)
    max_pages = pages_needed(200000, 4096)
    got = run_dp(setup, [txt], [4096], max_pages, 8)
    ch = check_call(blocks, got, [txt], [4096], max_pages, 8, 1, "the 64 KiB bound")[0]
    validate(oracle, kept, [txt], [ch])
    full_and_progress([ch], [4096])
    assert any(n == 65536 for *_, n, _ in ch) and any(n < 65536 for *_, n, _ in ch[:-1])
    assert sum(u for _, u, *_ in ch) == 200000
    decode_pages_on_device(setup, got, [txt], max_pages, D64K)


@pytest.mark.parametrize("accel", [1, 8])
def test_cuts_at_the_queue_s_edges(setup, blocks, oracle, accel):
    """page sizes at which the page of the 32 KiB text's first slice ends behind sequence 60..68 and 124..132 of its block: the edges
    of the encoder's queue of 64 sequences.  Read off E (the dictionary batch call's block)."""
    kept = setup[3](D64K)
    blocks.fetch([(TEXT32K, 0)], accel)
    seqs, _ = DM.sequences(blocks.encoder(TEXT32K, accel)(None, 0), len(TEXT32K))
    assert len(seqs) > 140, "the text input has too few sequences to reach the second edge of the queue"
    ts = sorted(set(range(seqs[60][2], seqs[68][2] + 12)) | set(range(seqs[124][2], seqs[132][2] + 12)))
    got = run_dp(setup, [TEXT32K] * len(ts), ts, 2, 8, accel)
    chains = check_call(blocks, got, [TEXT32K] * len(ts), ts, 2, 8, accel, "queue edges")
    validate(oracle, kept, [TEXT32K] * len(ts), chains)
    seen = {ch[0][2] for ch in chains if ch[0][5]}
    assert set(range(62, 67)) <= seen and set(range(126, 131)) <= seen, sorted(seen)


def test_persistent_grid_of_two_waves(setup, blocks, oracle):
    """40 inputs of mixed lengths through a grid of two waves: window and table state carried from one input to the next; the
    default grid's result, and the model's"""
    kept = setup[3](D64K)
    rs = np.random.RandomState(20261022)
    lens = [0, 1, 12, 13, 14, 70000, 300, 5000] + [int(rs.randint(0, 9000)) for _ in range(32)]
    inputs = [text(int(rs.randint(1 << 30)), n) if i % 4 else (D64K[i * 700: i * 700 + n] + text(i, n))[:n] for i, n in enumerate(lens)]
    ts = [int(rs.randint(9, 1200)) for _ in inputs]
    max_pages = 12
    two = run_dp(setup, inputs, ts, max_pages, 8, accel=1, waves=-2)
    dflt = run_dp(setup, inputs, ts, max_pages, 8, accel=1)
    for x, y in zip(two[:5], dflt[:5]):
        assert np.array_equal(x, y), "a grid of two waves gives other bytes than the default grid"
    chains = check_call(blocks, two, inputs, ts, max_pages, 8, 1, "two waves")
    validate(oracle, kept, inputs, chains)
    assert any(len(ch) == max_pages and sum(u for _, u, *_ in ch) < len(d) for ch, d in zip(chains, inputs))
    assert setup[4]["images"] == (setup[2].image(), setup[2].fast_image()), "a page call wrote the prepared dictionary"


def test_chain_stops_and_skips(setup, blocks, oracle):
    kept = setup[3](D64K)
    txt = EDGE8K[:2048]
    # inputs under 13 bytes: literals only, whatever the dictionary holds
    small = [b"", b"a", D64K[-12:], D64K[-13:], text(5, 12)]
    for t in (1, 2, 5, 13, 14, 15, 100):
        got = run_dp(setup, small, [t] * len(small), 16, 4)
        chains = check_call(blocks, got, small, [t] * len(small), 16, 4, 1, "small")
        validate(oracle, kept, small, chains)
        assert [p for p, *_ in chains[0]] == [b"\x00"]
        assert all(j in (-1, None) for k in (0, 1, 2, 4) for _, _, j, *_ in chains[k])
        for k in (1, 2, 4):
            assert all(lz4_check.check_block(p, u, dict_len=len(kept))[0] == 0 for p, u, *_ in chains[k])
    # chains one page short
    for t in (16, 64, 256):
        full = len(positions(run_dp(setup, [txt], [t], pages_needed(2048, t), 8), 0, pages_needed(2048, t))) - 1
        got = run_dp(setup, [txt], [t], full - 1, 8)
        ch = check_call(blocks, got, [txt], [t], full - 1, 8, 1, "one page short")[0]
        assert len(ch) == full - 1 and got[3][0] < 2048
    # the per-input skips: a length outside 0..MI355LZ4_MAX_INPUT_SIZE, a page that does not fit the stride
    inputs = [txt, txt, txt, txt, txt, b""]
    lens = [2048, -1, 2048, 0x7E000001, 2048, 0]
    sizes = [100, 100, 101, 100, 64, 100]
    hk, stride, max_pages = 4, 104, 3
    got = run_dp(setup, inputs, sizes, max_pages, hk, stride=stride, lens=lens)
    sl, cl, cnt, cons, pages, _, _ = got
    for i in (1, 2, 3):
        assert cnt[i] == 0 and cons[i] == -77, (i, "a skipped input gets nPages = 0 and nothing else")
        TP.check_input((sl, cl, cnt, np.where(cons == -77, 0, cons), pages, stride), i, max_pages, hk, [], 0, ("skipped", i))
    check_call(blocks, got, inputs, sizes, max_pages, hk, 1, "beside a skipped input", skipped=(1, 2, 3))
    # pageSize < 1: no page, nothing consumed; pageSize == 1: a counted zero token that consumes nothing
    got = run_dp(setup, [txt, txt, txt], [0, -5, 1], 2, 8, stride=16)
    assert got[2].tolist() == [0, 0, 1] and got[3].tolist() == [0, 0, 0]
    check_call(blocks, got, [txt, txt, txt], [0, -5, 1], 2, 8, 1, "T < 1 and T == 1")


@pytest.mark.parametrize("hk", [0, 8])
def test_call_is_confined(setup, blocks, hk):
    """guard patterns (tests/guarded.py) as tests/test_fastpages_gpu.py: of a page the bytes [0, headerKind + compLen) and nothing
    behind them, unwritten pages and skipped inputs not at all, the arrays only at the entries of pages written, never an input,
    never the prepared dictionary.  The sizes come from a first, unguarded call that the model has confirmed."""
    import torch
    _, eng, hd, use, state = setup
    use(D64K)
    cases = [("text2048", 64), ("zeros70000", 100), ("random2048", 300), ("text70000", 4096), ("text0", 50), ("text13", 9),
             ("mixed2048", 17), ("period2048", 1), ("text100", 0), ("text100", 117), ("text2048", 271), ("text12", 13), ("text2048", 90)]
    max_pages = 5
    inputs = [PC.input_bytes(name) for name, _ in cases] + [EDGE8K, D64K[100:9000]]
    sizes = [t for _, t in cases] + [12, 700]
    n = len(inputs)
    lens = [len(d) for d in inputs]
    lens[2], sizes[9], dead = -3, 5000, {2, 9}
    stride = hk + 4096 + 41
    stride += (1 - stride) % 2
    first = run_dp(setup, inputs, sizes, max_pages, hk, stride=stride, lens=lens)
    want = check_call(blocks, first, inputs, sizes, max_pages, hk, 1, "before the guarded call", skipped=dead)
    assert any(len(w) == max_pages and sum(u for _, u, *_ in w) < len(d) for w, d in zip(want, inputs)), "no chain runs out of pages"
    written = [hk + len(want[i][k][0]) if k < len(want[i]) else 0 for i in range(n) for k in range(max_pages)]
    lay = G.layout(written, stride=stride, first_residue=5)
    seed = 257 + hk
    buf = G.new_torch(lay.total + stride, seed, DEV)
    lay_src = G.layout([len(d) for d in inputs])
    src = _t(G.pair(lay_src, inputs)[0])
    off = _t(np.array(lay_src.starts, dtype=np.int64))
    ln = _t(np.array(lens, dtype=np.int32))
    ps = _t(np.array(sizes, dtype=np.int32))
    copies = [t.clone() for t in (src, off, ln, ps)]
    sl, cl = (G.GuardedArray(n * max_pages, torch.int32, seed + 10 + j, DEV) for j in range(2))
    cnt, cons = (G.GuardedArray(n, torch.int32, seed + 20 + j, DEV) for j in range(2))
    eng.compress_pages_fastdict_device(hd, src, off, ln, n, ps, max_pages, buf[lay.starts[0]:], stride, sl.view, cl.view, cnt.view,
                                       cons.view, header_kind=hk, accel=1)
    eng.synchronize()
    torch.cuda.synchronize()
    G.assert_confined(buf, lay.ranges(), seed, "pages")
    for t, c in zip((src, off, ln, ps), copies):
        assert torch.equal(t, c), "an input was written"
    assert state["images"] == (hd.image(), hd.fast_image()), "the prepared dictionary was written"
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


def test_host_form_and_argument_errors(setup, blocks):
    """mi355lz4_compress_pages_fastdict: one upload, the device call, the pages and the four arrays back: the device call's pages.
    A level other than 0, block checksums and a null object are refused"""
    _, eng, hd, use, _ = setup
    use(D64K)
    inputs = [EDGE8K[:2048], PC.input_bytes("zeros70000"), b"", D64K[500:3000]]
    for t, max_pages, hk, accel in ((64, 50, 8, 1), (300, 4, 4, 8), (4096, 2, 0, 1)):
        got = eng.compress_pages_fastdict(inputs, hd, t, max_pages, header_kind=hk, accel=accel)
        dev = run_dp(setup, inputs, [t] * len(inputs), max_pages, hk, accel)
        check_call(blocks, dev, inputs, [t] * len(inputs), max_pages, hk, accel, "host form")
        sl, cl, cnt, cons, pages, stride, _ = dev
        for i, (pl, consumed) in enumerate(got):
            assert consumed == cons[i] and len(pl) == cnt[i]
            for k, (page, used) in enumerate(pl):
                e = i * max_pages + k
                assert used == sl[e] and page == pages[e * stride: e * stride + hk + int(cl[e])].tobytes(), (t, i, k)
    eng.set_compression_level(1)
    try:
        with pytest.raises(Exception, match="level"):
            eng.compress_pages_fastdict(inputs, hd, 64, 2)
        with pytest.raises(Exception, match="level"):
            run_dp(setup, inputs, [64] * 4, 2, 8)
    finally:
        eng.set_compression_level(0)
    eng.set_block_checksum(True)
    try:
        with pytest.raises(Exception, match="checksum"):
            eng.compress_pages_fastdict(inputs, hd, 64, 2)
        with pytest.raises(Exception, match="checksum"):
            run_dp(setup, inputs, [64] * 4, 2, 8)
    finally:
        eng.set_block_checksum(False)
    with pytest.raises(Exception, match="compress_pages_fastdict"):
        eng.compress_pages_fastdict(inputs, None, 64, 2)
    with pytest.raises(Exception, match="compress_pages_fastdict_device"):
        run_dp((setup[0], eng, None, use, setup[4]), inputs, [64] * 4, 2, 8)


def test_page_count_against_the_call_without_a_dictionary(setup, engine):
    """64 text records of 4 KiB into 1 KiB pages: at most 3/4 of the pages compress_pages_fast_device needs for the same records.
    (The CPU model with the reference's parse gives 128 against 256; the margin is for the engine's own parse and for the slack of
    a record's last page.)"""
    import test_fastpages_gpu as TF
    setup[3](D64K)
    recs = [dict_cases.text(42000 + i, 4096) for i in range(64)]
    t, max_pages = 1024, 8
    with_dict = run_dp(setup, recs, [t] * 64, max_pages, 8)
    without = TF.run_fast(engine, recs, [t] * 64, max_pages, 8)
    assert (with_dict[3] == 4096).all() and (without[3] == 4096).all()
    n_dict, n_plain = int(with_dict[2].sum()), int(without[2].sum())
    print("pages: with the dictionary %d, without %d" % (n_dict, n_plain))
    assert 4 * n_dict <= 3 * n_plain, "pages with the dictionary %d, without %d" % (n_dict, n_plain)
