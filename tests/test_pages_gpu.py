"""Fixed-size output pages on the GPU (mi355lz4_compress_pages_device, mi355lz4_compress_pages): page k of an input is what the
reference's LZ4_compress_destSize returns, consumes and writes on the bytes behind pages 0..k-1.

The whole grid of tests/pages_cases.py runs through the device call for every header kind and must equal the golden
(tests/golden/pages_vectors.json: the reference's recorded results) and, byte for byte, the CPU model
(tests/native/fill_model.c, held to the same golden and to the reference itself by tests/test_pages_host.py); then the chains,
the per-input skips, the round trip through every decoder, a seeded differential fuzz, the progress bound, the host form and a
placement beyond 4 GiB.  The grid is about 4300 wavefronts in a handful of launches."""
import ctypes as C
import os

import numpy as np
import pytest

import guarded as G
import pages_cases as PC
import pages_model as PM
import placement as P
from conftest import DECODERS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "liblz4ref.so")
GAP = 7                                 # sources lie 7 bytes apart: every alignment, nothing to lean on


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pack(inputs, gap=GAP):
    """the inputs `gap` bytes apart in one buffer (0xEE between them): (bytes, offsets)"""
    parts, offs, pos = [], [], 0
    for d in inputs:
        parts.append(b"\xEE" * gap)
        pos += gap
        offs.append(pos)
        parts.append(bytes(d))
        pos += len(d)
    parts.append(b"\xEE" * 64)
    return np.frombuffer(bytearray(b"".join(parts)), dtype=np.uint8), offs


def run_device(engine, inputs, page_sizes, max_pages, hk, stride=None, lens=None):
    """one mi355lz4_compress_pages_device call: (pageSrcLen, pageCompLen, nPages, consumed, pages, stride), all numpy; the pages
    buffer starts as 0xA5 and the result arrays as -77, so what the call left alone shows"""
    import torch
    n = len(inputs)
    if stride is None:
        stride = hk + max(1, max(page_sizes))
    src, offs = pack(inputs)
    lens = [len(d) for d in inputs] if lens is None else lens
    pages = torch.full((n * max_pages * stride + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    sl, cl = (torch.full((n * max_pages,), -77, dtype=torch.int32, device=DEV) for _ in range(2))
    cnt, cons = (torch.full((n,), -77, dtype=torch.int32, device=DEV) for _ in range(2))
    engine.compress_pages_device(_t(src), _t(np.array(offs, dtype=np.int64)), _t(np.array(lens, dtype=np.int32)), n,
                                 _t(np.array(page_sizes, dtype=np.int32)), max_pages, pages, stride, sl, cl, cnt, cons, header_kind=hk)
    engine.synchronize()
    return sl.cpu().numpy(), cl.cpu().numpy(), cnt.cpu().numpy(), cons.cpu().numpy(), pages.cpu().numpy(), stride


def header(hk, comp, used):
    return b"" if hk == 0 else (int(comp).to_bytes(4, "little") + (int(used).to_bytes(4, "little") if hk == 8 else b""))


def check_input(got, i, max_pages, hk, want_pages, want_consumed, what):
    """input i of a call against its expected chain [(block bytes, compLen, srcLen)]: the four arrays, the bytes, and that
    everything behind a page's bytes and every page behind the chain is as the caller left it"""
    sl, cl, cnt, cons, pages, stride = got
    assert cnt[i] == len(want_pages), (what, "nPages", int(cnt[i]), len(want_pages))
    assert cons[i] == want_consumed, (what, "consumed", int(cons[i]), want_consumed)
    for k in range(max_pages):
        at = i * max_pages + k
        region = pages[at * stride:(at + 1) * stride]
        if k < len(want_pages):
            block, comp, used = want_pages[k]
            assert (int(cl[at]), int(sl[at])) == (comp, used), (what, "page", k, int(cl[at]), int(sl[at]), comp, used)
            assert region[:hk + comp].tobytes() == header(hk, comp, used) + block, (what, "page", k, "bytes differ")
            assert (region[hk + comp:] == 0xA5).all(), (what, "page", k, "written behind compLen")
        else:
            assert (int(cl[at]), int(sl[at])) == (-77, -77), (what, "entry of an unwritten page", k)
            assert (region == 0xA5).all(), (what, "unwritten page", k, "touched")


@pytest.fixture(scope="module")
def model_grid():
    """the model on every single-page case, once: {series: [(ret, used, rule, bytes)]}"""
    return {key: [PM.page(PC.input_bytes(name), t) for t in sizes] for key, name, sizes in PC.singles()}


@pytest.fixture(scope="module")
def model_chains():
    """the model on every chain, maxPages large enough, raw blocks: {(name, T): ([(block, compLen, srcLen)], consumed)}"""
    out = {}
    for name, t in PC.CHAINS:
        pages, consumed = PM.chain(PC.input_bytes(name), t, len(PC.input_bytes(name)) + 1)
        out[(name, t)] = ([(b, c, u) for b, c, u, _ in pages], consumed)
    return out


def expect_single(p):
    """a model page (ret, used, rule, bytes) as the chain of a maxPages == 1 call"""
    return ([(p[3], p[0], p[1])], p[1]) if p[0] > 0 else ([], 0)


@pytest.mark.parametrize("hk", [0, 4, 8])
def test_grid_equals_the_golden(engine, model_grid, hk):
    """every case of the grid as one input of maxPages == 1 calls (one call per stride class, so the buffers stay small)"""
    singles = PC.singles()
    for group in (lambda t: t <= 700, lambda t: 700 < t):
        inputs, sizes, want, keys = [], [], [], []
        for key, name, ts in singles:
            for j, t in enumerate(ts):
                if group(t):
                    inputs.append(PC.input_bytes(name)); sizes.append(t); want.append(model_grid[key][j]); keys.append((key, j, t))
        got = run_device(engine, inputs, sizes, 1, hk)
        for i, (p, (key, j, t)) in enumerate(zip(want, keys)):
            pages, consumed = expect_single(p)
            check_input(got, i, 1, hk, pages, consumed, (key, "pageSize", t, "headerKind", hk))
            gr, gu, gs = PM.golden_pages(key)[j]
            if gr > 0:                                                  # the reference's own numbers, not only the model's
                block = got[4][i * got[5] + hk: i * got[5] + hk + int(got[1][i])].tobytes()
                assert (int(got[1][i]), int(got[0][i]), PM.sha(block)) == (gr, gu, gs), (key, t, "golden")
            else:
                assert got[2][i] == 0 and got[3][i] == 0, (key, t, "a page that returns 0 is not written")


def test_chains(engine, model_chains):
    """every chain with maxPages large enough and one short of enough; pageSize 1 writes its zero token and stops"""
    for (name, t), (pages, consumed) in model_chains.items():
        data = PC.input_bytes(name)
        gold = PM.golden_pages(PC.chain_key(name, t))
        assert [(c, u, PM.sha(b)) for b, c, u in pages] == gold, (name, t, "model against golden")
        full = len(pages)
        for max_pages in sorted({full, full + 3} | ({full - 1} if full >= 2 else set())):
            want = pages[:max_pages]
            got = run_device(engine, [data], [t], max_pages, 8)
            check_input(got, 0, max_pages, 8, want, sum(u for _, _, u in want), (name, t, "maxPages", max_pages))
        if t == 1:
            assert full == 1 and pages[0] == (b"\x00", 1, 0) and consumed == 0
        else:
            assert consumed == len(data)


def test_skipped_inputs_leave_the_others_alone(engine):
    """a length outside 0..MI355LZ4_MAX_INPUT_SIZE and a page that does not fit the stride: nPages = 0 and nothing else"""
    text = PC.input_bytes("text2048")
    inputs = [text, text, text, text, text, b""]
    lens = [2048, -1, 2048, 0x7E000001, 2048, 0]
    sizes = [100, 100, 101, 100, 64, 100]                               # input 2: headerKind + 101 > stride
    hk, stride, max_pages = 4, 104, 3
    got = run_device(engine, inputs, sizes, max_pages, hk, stride=stride, lens=lens)
    sl, cl, cnt, cons, pages, _ = got
    for i in (1, 2, 3):
        assert cnt[i] == 0 and cons[i] == -77, (i, "a skipped input gets nPages = 0 and nothing else")
        check_input((sl, cl, cnt, np.where(cons == -77, 0, cons), pages, stride), i, max_pages, hk, [], 0, ("skipped", i))
    for i, t in ((0, 100), (4, 64)):
        want, _ = PM.chain(text, t, max_pages)
        check_input(got, i, max_pages, hk, [(b, c, u) for b, c, u, _ in want], sum(p[2] for p in want), ("beside a skipped input", i))
    check_input(got, 5, max_pages, hk, [(b"\x00", 1, 0)], 0, "the empty input")


@pytest.mark.parametrize("decoder", DECODERS + [0])
def test_round_trip(engine, model_chains, decoder):
    """the headerKind 8 pages of every chain are ordinary blocks: decoded where they lie, they concatenate to the input"""
    import torch
    names = list(model_chains)
    inputs = [PC.input_bytes(name) for name, _ in names]
    sizes = [t for _, t in names]
    max_pages = max(len(p) for p, _ in model_chains.values())
    sl, cl, cnt, cons, pages, stride = run_device(engine, inputs, sizes, max_pages, 8)
    boff, ooff, want, pos = [], [], [], 0
    for i, (key, data) in enumerate(zip(names, inputs)):
        assert cnt[i] == len(model_chains[key][0]) and cons[i] == model_chains[key][1], key
        at = 0
        for k in range(int(cnt[i])):
            boff.append((i * max_pages + k) * stride)
            ooff.append(pos)
            want.append(data[at:at + int(sl[i * max_pages + k])])
            at += int(sl[i * max_pages + k])
            pos += int(sl[i * max_pages + k]) + 3
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
    for (name, t), data in zip(names, inputs):
        if t > 1:
            assert model_chains[(name, t)][1] == len(data)


def fuzz_inputs(count=512, seed=20261020):
    """`count` inputs of 0..3000 bytes of four kinds, each with one random pageSize"""
    rs = np.random.RandomState(seed)
    inputs, sizes = [], []
    for i in range(count):
        n = int(rs.randint(0, 3001))
        kind = i % 4
        if kind == 0:
            d = PC.text(int(rs.randint(1 << 30)), n)
        elif kind == 1:
            d = rs.randint(0, 256, size=n).astype(np.uint8).tobytes()
        elif kind == 2:                                                 # long runs and short periods
            unit = rs.randint(0, 4, size=int(rs.randint(1, 9))).astype(np.uint8).tobytes()
            d = (unit * (n // len(unit) + 1))[:n]
        else:                                                           # pieces of the three
            cut = sorted(int(x) for x in rs.randint(0, n + 1, size=2))
            d = (rs.randint(0, 256, size=cut[0]).astype(np.uint8).tobytes() + bytes(cut[1] - cut[0]) + PC.text(i, n - cut[1]))
        inputs.append(d)
        sizes.append(int(rs.randint(-2, 3400)) if i % 8 else int(rs.randint(-2, 40)))
    return inputs, sizes


def test_differential_fuzz(engine):
    """against the model always, against the reference itself where it is built"""
    inputs, sizes = fuzz_inputs()
    max_pages = 6
    for hk in (0, 8):
        got = run_device(engine, inputs, sizes, max_pages, hk)
        for i, (d, t) in enumerate(zip(inputs, sizes)):
            want, consumed = PM.chain(d, t, max_pages)
            check_input(got, i, max_pages, hk, [(b, c, u) for b, c, u, _ in want], consumed, ("fuzz", i, len(d), t, hk))
    if os.path.exists(REF_SO):
        L = C.CDLL(REF_SO)
        L.LZ4_compress_destSize.restype = C.c_int
        L.LZ4_compress_destSize.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int]
        sl, cl, cnt, cons, pages, stride = got                          # the headerKind 8 run
        for i, (d, t) in enumerate(zip(inputs, sizes)):
            buf = np.frombuffer(d + bytes(64), dtype=np.uint8)
            pos = 0
            for k in range(int(cnt[i])):
                dst = np.zeros(max(t, 0) + 64, dtype=np.uint8)
                m = C.c_int(len(d) - pos)
                r = L.LZ4_compress_destSize(buf.ctypes.data + pos, dst.ctypes.data, C.byref(m), t)
                at = i * max_pages + k
                assert (r, m.value) == (int(cl[at]), int(sl[at])), ("fuzz against the reference", i, k)
                assert pages[at * stride + 8: at * stride + 8 + r].tobytes() == dst[:r].tobytes(), ("fuzz against the reference", i, k)
                pos += m.value


def test_progress(engine, model_grid):
    """every page of the grid that leaves input behind consumes at least (T - 1) - (T + 240) / 256 bytes: what a caller sizes
    maxPages by (include/mi355lz4.h).  Read off the device's own results, on the 2048-byte inputs and the long zeros."""
    inputs, sizes = [], []
    for key, name, ts in PC.singles():
        if key.startswith("grid/"):
            for t in ts:
                if t >= 1:
                    inputs.append(PC.input_bytes(name)); sizes.append(t)
    sl, cl, cnt, cons, _, _ = run_device(engine, inputs, sizes, 1, 0)
    checked = 0
    for i, (d, t) in enumerate(zip(inputs, sizes)):
        assert cnt[i] == 1
        if cons[i] < len(d):
            assert sl[i] >= PC.min_progress(t), (len(d), t, int(sl[i]))
            checked += 1
    assert checked > 2000, checked


def test_host_form(engine):
    """mi355lz4_compress_pages on three chains: one upload, the device call, the pages and the four arrays back"""
    inputs = [PC.input_bytes("text2048"), PC.input_bytes("zeros65000"), b"", PC.input_bytes("mixed2048")]
    for t, max_pages, hk in ((64, 50, 8), (300, 4, 4), (4096, 2, 0)):
        got = engine.compress_pages(inputs, t, max_pages, header_kind=hk)
        assert len(got) == len(inputs)
        for d, (pages, consumed) in zip(inputs, got):
            want, wc = PM.chain(d, t, max_pages, hk)
            assert consumed == wc
            assert pages == [(b, u) for b, _, u, _ in want], (t, max_pages, hk, len(d))


def test_placement_beyond_4gib(engine):
    """sources in permuted order and beyond 2^32 (srcOff from placement.place), pages at a stride of 2^28 + 37 so that pages 8..
    lie past 2^31 and pages 16.. past 2^32 -- (i * maxPages + k) * pageStride is a 64-bit product --, guard windows around every
    page and at its 32-bit aliases, other valid input at every alias of a source"""
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(0)
    if free < P.MIN_FREE:
        pytest.skip("needs 40 GiB of free device memory")
    wide = P.Space(32, front=1 << 30)
    stride, max_pages, hk = (1 << 28) + 37, 4, 8
    cases = [("text70000", 20000), ("text2048", 256), ("zeros65000", 100), ("text13", 64), ("mixed2048", 1000)]
    inputs = [PC.input_bytes(name) for name, _ in cases]
    sizes = [t for _, t in cases]
    want = [PM.chain(d, t, max_pages) for d, t in zip(inputs, sizes)]
    assert len(want[1][0]) == max_pages and want[1][1] < 2048, "one chain runs out of pages"
    far_in, far_out = P.new_far(DEV), P.new_far(DEV)
    try:
        starts = P.place([len(d) for d in inputs], "far_permuted", first_residue=3)
        layout = P.describe(starts, [len(d) for d in inputs])
        assert layout["above_full"] and layout["below_predecessor"] and layout["max_predecessor_distance"] > 1 << 32
        decoys = []                                                     # other valid input of another length, shorter where there is one
        for d in inputs:
            shorter = [x for x in inputs if len(x) < len(d)]
            decoys.append(max(shorter, key=len) if shorter else min((x for x in inputs if len(x) > len(d)), key=len))
        P.put_inputs(far_in, starts, inputs, decoys)
        n = len(inputs)
        pstarts, psizes = [], []
        for i in range(n):
            for k in range(max_pages):
                pstarts.append((i * max_pages + k) * stride)
                psizes.append(hk + want[i][0][k][1] if k < len(want[i][0]) else 0)
        assert pstarts[-1] > 1 << 32
        win = P.Windows(pstarts, psizes, space=wide, seed=90)
        win.fill(far_out)
        sl, cl = (G.GuardedArray(n * max_pages, torch.int32, 91 + j, DEV) for j in range(2))
        cnt, cons = (G.GuardedArray(n, torch.int32, 93 + j, DEV) for j in range(2))
        engine.compress_pages_device(P.view(far_in), _t(np.array(starts, dtype=np.int64)), _t(np.array([len(d) for d in inputs], dtype=np.int32)),
                                     n, _t(np.array(sizes, dtype=np.int32)), max_pages, P.view(far_out, wide), stride, sl.view, cl.view,
                                     cnt.view, cons.view, header_kind=hk)
        engine.synchronize()
        win.check(far_out, "pages")
        cnt.check(what="nPages[]"); cons.check(what="consumed[]")
        slv, clv = sl.view.cpu().numpy(), cl.view.cpu().numpy()
        assert cnt.view.cpu().tolist() == [len(w[0]) for w in want]
        assert cons.view.cpu().tolist() == [w[1] for w in want]
        for i in range(n):
            for k, (block, comp, used, _) in enumerate(want[i][0]):
                at = i * max_pages + k
                assert (int(clv[at]), int(slv[at])) == (comp, used), (i, k)
                assert P.read(far_out, at * stride, hk + comp, wide) == header(hk, comp, used) + block, (i, k)
    finally:
        far_in = far_out = None
        torch.cuda.empty_cache()
