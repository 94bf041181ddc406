"""What mi355lz4_compress_pages_device may write (include/mi355lz4.h, "what a call may write"), held with guard patterns
(tests/guarded.py) as tests/test_write_confinement_gpu.py does for the other calls: of page (i, k) the bytes
[0, headerKind + pageCompLen) and nothing behind them, pages that are not written not at all, pageSrcLen[] / pageCompLen[] only at
the entries of pages written, nPages[i], consumed[i] unless the input is skipped, and never an input.  Page regions start at all
16 residues and their written sizes are ragged; the tail of a written page and every unwritten page count as guard."""
import numpy as np
import pytest

import guarded as G
import pages_cases as PC
import pages_model as PM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (input, its length as the call is told -- None: the true one --, pageSize)
CASES = [("text2048", None, 64), ("zeros65000", None, 100), ("random2048", None, 300), ("text70000", None, 4096), ("text0", None, 50),
         ("text13", None, 9), ("mixed2048", None, 17), ("period2048", None, 1), ("text100", None, 0), ("text100", None, 117),
         ("zeros70000", None, 271), ("text65547", None, 4000), ("text12", None, 13)]
SKIPS = {2: ("len", -3), 5: ("len", 0x7E000001), 9: ("size", 5000)}     # with bad = True: two bad lengths, one page beyond the stride
MAX_PAGES = 5


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("bad", [False, True])
@pytest.mark.parametrize("extra", [1, 40])
@pytest.mark.parametrize("hk", [0, 4, 8])
def test_compress_pages_call_is_confined(engine, hk, extra, bad):
    import torch
    inputs = [PC.input_bytes(name) for name, _, _ in CASES]
    n = len(inputs)
    lens = [len(d) for d in inputs]
    sizes = [t for _, _, t in CASES]
    dead = set()
    if bad:
        for i, (what, v) in SKIPS.items():
            dead.add(i)
            if what == "len":
                lens[i] = v
            else:
                sizes[i] = v
    stride = hk + 4096 + extra
    stride += (1 - stride) % 2                                          # odd: 16 consecutive pages start at all 16 residues
    want = [([], 0) if i in dead else PM.chain(inputs[i], sizes[i], MAX_PAGES, hk) for i in range(n)]
    assert any(len(w[0]) == MAX_PAGES and w[1] < len(d) for w, d in zip(want, inputs)), "no chain runs out of pages"
    assert any(len(w[0]) == 0 for i, w in enumerate(want) if i not in dead), "no pageSize < 1"
    # the pages: region (i, k) is what the call may write of it -- nothing for a page that is not written
    written = [len(want[i][0][k][0]) if k < len(want[i][0]) else 0 for i in range(n) for k in range(MAX_PAGES)]
    lay = G.layout(written, stride=stride, first_residue=extra)
    assert lay.start_residues() == set(range(16)) and len(lay.end_residues()) >= 12 and len(set(written)) >= 8
    seed = 57 + hk
    buf = G.new_torch(lay.total + stride, seed, DEV)
    lay_src = G.layout([len(d) for d in inputs])
    assert lay_src.start_residues() == set(range(min(n, 16)))
    src = _t(G.pair(lay_src, inputs)[0])
    off = _t(np.array(lay_src.starts, dtype=np.int64))
    ln = _t(np.array(lens, dtype=np.int32))
    ps = _t(np.array(sizes, dtype=np.int32))
    copies = [t.clone() for t in (src, off, ln, ps)]
    sl, cl = (G.GuardedArray(n * MAX_PAGES, torch.int32, seed + 10 + j, DEV) for j in range(2))
    cnt, cons = (G.GuardedArray(n, torch.int32, seed + 20 + j, DEV) for j in range(2))
    engine.compress_pages_device(src, off, ln, n, ps, MAX_PAGES, buf[lay.starts[0]:], stride, sl.view, cl.view, cnt.view, cons.view,
                                 header_kind=hk)
    engine.synchronize()
    torch.cuda.synchronize()
    G.assert_confined(buf, lay.ranges(), seed, "pages")
    for t, c in zip((src, off, ln, ps), copies):
        assert torch.equal(t, c), "an input was written"
    entries = [i * MAX_PAGES + k for i in range(n) for k in range(len(want[i][0]))]
    for arr, what in ((sl, "pageSrcLen[]"), (cl, "pageCompLen[]")):
        s = arr.lay.starts[0]
        G.assert_confined(arr.buf, [(s + 4 * e, s + 4 * e + 4) for e in entries], arr.seed, what)
    cnt.check(what="nPages[]")
    s = cons.lay.starts[0]
    G.assert_confined(cons.buf, [(s + 4 * i, s + 4 * i + 4) for i in range(n) if i not in dead], cons.seed, "consumed[]")
    # ... and what it did write is the model's
    hb = buf.cpu().numpy()
    slv, clv, cntv, consv = (a.view.cpu().numpy() for a in (sl, cl, cnt, cons))
    for i in range(n):
        assert cntv[i] == len(want[i][0]), (i, int(cntv[i]))
        if i not in dead:
            assert consv[i] == want[i][1], i
        for k, (page, comp, used, _) in enumerate(want[i][0]):
            at = i * MAX_PAGES + k
            assert (int(clv[at]), int(slv[at])) == (comp, used), (i, k)
            assert hb[lay.starts[at]:lay.starts[at] + len(page)].tobytes() == page, (i, k)
