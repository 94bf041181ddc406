"""mi355lz4_frames_decode on a non-blocking stream with late input: the protocol of tests/stream_order.py (imported, not edited).

The tables come from a load of the real frames; the decode is what runs late.  Real and decoy are frame pairs of equal shapes
-- the same block words at the same places, the same decoded sizes, other bytes -- so the tables fit both, and the decoy's
content checksums do not: a decode that read buf too early reports the decoy's codes and bytes, one that wrote too late leaves
the fill pattern.  The outputs must equal the default-stream run byte for byte, and gate.query() must be false right after
mi355lz4_frames_decode returns: the call only enqueues."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import frames_cases as FC  # noqa: E402
import frames_model as M  # noqa: E402
import lz4_synth as Z  # noqa: E402
import stream_order as SO  # noqa: E402

pytestmark = pytest.mark.gpu


def _frames(var):
    """six inputs whose shapes do not depend on the variant: literal-only and match-bearing hand-built blocks, stored blocks,
    linked and independent frames, with and without checksums"""
    seed = SO.SEED[var]
    t = lambda n, k: FC.content("text", n, seed * 100 + k)          # noqa: E731
    r = lambda n, k: FC.content("random", n, seed * 100 + k)        # noqa: E731

    def matchy(k):
        # the same sequence shapes for both variants, other literals: 40 literals, a match of 24 from 30 back, 12 last literals
        return Z.write_block([(r(40, k), 30, 24), (r(9, k + 1), 50, 60)], last_literals=r(12, k + 2))

    out = []
    for k, (linked, bsum, csum) in enumerate([(True, False, True), (False, True, True), (True, True, False), (False, False, True)]):
        blocks = [("c", FC.lit_block(t(3000, 10 * k))), ("s", r(700, 10 * k + 1)), ("c", matchy(10 * k + 2)), ("s", t(65536, 10 * k + 5)),
                  ("c", matchy(10 * k + 6))]
        body = FC._decode_linked(blocks) if linked else b"".join(
            b if kind == "s" else Z.plain_decode(b, 1 << 20)[1] for kind, b in blocks)
        out.append(FC.build(blocks, body, linked=linked, bsum=bsum, csum=csum, csize=True).data)
    out.append(FC.skippable(r(33, 90)) + out[0])
    out.append(b"")
    return out


def test_decode_only_enqueues_and_keeps_stream_order(oracle):
    import torch
    import streamly_lz4_amd as S
    frames = {v: _frames(v) for v in SO.VARIANTS}
    assert [len(f) for f in frames["real"]] == [len(f) for f in frames["decoy"]]
    want = [M.model(f, oracle) for f in frames["real"]]
    assert all(w[1] >= 0 for w in want)
    assert [M.model(f, oracle)[0] for f in frames["decoy"]] == [w[0] for w in want]
    off, bufs = SO.place(frames, gap=5)
    n = len(off)
    sizes = [w[0] for w in want]
    out_off = np.cumsum([0] + sizes)[:-1].astype(np.int64) + 3
    total = int(sum(sizes)) + 16
    inputs = {v: {"buf": bufs[v]} for v in SO.VARIANTS}
    state = {}

    def call(ctx, i, o):
        state["fr"].decode(o["out"], state["out_off"], o["result"])

    def canon(o):
        return {"out": np.asarray(o["out"]), "result": np.asarray(o["result"])}

    built = SO.Built("frames_decode", ["mi355lz4_frames_decode"], inputs, {"out": (total, np.uint8), "result": (n, np.int64)}, call, canon)
    h = SO.Harness(torch, lambda *a, **k: None)
    try:
        slot = h.slot(built)
        slot.load("real")
        torch.cuda.synchronize()
        fr = S.Frames(h.eng)
        state["fr"] = fr
        state["out_off"] = torch.from_numpy(out_off).to("cuda:0")
        doff = torch.from_numpy(np.array(off, dtype=np.int64)).to("cuda:0")
        dlen = torch.from_numpy(np.array([len(f) for f in frames["real"]], dtype=np.int64)).to("cuda:0")
        assert fr.load(slot.inp["buf"], doff, dlen) == sizes
        ref = h.reference([slot], model=False)[0]
        assert ref["real"]["result"].tolist() == sizes
        assert M.E_CONTENT_CHECKSUM in ref["decoy"]["result"].tolist()
        got = ref["real"]["out"]
        for o, w in zip(out_off, want):
            assert got[o:o + w[0]].tobytes() == w[2]
        for warm in (False, True):
            kept = h.late([slot], no_wait=(0,) if warm else ())
            h.judge(slot, kept[0])
        torch.cuda.synchronize()
        fr.close()
    finally:
        h.close()
