"""mi355lz4_cframes_compress on a non-blocking stream with late input: the protocol of tests/stream_order.py (imported, not
edited).

Real and decoy are inputs of equal lengths and other bytes at the same places, so one layout and one set of capacities fit
both.  The inputs hold the decoy and the outputs a fill pattern; behind a delay on the stream the real bytes are copied over
them, the call runs, the outputs are kept and the decoy comes back.  A call that read src too early writes the decoy's frames
-- other payloads, other lengths, other checksums -- one that wrote too late leaves the fill pattern.  The kept frames must equal
the default-stream run byte for byte, and gate.query() must be false right after a warm call returns: it only enqueues."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import cframes_model as CM  # noqa: E402
import frames_cases as FC  # noqa: E402
import frames_model as M  # noqa: E402
import stream_order as SO  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = (70000, 0, 13, 65536, 200000, 3000)
FLAGS = CM.LINKED | CM.BLOCK_CHECKSUM | CM.CONTENT_SIZE | CM.CONTENT_CHECKSUM


def _inputs(var):
    seed = SO.SEED[var]
    return [FC.content("text", n, seed * 100 + k) for k, n in enumerate(LENGTHS)]


def test_compress_only_enqueues_and_keeps_stream_order(oracle):
    import torch
    import streamly_lz4_amd as S
    datas = {v: _inputs(v) for v in SO.VARIANTS}
    off, bufs = SO.place(datas, gap=0)                  # back to back: the linked frames' spacers are at work too
    n = len(off)
    caps = [CM.bound(x, 4, FLAGS) for x in LENGTHS]
    dst_off = (np.cumsum([0] + [c + 9 for c in caps])[:-1] + 5).astype(np.int64)
    total = int(dst_off[-1] + caps[-1] + 16)
    meta = {"inOff": SO.arr(off + [0], np.int64), "inLen": SO.arr(list(LENGTHS) + [0], np.int64),
            "dstOff": SO.arr(list(dst_off) + [0], np.int64), "dstCap": SO.arr(caps + [0], np.int64)}
    inputs = {v: dict(meta, src=bufs[v]) for v in SO.VARIANTS}
    state = {}

    def call(ctx, i, o):
        state["w"].compress(i["src"], i["inOff"], i["inLen"], max(LENGTHS), sum(LENGTHS), o["dst"], i["dstOff"], i["dstCap"],
                            o["frameLen"], block_size_id=4, flags=FLAGS, n_inputs=n)

    def canon(o):
        lens = np.asarray(o["frameLen"])
        return {"frameLen": lens.copy(),
                "frames": [o["dst"][dst_off[i]:dst_off[i] + SO.clip(lens[i], caps[i])].tobytes() for i in range(n)]}

    built = SO.Built("cframes_compress", ["mi355lz4_cframes_compress"], inputs, {"dst": (total, np.uint8), "frameLen": (n, np.int64)},
                     call, canon)
    h = SO.Harness(torch, lambda *a, **k: None)
    try:
        slot = h.slot(built)
        w = S.FrameWriter(h.eng)
        w.reserve(n, max(LENGTHS), sum(LENGTHS), 4)
        state["w"] = w
        ref = h.reference([slot], model=False)[0]
        for v in SO.VARIANTS:
            assert all(x > 0 for x in ref[v]["frameLen"].tolist())
            for d, f in zip(datas[v], ref[v]["frames"]):
                assert M.model(f, oracle) == (len(d), len(d), d)
        for warm in (False, True):
            kept = h.late([slot], no_wait=(0,) if warm else ())
            h.judge(slot, kept[0])
        torch.cuda.synchronize()
        w.close()
    finally:
        h.close()
