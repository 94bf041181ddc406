"""Development aid: many linked compress streams continued across calls, through the fast call and through the
calls it stands beside, all timed in one session.  Text of the engine's generator, every stream in a reset slot:
  (a) 2560 streams x 1 block of 64 KiB;
  (b) 16 streams x 160 blocks of 64 KiB -- a stream's blocks contiguous, as a file read in pieces is; also as one linked
      mi355lz4_compress_batch_device call per stream (16 calls, timed as one window), which the fast call's bytes must equal;
  (c) 16384 streams x 1 block of 4 KiB.
Each shape through mi355lz4_compress_streams_fast_device and through mi355lz4_compress_streams_device on the same input.
Every call is device-resident and event-timed on the engine's stream: one warm-up call per form, then `REPS` rounds in which the
forms alternate, the slots reset (enqueued, outside the timed window) in front of every call; a record holds the five times, their
median and the ratio input bytes / compressed bytes.
The one assertion: on (b) the fast call is at least 10 times faster than the exact call -- the exact call walks a stream's 160
blocks one after the other (about 11 ms a block), the fast call compresses all 2560 at once, and only a serialised implementation
can miss a factor of 10.
    timeout -k 10 900 python3 scripts/fstreams_rate.py [OUT.json [COMMIT]]
OUT.json defaults to profiles/fstreams_rate.json."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "streamly-lz4_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import streamly_lz4_amd as S  # noqa: E402

dev = "cuda:0"
eng = S.Engine(0)
REPS = 5


def timed(fn, before):
    before()
    a, b = S.Event(), S.Event()
    eng.record(a)
    fn()
    eng.record(b)
    eng.synchronize()
    return S.Engine.elapsed_ms(a, b)


def alternate(forms):
    """forms: {name: (fn, before)}.  One warm-up call each, then REPS rounds over all forms"""
    for fn, before in forms.values():
        before()
        fn()
    eng.synchronize()
    ts = {k: [] for k in forms}
    for _ in range(REPS):
        for name, (fn, before) in forms.items():
            ts[name].append(timed(fn, before))
    return {k: {"ms": v, "median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}


def shape(name, n_streams, per, bl, with_linked=False):
    n = n_streams * per
    src = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    eng.generate("text", src, bl, n, first_block=17)
    stride = S.slot_stride(bl, 8)
    sf = np.arange(n_streams + 1, dtype=np.int32) * per
    sl = np.arange(n_streams, dtype=np.int32)
    fs, cs = S.FastCompressStreams(eng, n_streams), S.CompressStreams(eng, n_streams)
    slots = {k: torch.empty(n * stride, dtype=torch.uint8, device=dev) for k in ("fast", "exact", "linked")[:3 if with_linked else 2]}
    flen = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in slots}
    eng.synchronize()

    def linked_calls():
        eng.set_linked_compress(True)
        for s in range(n_streams):
            lo = s * per
            eng.compress_batch_device(src[lo * bl:], per, bl, slots["linked"][lo * stride:], stride, flen["linked"][lo:])
        eng.set_linked_compress(False)

    forms = {
        "fast": (lambda: eng.compress_streams_fast_device(fs, src, n, bl, sf, sl, slots["fast"], stride, flen["fast"]), fs.reset),
        "exact": (lambda: eng.compress_streams_device(cs, src, n, bl, sf, sl, slots["exact"], stride, flen["exact"]), cs.reset),
    }
    if with_linked:
        forms["linked_call_per_stream"] = (linked_calls, lambda: None)
    rec = alternate(forms)
    for k in slots:
        fl = flen[k].cpu().numpy()
        assert (fl > 8).all(), (name, k, "a block failed")
        rec["linked_call_per_stream" if k == "linked" else k]["ratio"] = n * bl / float(fl.sum() - 8 * n)
    if with_linked:
        same = bool(torch.equal(flen["fast"], flen["linked"]))
        if same:
            rows_f, rows_l = slots["fast"].view(n, stride), slots["linked"].view(n, stride)
            keep = torch.arange(stride, device=dev)[None, :] < flen["fast"][:, None]
            same = bool(torch.equal(rows_f * keep, rows_l * keep))
        rec["fast_bytes_equal_linked_calls"] = same
    rec["shape"] = {"kind": "text", "streams": n_streams, "blocks_per_stream": per, "block": bl, "reps": REPS}
    rec["exact_over_fast"] = rec["exact"]["median_ms"] / rec["fast"]["median_ms"]
    rec["separated"] = rec["fast"]["max_ms"] < rec["exact"]["min_ms"]
    fs.close()
    cs.close()
    print(name, json.dumps({k: v for k, v in rec.items() if k != "shape"}), flush=True)
    return rec


record = {
    "a_2560_streams_x_1_block_64k": shape("a", 2560, 1, 65536),
    "b_16_streams_x_160_blocks_64k": shape("b", 16, 160, 65536, with_linked=True),
    "c_16384_streams_x_1_block_4k": shape("c", 16384, 1, 4096),
}
record["commit"] = sys.argv[2] if len(sys.argv) > 2 else None
record["device"] = torch.cuda.get_device_name(0)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fstreams_rate.json")
with open(out, "w") as f:
    json.dump(record, f, indent=1, sort_keys=True)
    f.write("\n")
b = record["b_16_streams_x_160_blocks_64k"]
assert b["exact_over_fast"] >= 10.0, "16 streams x 160 blocks: the fast call took %.2f ms, the exact call %.2f ms" % (
    b["fast"]["median_ms"], b["exact"]["median_ms"])
eng.close()
