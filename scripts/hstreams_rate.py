"""Development aid: the fast linked streams at a set's own level next to the forms they stand beside, all timed in
one session.  scripts/fstreams_rate.py's protocol and shapes -- text of the engine's generator, every stream in a reset slot:
  (a) 2560 streams x 1 block of 64 KiB;
  (b) 16 streams x 160 blocks of 64 KiB, a stream's blocks contiguous;
  (c) 16384 streams x 1 block of 4 KiB.
At levels 3 and 9, each shape through
  "set":    mi355lz4_compress_streams_fast_device with the set at level L (k_encode_hc_fstreams);
  "level0": the same call with the set at level 0 (k_encode_fstreams);
  "linked_call_per_stream": one linked mi355lz4_compress_batch_device call per stream with the engine at level L on the contiguous
            stream, timed as one window -- its bytes are the set form's by contract (checked here), and it is what the engine
            could run before the set had a level.
Every call is device-resident and event-timed on the engine's stream: one warm-up call per form, then `REPS` rounds in which the
forms alternate, the slots reset (enqueued, outside the timed window) in front of every call; a record holds the five times, their
median and the ratio input bytes / compressed bytes.  No rate is asserted: the new kernel is k_encode_hc plus two copies per staged
block, so the figure to look at is "set" against "linked_call_per_stream".
    timeout -k 10 1100 python3 scripts/hstreams_rate.py [OUT.json [COMMIT]]
OUT.json defaults to profiles/hstreams_rate.json."""
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
LEVELS = (3, 9)


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


def shape(name, level, n_streams, per, bl):
    n = n_streams * per
    src = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    eng.generate("text", src, bl, n, first_block=17)
    stride = S.slot_stride(bl, 8)
    sf = np.arange(n_streams + 1, dtype=np.int32) * per
    sl = np.arange(n_streams, dtype=np.int32)
    fs = S.FastCompressStreams(eng, n_streams)
    keys = ("set", "level0", "linked_call_per_stream")
    slots = {k: torch.empty(n * stride, dtype=torch.uint8, device=dev) for k in keys}
    flen = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in keys}
    eng.synchronize()

    def set_call(lv, key):
        def fn():
            fs.set_level(lv)
            eng.compress_streams_fast_device(fs, src, n, bl, sf, sl, slots[key], stride, flen[key])
            fs.set_level(0)
        return fn

    def linked_calls():
        eng.set_compression_level(level)
        eng.set_linked_compress(True)
        for s in range(n_streams):
            lo = s * per
            eng.compress_batch_device(src[lo * bl:], per, bl, slots[keys[2]][lo * stride:], stride, flen[keys[2]][lo:])
        eng.set_linked_compress(False)
        eng.set_compression_level(0)

    rec = alternate({"set": (set_call(level, "set"), fs.reset), "level0": (set_call(0, "level0"), fs.reset),
                     keys[2]: (linked_calls, lambda: None)})
    for k in keys:
        fl = flen[k].cpu().numpy()
        assert (fl > 8).all(), (name, k, "a block failed")
        rec[k]["ratio"] = n * bl / float(fl.sum() - 8 * n)
        rec[k]["compressed_bytes"] = int(fl.sum() - 8 * n)
    same = bool(torch.equal(flen["set"], flen[keys[2]]))
    if same:
        rows_s, rows_l = slots["set"].view(n, stride), slots[keys[2]].view(n, stride)
        keep = torch.arange(stride, device=dev)[None, :] < flen["set"][:, None]
        same = bool(torch.equal(rows_s * keep, rows_l * keep))
    rec["set_bytes_equal_linked_calls"] = same
    rec["shape"] = {"kind": "text", "level": level, "streams": n_streams, "blocks_per_stream": per, "block": bl, "reps": REPS}
    rec["linked_calls_over_set"] = rec[keys[2]]["median_ms"] / rec["set"]["median_ms"]
    rec["set_over_level0"] = rec["set"]["median_ms"] / rec["level0"]["median_ms"]
    rec["size_vs_level0"] = rec["set"]["compressed_bytes"] / rec["level0"]["compressed_bytes"]
    fs.close()
    print(name, level, json.dumps({k: v for k, v in rec.items() if k != "shape"}), flush=True)
    return rec


record = {}
for lv in LEVELS:
    record["level%d" % lv] = {
        "a_2560_streams_x_1_block_64k": shape("a", lv, 2560, 1, 65536),
        "b_16_streams_x_160_blocks_64k": shape("b", lv, 16, 160, 65536),
        "c_16384_streams_x_1_block_4k": shape("c", lv, 16384, 1, 4096),
    }
record["commit"] = sys.argv[2] if len(sys.argv) > 2 else None
record["device"] = torch.cuda.get_device_name(0)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hstreams_rate.json")
with open(out, "w") as f:
    json.dump(record, f, indent=1, sort_keys=True)
    f.write("\n")
for lv in LEVELS:
    for k, r in record["level%d" % lv].items():
        assert r["set_bytes_equal_linked_calls"], (lv, k, "the set's bytes are not the linked calls'")
eng.close()
