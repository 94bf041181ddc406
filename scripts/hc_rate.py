"""Development aid: what the compression levels (mi355lz4_set_compression_level) cost and give on the device.  One JSON
record, printed and written to profiles/hc_rate.json (or the path given as the first argument): for levels 0, 3, 6 and 9,
device-resident compress rate (GB/s of input) and compressed bytes of
  65 536 x 64 KiB of text and of lzsynth (the bench's 4 GiB shape), and
  160 x 64 KiB of text (the small-call shape).
Times are the median of `reps` event-timed calls on the engine's stream after one warm-up call.
    python3 scripts/hc_rate.py [OUT.json] [CASE ...]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "streamly-lz4_amd"))
import torch  # noqa: E402
import streamly_lz4_amd as S  # noqa: E402

dev = "cuda:0"
eng = S.Engine(0)
LEVELS = (0, 3, 6, 9)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        a, b = S.Event(), S.Event()
        eng.record(a)
        fn()
        eng.record(b)
        ts.append(S.Engine.elapsed_ms(a, b))
    ts.sort()
    return ts[len(ts) // 2]


def rates(kind, bl, n, reps):
    src = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    eng.generate(kind, src, bl, n)
    stride = S.slot_stride(bl, 8)
    slots = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    flen = torch.zeros(n, dtype=torch.int32, device=dev)
    rec = {"kind": kind, "block": bl, "blocks": n, "input_bytes": n * bl, "reps": reps}
    for lv in LEVELS:
        eng.set_compression_level(lv)
        ms = timed(lambda: eng.compress_batch_device(src, n, bl, slots, stride, flen), reps)
        comp = int(flen.sum().item()) - 8 * n
        rec["level%d" % lv] = {"ms": ms, "GBps": n * bl / ms / 1e6, "compressed_bytes": comp, "ratio": n * bl / comp}
    eng.set_compression_level(0)
    base = rec["level0"]["compressed_bytes"]
    for lv in LEVELS[1:]:
        rec["level%d" % lv]["size_vs_level0"] = rec["level%d" % lv]["compressed_bytes"] / base
    del src, slots, flen
    torch.cuda.empty_cache()
    return rec


CASES = {
    "text_4GiB": ("text", 65536, 65536, 5),
    "lzsynth_4GiB": ("lzsynth", 65536, 65536, 5),
    "text_160x64k": ("text", 65536, 160, 15),
}
only = sys.argv[2:] or list(CASES)           # e.g. one case under rocprofv3 --kernel-trace
records = {name: rates(*CASES[name]) for name in only}
records["device"] = torch.cuda.get_device_name(0)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hc_rate.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(records, f, indent=1)
print(json.dumps(records))
eng.close()
