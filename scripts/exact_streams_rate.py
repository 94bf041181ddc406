"""Development aid: many reference-exact streams in one call (mi355lz4_compress_streams_device) against the only other
route to the same bytes on one engine -- reset_compress_stream plus one exact compress_batch_device call per stream, one
after another.  One JSON record per shape, printed and written to profiles/exact_streams_rate.json (or the path given as
the first argument):
  S streams x 4 blocks of 64 KiB of text, S in {64, 512, 2048, 8192}, and
  160 streams x 1 block of 64 KiB (the reference's 10 MiB protocol: 12.8 ms on one core, 1.5 ms on sixteen).
Device-resident, event-timed on the engine's stream, the median of `reps` calls after one warm-up call; every call starts
from reset slots.  The loop runs S serial chains one behind the other, so it takes S times one chain: LOOP_REPS (default
the same 5 after a warm-up; 0 leaves the loop out of a shape) shortens it where that is minutes.
    python3 scripts/exact_streams_rate.py [OUT.json] [CASE[:LOOP_REPS] ...]"""
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
BL = 65536


def timed(fn, reps, warm=True):
    if warm:
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


def rates(streams, per, reps, loop_reps):
    n = streams * per
    src = torch.empty(n * BL, dtype=torch.uint8, device=dev)
    eng.generate("text", src, BL, n)
    stride = S.slot_stride(BL, 8)
    slots = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    flen = torch.zeros(n, dtype=torch.int32, device=dev)
    cs = S.CompressStreams(eng, streams)
    first = list(range(0, n + 1, per))
    slot_of = list(range(streams))
    rec = {"kind": "text", "block": BL, "streams": streams, "blocks_per_stream": per, "input_bytes": n * BL, "reps": reps}

    def call():
        cs.reset()
        eng.compress_streams_device(cs, src, n, BL, first, slot_of, slots, stride, flen)

    ms = timed(call, reps)
    got = slots.clone()
    got_len = flen.clone()
    rec.update({"ms": ms, "GBps": n * BL / ms / 1e6, "compressed_bytes": int(flen.sum().item()) - 8 * n})
    if loop_reps > 0:
        eng.set_compress_exact(True)

        def loop():
            for s in range(streams):
                eng.reset_compress_stream()
                eng.compress_batch_device(src[s * per * BL:], per, BL, slots[s * per * stride:], stride, flen[s * per:])

        # (the streams call above has warmed the device up; a warm-up loop of its own only where the loop is short)
        lms = timed(loop, loop_reps, warm=streams * per <= 1024)
        eng.set_compress_exact(False)
        torch.cuda.synchronize()
        same = bool(torch.equal(got_len, flen)) and all(
            torch.equal(got[i * stride:i * stride + int(k)], slots[i * stride:i * stride + int(k)])
            for i, k in list(enumerate(got_len.tolist()))[:: max(1, n // 64)])
        rec.update({"loop_ms": lms, "loop_GBps": n * BL / lms / 1e6, "loop_reps": loop_reps, "loop_over_call": lms / ms,
                    "same_bytes": same})
    cs.close()
    del src, slots, flen, got, got_len
    torch.cuda.empty_cache()
    return rec


CASES = {
    "64x4": (64, 4, 5),
    "512x4": (512, 4, 5),
    "2048x4": (2048, 4, 5),
    "8192x4": (8192, 4, 5),
    "160x1": (160, 1, 5),
}
args = sys.argv[2:] or list(CASES)
records = {}
for a in args:
    name, _, lr = a.partition(":")
    streams, per, reps = CASES[name]
    records[name] = rates(streams, per, reps, int(lr) if lr else reps)
    print(name, json.dumps(records[name]), flush=True)
records["reference_160x64k_ms"] = {"one_core": 12.8, "sixteen_cores": 1.5}
records["device"] = torch.cuda.get_device_name(0)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "exact_streams_rate.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(records, f, indent=1)
print(json.dumps(records))
eng.close()
