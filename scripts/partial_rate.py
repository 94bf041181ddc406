"""Development aid: what a partial decode (mi355lz4_decompress_partial_device / mi355lz4_decompress_partial) costs next to the
full decode.  One JSON record, printed and written to profiles/partial_rate.json (or the path given as the first argument):
4096 x 64 KiB blocks of lzsynth and text-like data, targets 256 B, 4 KiB, 32 KiB and the full size, for
  device  the device call (prefixes packed at target stride) and, for comparison, mi355lz4_decompress_batch_device: ms per
          call (median of `reps` event-timed calls after a warm-up) and prefix bytes per second;
  host    the host form over the same chain in host memory and mi355lz4_decompress_batch: wall time per call (median of
          three after a warm-up) and prefix bytes per second.
    python3 scripts/partial_rate.py [OUT.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "streamly-lz4_amd"))
import torch  # noqa: E402
import streamly_lz4_amd as S  # noqa: E402

dev = "cuda:0"
eng = S.Engine(0)
reps = 9
N, BL = 4096, 65536
TARGETS = (256, 4096, 32768, BL)


def timed(fn):
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


def wall(fn):
    fn()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[1]


def case(kind):
    src = torch.empty(N * BL, dtype=torch.uint8, device=dev)
    eng.generate(kind, src, BL, N)
    stride = S.slot_stride(BL, 8)
    slots = torch.empty(N * stride, dtype=torch.uint8, device=dev)
    flen = torch.zeros(N, dtype=torch.int32, device=dev)
    eng.compress_batch_device(src, N, BL, slots, stride, flen)
    eng.synchronize()
    boff = torch.arange(N, dtype=torch.int64, device=dev) * stride
    res = torch.zeros(N, dtype=torch.int32, device=dev)
    full = torch.empty(N * BL, dtype=torch.uint8, device=dev)
    at = torch.arange(N + 1, dtype=torch.int64, device=dev) * BL
    rec = {"kind": kind, "blocks": N, "block": BL, "compressed_bytes": int(flen.sum().item()), "device": [], "host": []}
    ms = timed(lambda: eng.decompress_batch_device(slots, N * stride, boff, N, full, at, res))
    assert res.cpu().tolist() == [BL] * N and torch.equal(full, src)
    rec["full_decode_ms"] = ms
    rec["full_decode_GBps"] = N * BL / ms / 1e6
    for t in TARGETS:
        out = torch.empty(N * t, dtype=torch.uint8, device=dev)
        off = torch.arange(N + 1, dtype=torch.int64, device=dev) * t
        tgt = torch.full((N,), t, dtype=torch.int32, device=dev)
        ms = timed(lambda: eng.decompress_partial_device(slots, N * stride, boff, N, out, off, tgt, res))
        assert res.cpu().tolist() == [t] * N and torch.equal(out.view(N, t), src.view(N, BL)[:, :t])
        rec["device"].append({"target": t, "ms": ms, "prefix_GBps": N * t / ms / 1e6, "full_over_partial": rec["full_decode_ms"] / ms})
    # the host forms: the dense chain in host memory
    dense = torch.empty(int(flen.sum().item()), dtype=torch.uint8, device=dev)
    doff = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    eng.compact_device(slots, stride, flen, N, dense, dense.numel(), doff)
    eng.synchronize()
    framed = dense.cpu().numpy().tobytes()
    raw = src.cpu().numpy()
    ms = wall(lambda: eng.decompress_batch(framed))
    rec["host_full_decode_ms"] = ms
    rec["host_full_decode_GBps"] = N * BL / ms / 1e6
    for t in TARGETS:
        got = []
        ms = wall(lambda: got.append(eng.decompress_partial(framed, t)))
        data, blen = got[-1]
        assert blen == [t] * N and data == raw.reshape(N, BL)[:, :t].tobytes()
        rec["host"].append({"target": t, "ms": ms, "prefix_GBps": N * t / ms / 1e6, "full_over_partial": rec["host_full_decode_ms"] / ms})
    return rec


out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "partial_rate.json")
record = {"what": "partial decode: time per call and prefix bytes per second, device call and host form", "reps": reps,
          "cases": [case("lzsynth"), case("text")]}
print(json.dumps(record))
with open(out_path, "w") as f:
    json.dump(record, f, indent=1)
    f.write("\n")
eng.close()
