"""Development aid: fixed-size output pages (mi355lz4_compress_pages_device) beside the same records through
mi355lz4_compress_batch_device.  One JSON record per shape, printed and written to profiles/pages_rate.json (or the path given as
the first argument):
  16384 text records of 4 KiB into pages of 1 KiB, 2560 text records of 64 KiB into pages of 4 KiB.
Every call is device-resident and event-timed on the engine's stream, the median of `reps` calls after one warm-up call.  A record
holds the time of both calls, the pages written, the bytes they hold and their fill, and whether the chains consumed their inputs.
A chain is serial per input: the pages call's parallelism is the number of records.
    python3 scripts/pages_rate.py [OUT.json] [CASE ...]"""
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


def rates(bl, n, page, reps):
    src = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    eng.generate("text", src, bl, n)
    # a page that leaves input behind holds at least (T - 1) - (T + 240) / 256 bytes: enough pages for the worst case
    max_pages = -(-bl // ((page - 1) - (page + 240) // 256))
    hk, stride = 8, 8 + page
    rec = {"kind": "text", "block": bl, "blocks": n, "page": page, "max_pages": max_pages, "input_bytes": n * bl, "reps": reps}
    off = torch.arange(n, dtype=torch.int64, device=dev) * bl
    ln = torch.full((n,), bl, dtype=torch.int32, device=dev)
    ps = torch.full((n,), page, dtype=torch.int32, device=dev)
    pages = torch.empty(n * max_pages * stride, dtype=torch.uint8, device=dev)
    sl = torch.zeros(n * max_pages, dtype=torch.int32, device=dev)
    cl = torch.zeros(n * max_pages, dtype=torch.int32, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    cons = torch.zeros(n, dtype=torch.int32, device=dev)
    pms = timed(lambda: eng.compress_pages_device(src, off, ln, n, ps, max_pages, pages, stride, sl, cl, cnt, cons, header_kind=hk), reps)
    eng.synchronize()
    total_pages = int(cnt.sum().item())
    written = torch.arange(max_pages, device=dev).repeat(n) < cnt.repeat_interleave(max_pages)
    comp_bytes = int(cl[written].to(torch.int64).sum().item())
    rec.update({"pages_ms": pms, "pages_GBps": n * bl / pms / 1e6, "pages_written": total_pages, "pages_compressed_bytes": comp_bytes,
                "pages_fill": comp_bytes / max(total_pages * page, 1), "pages_consumed_all": bool((cons == bl).all().item())})
    del pages
    bstride = S.slot_stride(bl, 8)
    slots = torch.empty(n * bstride, dtype=torch.uint8, device=dev)
    flen = torch.zeros(n, dtype=torch.int32, device=dev)
    bms = timed(lambda: eng.compress_batch_device(src, n, bl, slots, bstride, flen), reps)
    eng.synchronize()
    rec.update({"batch_ms": bms, "batch_GBps": n * bl / bms / 1e6, "batch_compressed_bytes": int(flen.sum().item()) - 8 * n})
    rec["ratio_pages"] = n * bl / max(comp_bytes, 1)
    rec["ratio_batch"] = n * bl / rec["batch_compressed_bytes"]
    del slots, src
    torch.cuda.empty_cache()
    return rec


CASES = {"4KiB_into_1KiB": (4096, 16384, 1024, 5), "64KiB_into_4KiB": (65536, 2560, 4096, 5)}
records = {}
for name in (sys.argv[2:] or list(CASES)):
    records[name] = rates(*CASES[name])
    print(name, json.dumps(records[name]), flush=True)
records["device"] = torch.cuda.get_device_name(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pages_rate.json")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(records, f, indent=1)
print(json.dumps(records))
eng.close()
