"""Development aid: fast fixed-size output pages against a prepared dictionary (mi355lz4_compress_pages_fastdict_device) beside the
same pages without a dictionary (mi355lz4_compress_pages_fast_device) and the dictionary batch without pages
(mi355lz4_compress_fastdict_device) on the same records, timed in the same session.  One case per run -- each workload in a process
of its own -- merged into profiles/dictpages_rate.json (or the path given as the first argument):
  4KiB_into_1KiB: 16384 text records of 4 KiB into pages of 1 KiB;  64KiB_into_4KiB: 2560 text records of 64 KiB into 4 KiB;
both against a 64 KiB dictionary of the same generator (scripts/fastdict_rate.py's).
Every call is device-resident and event-timed on the engine's stream: one warm-up call, then `reps` timed calls; all times are kept,
with their median and their minimum.  A record holds, per call, the pages written, the bytes they hold, their fill and ratio and
whether the chains consumed their inputs, and the page count ratio with / without the dictionary.  The pages of both page calls are
decoded and compared with the input.  No rate is a condition of anything.
    python3 scripts/dictpages_rate.py [OUT.json] [CASE]"""
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
DICT = 65536


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        a, b = S.Event(), S.Event()
        eng.record(a)
        fn()
        eng.record(b)
        ts.append(S.Engine.elapsed_ms(a, b))
    return ts


def rates(bl, n, page, reps):
    src = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    eng.generate("text", src, bl, n)
    d = torch.empty(DICT, dtype=torch.uint8, device=dev)
    eng.generate("text", d, bl, max(DICT // bl, 1), first_block=n + 7)
    hd = S.HcDict(eng)
    hd.load(d, DICT)
    # a page that leaves input behind holds at least (T - 1) - (T + 240) / 256 bytes: enough pages for the worst case
    max_pages = -(-bl // ((page - 1) - (page + 240) // 256))
    hk, stride = 8, 8 + page
    rec = {"kind": "text", "block": bl, "blocks": n, "page": page, "dictionary": DICT, "max_pages": max_pages, "input_bytes": n * bl,
           "reps": reps, "calls": {}}
    off = torch.arange(n, dtype=torch.int64, device=dev) * bl
    ln = torch.full((n,), bl, dtype=torch.int32, device=dev)
    ps = torch.full((n,), page, dtype=torch.int32, device=dev)
    pages = torch.empty(n * max_pages * stride, dtype=torch.uint8, device=dev)
    sl = torch.zeros(n * max_pages, dtype=torch.int32, device=dev)
    cl = torch.zeros(n * max_pages, dtype=torch.int32, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    cons = torch.zeros(n, dtype=torch.int32, device=dev)
    calls = [("pages_fast", None, lambda: eng.compress_pages_fast_device(src, off, ln, n, ps, max_pages, pages, stride, sl, cl, cnt, cons,
                                                                         header_kind=hk, accel=1)),
             ("pages_fastdict", d, lambda: eng.compress_pages_fastdict_device(hd, src, off, ln, n, ps, max_pages, pages, stride, sl, cl, cnt,
                                                                              cons, header_kind=hk, accel=1))]
    for name, dic, fn in calls:
        ts = timed(fn, reps)
        eng.synchronize()
        total_pages = int(cnt.sum().item())
        written = torch.arange(max_pages, device=dev).repeat(n) < cnt.repeat_interleave(max_pages)
        comp_bytes = int(cl[written].to(torch.int64).sum().item())
        med = sorted(ts)[len(ts) // 2]
        rec["calls"][name] = {"ms": ts, "median_ms": med, "min_ms": min(ts), "GBps": n * bl / med / 1e6, "pages_written": total_pages,
                              "compressed_bytes": comp_bytes, "fill": comp_bytes / max(total_pages * page, 1),
                              "ratio": n * bl / max(comp_bytes, 1), "consumed_all": bool((cons == bl).all().item())}
        # the call's pages are ordinary blocks: decoded where they lie (with the dictionary, where there is one), an input's pages
        # concatenate to it
        idx = torch.nonzero(written).flatten()
        boff = idx.to(torch.int64) * stride
        lens = sl[idx].to(torch.int64)
        starts = torch.cumsum(lens, 0) - lens
        ooff = torch.cat([starts, lens.sum().reshape(1)])
        out = torch.zeros(n * bl, dtype=torch.uint8, device=dev)
        res = torch.zeros(idx.numel(), dtype=torch.int32, device=dev)
        if dic is None:
            eng.decompress_batch_device(pages, pages.numel(), boff, idx.numel(), out, ooff, res, header_kind=8, linked=False)
        else:
            eng.decompress_dict_device(pages, pages.numel(), boff, idx.numel(), dic, DICT, out, ooff, res)
        eng.synchronize()
        rec["calls"][name]["decodes"] = bool(torch.equal(out, src)) and bool((res.to(torch.int64) == lens).all().item())
        del out
    del pages
    bstride = S.slot_stride(bl, 8)
    slots = torch.empty(n * bstride, dtype=torch.uint8, device=dev)
    flen = torch.zeros(n, dtype=torch.int32, device=dev)
    ts = timed(lambda: eng.compress_fastdict_device(hd, src, n, bl, slots, bstride, flen), reps)
    eng.synchronize()
    comp = int(flen.sum().item()) - 8 * n
    med = sorted(ts)[len(ts) // 2]
    rec["calls"]["fastdict"] = {"ms": ts, "median_ms": med, "min_ms": min(ts), "GBps": n * bl / med / 1e6, "compressed_bytes": comp,
                                "ratio": n * bl / comp}
    c = rec["calls"]
    rec["page_count_ratio"] = c["pages_fastdict"]["pages_written"] / c["pages_fast"]["pages_written"]
    rec["fastdict_pages_over_fast_pages"] = c["pages_fastdict"]["median_ms"] / c["pages_fast"]["median_ms"]
    rec["fastdict_pages_over_fastdict"] = c["pages_fastdict"]["median_ms"] / c["fastdict"]["median_ms"]
    hd.close()
    return rec


CASES = {"4KiB_into_1KiB": (4096, 16384, 1024, 5), "64KiB_into_4KiB": (65536, 2560, 4096, 5)}
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dictpages_rate.json")
case = sys.argv[2] if len(sys.argv) > 2 else "4KiB_into_1KiB"
records = {}
if os.path.exists(out_path):
    with open(out_path) as f:
        records = json.load(f)
records[case] = rates(*CASES[case])
print(case, json.dumps(records[case]), flush=True)
records["device"] = torch.cuda.get_device_name(0)
records["note"] = "scripts/dictpages_rate.py, each workload in a process of its own; 5 event-timed calls after a warm-up call"
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(records, f, indent=1)
    f.write("\n")
eng.close()
