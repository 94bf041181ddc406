"""Development aid: level 0 against a prepared dictionary by the wave encoder (mi355lz4_compress_fastdict_device) beside the other
ways to compress the same records, all timed in one session: mi355lz4_compress_batch_device (no dictionary),
mi355lz4_compress_dict_device (level 0, the reference's bytes), mi355lz4_compress_hcdict_device at level 3, and the new call at
MI355LZ4_FASTDICT_WAVES 4, 8 and 16; and mi355lz4_hcdict_load of 64 KiB.  The shapes are scripts/dict_rate.py's:
  N text records of 4 KiB and of 64 KiB against one 64 KiB dictionary of the same generator's text.
Every call is device-resident and event-timed on the engine's stream: one warm-up call, then `reps` calls; a record holds all the
times, their median and minimum, and the call's ratio.  "faster_than_dict" is the feature's condition: the new call's median at
the default grid below the FASTEST of compress_dict_device's calls of the same session.  Every block of the new call is decoded
with the dictionary and compared with its source.
One case per run, merged into the output file, so that each runs under a time limit of its own:
    timeout -k 10 300 python3 scripts/fastdict_rate.py OUT.json 4KiB COMMIT && timeout -k 10 300 python3 scripts/fastdict_rate.py OUT.json 64KiB COMMIT
OUT.json defaults to profiles/fastdict_rate.json."""
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
KNOB = "MI355LZ4_FASTDICT_WAVES"


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


def rates(bl, n, reps):
    src = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    eng.generate("text", src, bl, n)
    d = torch.empty(DICT, dtype=torch.uint8, device=dev)
    eng.generate("text", d, bl, max(DICT // bl, 1), first_block=n + 7)
    cs = S.CompressStreams(eng, 1)
    cs.load_dict(0, d, DICT)
    hd = S.HcDict(eng)
    rec = {"kind": "text", "block": bl, "blocks": n, "dictionary": DICT, "input_bytes": n * bl, "reps": reps, "calls": {}}
    ts = timed(lambda: hd.load(d, DICT), reps)
    rec["hcdict_load_ms"] = sorted(ts)[len(ts) // 2]
    stride = S.slot_stride(bl, 8)
    slots = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    flen = torch.zeros(n, dtype=torch.int32, device=dev)

    def fast():
        eng.compress_fastdict_device(hd, src, n, bl, slots, stride, flen)

    def hc():
        eng.compress_hcdict_device(hd, src, n, bl, slots, stride, flen)

    calls = [("batch", lambda: eng.compress_batch_device(src, n, bl, slots, stride, flen), 0, None),
             ("dict", lambda: eng.compress_dict_device(cs, 0, src, n, bl, slots, stride, flen), 0, None),
             ("hcdict_level3", hc, 3, None),
             ("fastdict_w4", fast, 0, "4"), ("fastdict_w8", fast, 0, "8"), ("fastdict_w16", fast, 0, "16"),
             ("fastdict_default", fast, 0, None)]
    for name, fn, level, knob in calls:
        eng.set_compression_level(level)
        os.environ.pop(KNOB, None)
        if knob is not None:
            os.environ[KNOB] = knob
        ts = timed(fn, reps)
        eng.synchronize()
        os.environ.pop(KNOB, None)
        eng.set_compression_level(0)
        comp = int(flen.sum().item()) - 8 * n
        med = sorted(ts)[len(ts) // 2]
        rec["calls"][name] = {"ms": ts, "median_ms": med, "min_ms": min(ts), "GBps": n * bl / med / 1e6, "compressed_bytes": comp,
                              "ratio": n * bl / comp}
    # what the new call wrote last decodes with the dictionary
    out = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    boff = torch.arange(n, dtype=torch.int64, device=dev) * stride
    ooff = torch.arange(n + 1, dtype=torch.int64, device=dev) * bl
    eng.decompress_dict_device(slots, n * stride, boff, n, d, DICT, out, ooff, res)
    eng.synchronize()
    rec["fastdict_decodes"] = bool(torch.equal(out, src)) and res.tolist() == [bl] * n
    c = rec["calls"]
    rec["fastdict_over_batch"] = c["fastdict_default"]["median_ms"] / c["batch"]["median_ms"]
    rec["faster_than_dict"] = c["fastdict_default"]["median_ms"] < c["dict"]["min_ms"]
    hd.close()
    cs.close()
    return rec


CASES = {"4KiB": (4096, 16384, 5), "64KiB": (65536, 2560, 5)}
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fastdict_rate.json")
case = sys.argv[2] if len(sys.argv) > 2 else "4KiB"
records = {}
if os.path.exists(out_path):
    with open(out_path) as f:
        records = json.load(f)
records[case] = rates(*CASES[case])
print(case, json.dumps(records[case]), flush=True)
records["device"] = torch.cuda.get_device_name(0)
if len(sys.argv) > 3:
    records["commit"] = sys.argv[3]
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(records, f, indent=1)
eng.close()
