"""Development aid: shared-dictionary batches (mi355lz4_compress_dict_device / mi355lz4_decompress_dict_device) beside the same
blocks through mi355lz4_compress_batch_device / mi355lz4_decompress_batch_device.  One JSON record per shape, printed and
written to profiles/dict_rate.json (or the path given as the first argument):
  N text records of 4 KiB and of 64 KiB against one 64 KiB dictionary of the same generator's text.
Every call is device-resident and event-timed on the engine's stream, the median of `reps` calls after one warm-up call.  A
record holds the compressed size and the time of both compress calls and of both decode calls (each decoding what its own
compress call wrote), and whether the dictionary blocks decode to their sources.
    python3 scripts/dict_rate.py [OUT.json] [CASE ...]"""
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
    ts.sort()
    return ts[len(ts) // 2]


def rates(bl, n, reps):
    # the generator works in blocks of one length: the dictionary is 64 KiB of its text from block indices behind the records'
    src = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    eng.generate("text", src, bl, n)
    d = torch.empty(DICT, dtype=torch.uint8, device=dev)
    eng.generate("text", d, bl, DICT // bl, first_block=n + 7)
    cs = S.CompressStreams(eng, 1)
    cs.load_dict(0, d, DICT)
    stride = S.slot_stride(bl, 8)
    rec = {"kind": "text", "block": bl, "blocks": n, "dictionary": DICT, "input_bytes": n * bl, "reps": reps}
    boff = torch.arange(n, dtype=torch.int64, device=dev) * stride
    ooff = torch.arange(n + 1, dtype=torch.int64, device=dev) * bl
    for name in ("dict", "batch"):
        slots = torch.empty(n * stride, dtype=torch.uint8, device=dev)
        flen = torch.zeros(n, dtype=torch.int32, device=dev)
        out = torch.empty(n * bl, dtype=torch.uint8, device=dev)
        res = torch.zeros(n, dtype=torch.int32, device=dev)
        if name == "dict":
            def comp():
                eng.compress_dict_device(cs, 0, src, n, bl, slots, stride, flen)

            def dec():
                eng.decompress_dict_device(slots, n * stride, boff, n, d, DICT, out, ooff, res)
        else:
            def comp():
                eng.compress_batch_device(src, n, bl, slots, stride, flen)

            def dec():
                eng.decompress_batch_device(slots, n * stride, boff, n, out, ooff, res)
        cms = timed(comp, reps)
        eng.synchronize()
        dms = timed(dec, reps)
        eng.synchronize()
        rec.update({name + "_compressed_bytes": int(flen.sum().item()) - 8 * n,
                    name + "_compress_ms": cms, name + "_compress_GBps": n * bl / cms / 1e6,
                    name + "_decompress_ms": dms, name + "_decompress_GBps": n * bl / dms / 1e6,
                    name + "_decodes": bool(torch.equal(out, src)) and res.tolist() == [bl] * n})
        del slots, out
    rec["ratio_dict"] = n * bl / rec["dict_compressed_bytes"]
    rec["ratio_batch"] = n * bl / rec["batch_compressed_bytes"]
    cs.close()
    del src
    torch.cuda.empty_cache()
    return rec


CASES = {"4KiB": (4096, 16384, 5), "64KiB": (65536, 2560, 5)}
records = {}
for name in (sys.argv[2:] or list(CASES)):
    records[name] = rates(*CASES[name])
    print(name, json.dumps(records[name]), flush=True)
records["device"] = torch.cuda.get_device_name(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dict_rate.json")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(records, f, indent=1)
print(json.dumps(records))
eng.close()
