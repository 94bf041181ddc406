"""Development aid: high-compression dictionary batches (mi355lz4_compress_hcdict_device, levels 1, 3, 6 and 9) beside the same
records through mi355lz4_compress_dict_device (level 0, the reference-exact parse) and through mi355lz4_compress_batch_device at
the same level without a dictionary.  scripts/dict_rate.py's two workloads: 16384 text records of 4 KiB and 2560 of 64 KiB against
one 64 KiB dictionary of the same generator's text.  Every call is device-resident and event-timed on the engine's stream, the
median of 5 calls after one warm-up call.  One JSON record per workload, written to profiles/hcdict_rate.json (or the path given
as the first argument).

The driver itself never touches the GPU: every workload runs in a child process of its own under `timeout`, and the first child
that fails ends the run.
    python3 scripts/hcdict_rate.py [OUT.json] [CASE ...]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICT = 65536
LEVELS = (1, 3, 6, 9)
CASES = {"4KiB": (4096, 16384, 5), "64KiB": (65536, 2560, 5)}
STEP_SECONDS = 240


def step(case):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "streamly-lz4_amd"))
    import torch
    import streamly_lz4_amd as S

    dev = "cuda:0"
    eng = S.Engine(0)
    bl, n, reps = CASES[case]

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

    src = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    eng.generate("text", src, bl, n)
    d = torch.empty(DICT, dtype=torch.uint8, device=dev)
    eng.generate("text", d, bl, DICT // bl, first_block=n + 7)
    stride = S.slot_stride(bl, 8)
    slots = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    flen = torch.zeros(n, dtype=torch.int32, device=dev)
    out = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    boff = torch.arange(n, dtype=torch.int64, device=dev) * stride
    ooff = torch.arange(n + 1, dtype=torch.int64, device=dev) * bl
    rec = {"kind": "text", "block": bl, "blocks": n, "dictionary": DICT, "input_bytes": n * bl, "reps": reps,
           "device": torch.cuda.get_device_name(0)}

    def note(name, ms):
        eng.synchronize()
        size = int(flen.sum().item()) - 8 * n
        rec.update({name + "_compressed_bytes": size, name + "_compress_ms": ms, name + "_compress_GBps": n * bl / ms / 1e6,
                    name + "_ratio": n * bl / size})

    cs = S.CompressStreams(eng, 1)
    cs.load_dict(0, d, DICT)
    note("dict_level0", timed(lambda: eng.compress_dict_device(cs, 0, src, n, bl, slots, stride, flen)))
    cs.close()
    hd = S.HcDict(eng)
    rec["hcdict_load_ms"] = timed(lambda: hd.load(d, DICT))
    for lv in LEVELS:
        eng.set_compression_level(lv)
        note("hcdict_level%d" % lv, timed(lambda: eng.compress_hcdict_device(hd, src, n, bl, slots, stride, flen)))
        eng.set_compression_level(0)
        eng.decompress_dict_device(slots, n * stride, boff, n, d, DICT, out, ooff, res)
        eng.synchronize()
        rec["hcdict_level%d_decodes" % lv] = bool(torch.equal(out, src)) and res.tolist() == [bl] * n
        eng.set_compression_level(lv)
        note("batch_level%d" % lv, timed(lambda: eng.compress_batch_device(src, n, bl, slots, stride, flen)))
    eng.set_compression_level(0)
    hd.close()
    eng.close()
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hcdict_rate.json")
    records = {}
    for case in (sys.argv[2:] or list(CASES)):
        r = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", case],
                           capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not lines:
            print("step %s ended with status %d; nothing more is started\n%s\n%s" % (case, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            sys.exit(1)
        records[case] = json.loads(lines[-1][7:])
        print(case, json.dumps(records[case]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(records, f, indent=1)
    print(json.dumps(records))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        step(sys.argv[2])
    else:
        main()
