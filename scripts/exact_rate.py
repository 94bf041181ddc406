"""Development aid: what the reference-exact compress mode (mi355lz4_set_compress_exact) costs on the device.  One JSON
record, printed and written to profiles/exact_rate.json (or the path given as the first argument): device-resident rate
(GB/s of input), compressed bytes against level 0's independent blocks, and the pieces the last call speculated, kept and
redone, for
  65 536 x 64 KiB of text and of lzsynth (one linked stream of 4 GiB, the bench's shape),
  16 384 x 64 KiB of Python sources (the interpreter's own library, repeated), and
  160 x 64 KiB of text (the small-call shape; the reference takes 12.8 ms for it on one core).
Every call starts a new stream.  Times are the median of `reps` event-timed calls on the engine's stream after one
warm-up call (a call waits on the host for its verify step: the events span it).
    python3 scripts/exact_rate.py [OUT.json] [CASE ...]"""
import glob
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


def pysrc(nbytes):
    buf = bytearray()
    for f in sorted(glob.glob(os.path.join(os.path.dirname(os.__file__), "**", "*.py"), recursive=True)):
        buf += open(f, "rb").read()
        if len(buf) >= nbytes:
            break
    reps = -(-nbytes // len(buf))
    return np.frombuffer(bytes(buf) * reps, dtype=np.uint8)[:nbytes]


def rates(kind, bl, n, reps):
    if kind == "pysrc":
        src = torch.from_numpy(pysrc(n * bl).copy()).to(dev)
    else:
        src = torch.empty(n * bl, dtype=torch.uint8, device=dev)
        eng.generate(kind, src, bl, n)
    stride = S.slot_stride(bl, 8)
    slots = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    flen = torch.zeros(n, dtype=torch.int32, device=dev)
    rec = {"kind": kind, "block": bl, "blocks": n, "input_bytes": n * bl, "reps": reps}
    eng.set_compress_exact(False)
    eng.compress_batch_device(src, n, bl, slots, stride, flen)
    base = int(flen.sum().item()) - 8 * n
    eng.set_compress_exact(True)

    def call():
        eng.reset_compress_stream()
        eng.compress_batch_device(src, n, bl, slots, stride, flen)

    ms = timed(call, reps)
    comp = int(flen.sum().item()) - 8 * n
    pieces, spec, kept, redone = eng.exact_state()
    rec.update({"ms": ms, "GBps": n * bl / ms / 1e6, "compressed_bytes": comp, "level0_bytes": base,
                "size_vs_level0": comp / base, "pieces": pieces, "speculated": spec, "kept": kept, "redone": redone,
                "runin": os.environ.get("MI355LZ4_EXACT_RUNIN", "default"),
                "piece": os.environ.get("MI355LZ4_EXACT_PIECE", "default")})
    eng.set_compress_exact(False)
    del src, slots, flen
    torch.cuda.empty_cache()
    return rec


CASES = {
    "text_4GiB": ("text", 65536, 65536, 3),
    "lzsynth_4GiB": ("lzsynth", 65536, 65536, 3),
    "pysrc_1GiB": ("pysrc", 65536, 16384, 3),
    "text_160x64k": ("text", 65536, 160, 9),
}
only = sys.argv[2:] or list(CASES)
records = {}
for name in only:
    records[name] = rates(*CASES[name])
    print(name, json.dumps(records[name]), flush=True)
records["device"] = torch.cuda.get_device_name(0)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "exact_rate.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(records, f, indent=1)
print(json.dumps(records))
eng.close()
