"""Development aid: many linked decode streams continued across calls (mi355lz4_decompress_dstreams_device and its host form)
beside the same blocks through ONE mi355lz4_decompress_streams_device call.  One JSON record per shape, printed and written
to profiles/dstreams_rate.json (or the path given as the first argument):
  S streams x P blocks of 64 KiB of text per stream per call, S in {2560, 10240}, P in {1, 4}.
The streams are linked ones (the engine's linked compressor over every stream's blocks).  The device calls are
device-resident and event-timed on the engine's stream, the median of `reps` calls after one warm-up call; every dstreams call
starts from slots that hold the block in front of the call's first (set_dict), so every block needs its dictionary.  The host
form is timed on the wall clock around the synchronous call.
    python3 scripts/dstreams_rate.py [OUT.json] [CASE ...]"""
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
BL = 65536


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


def rates(streams, per, reps):
    # every stream: per + 1 blocks compressed as one linked stream; block 0 is the dictionary the slots start from
    n_all = streams * (per + 1)
    src = torch.empty(n_all * BL, dtype=torch.uint8, device=dev)
    eng.generate("text", src, BL, n_all)
    stride = S.slot_stride(BL, 8)
    slots = torch.empty(n_all * stride, dtype=torch.uint8, device=dev)
    flen = torch.zeros(n_all, dtype=torch.int32, device=dev)
    cs = S.CompressStreams(eng, streams)
    eng.compress_streams_device(cs, src, n_all, BL, list(range(0, n_all + 1, per + 1)), list(range(streams)), slots, stride, flen)
    eng.synchronize()
    cs.close()
    n = streams * per
    blocks = [s * (per + 1) + 1 + k for s in range(streams) for k in range(per)]
    boff = torch.tensor(blocks, dtype=torch.int64, device=dev) * stride
    ooff = torch.arange(n + 1, dtype=torch.int64, device=dev) * BL
    out = torch.empty(n * BL, dtype=torch.uint8, device=dev)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    first = list(range(0, n + 1, per))
    slot_of = list(range(streams))
    ds = S.DecompressStreams(eng, streams)
    rec = {"kind": "text", "block": BL, "streams": streams, "blocks_per_stream": per, "output_bytes": n * BL, "reps": reps,
           "compressed_bytes": int(flen.sum().item()) - 8 * n_all}

    def seed():
        for s in range(streams):
            ds.set_dict(s, src[s * (per + 1) * BL:], BL)

    def call():
        eng.decompress_dstreams_device(ds, slots, n_all * stride, boff, n, first, slot_of, out, ooff, res)

    seed()
    call()
    eng.synchronize()
    want = torch.cat([src[b * BL:(b + 1) * BL] for b in blocks[:: max(1, n // 64)]])
    got = torch.cat([out[i * BL:(i + 1) * BL] for i in range(0, n, max(1, n // 64))])
    rec["decodes"] = bool(torch.equal(want, got)) and res.tolist() == [BL] * n
    # (a repeated call finds its slots holding the call's last blocks instead of the blocks in front: the first block of
    # every stream then gives an error code after the same walk of its tokens; seeding inside the timed region would time
    # `streams` small launches instead)
    ms = timed(call, reps)
    rec.update({"dstreams_ms": ms, "dstreams_GBps": n * BL / ms / 1e6})
    # the same blocks, whole streams in one decompress_streams_device call (dictionary block included, so every block decodes)
    boff_all = torch.arange(n_all, dtype=torch.int64, device=dev) * stride
    ooff_all = torch.arange(n_all + 1, dtype=torch.int64, device=dev) * BL
    out_all = torch.empty(n_all * BL, dtype=torch.uint8, device=dev)
    res_all = torch.zeros(n_all, dtype=torch.int32, device=dev)
    sf = torch.arange(0, n_all + 1, per + 1, dtype=torch.int32, device=dev)

    def whole():
        eng.decompress_streams_device(slots, n_all * stride, boff_all, n_all, sf, streams, out_all, ooff_all, res_all)

    wms = timed(whole, reps)
    rec.update({"streams_call_ms": wms, "streams_call_GBps": n_all * BL / wms / 1e6, "streams_call_blocks": n_all})
    # host form: the call's blocks as one dense chain in host memory
    fl = flen.tolist()
    host = slots.cpu().numpy()
    framed = b"".join(host[b * stride:b * stride + fl[b]].tobytes() for b in blocks)
    seed()
    eng.synchronize()
    t0 = time.perf_counter()
    data, blen = eng.decompress_dstreams(framed, first, ds, slots=slot_of)
    hms = (time.perf_counter() - t0) * 1e3
    rec.update({"host_ms": hms, "host_GBps": n * BL / hms / 1e6, "host_decodes": blen == [BL] * n and len(data) == n * BL})
    ds.close()
    del src, slots, out, out_all
    torch.cuda.empty_cache()
    return rec


CASES = {"2560x1": (2560, 1, 5), "2560x4": (2560, 4, 5), "10240x1": (10240, 1, 5), "10240x4": (10240, 4, 5)}
records = {}
for name in (sys.argv[2:] or list(CASES)):
    records[name] = rates(*CASES[name])
    print(name, json.dumps(records[name]), flush=True)
records["device"] = torch.cuda.get_device_name(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dstreams_rate.json")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(records, f, indent=1)
print(json.dumps(records))
eng.close()
