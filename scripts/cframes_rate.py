"""Development aid: writing batches of standard LZ4 frames through mi355lz4_cframes_compress, timed in one session
against the ceiling and against what the library offered before, on text in 64 KiB blocks:
  (1) 2560 inputs of 1 MiB, independent frames;
  (2) 16384 inputs of 64 KiB, linked frames;
  (3) one input of 1 GiB, one linked frame -- without and with a content checksum (four lanes hash the whole input).
Per shape: `cframes` -- mi355lz4_cframes_compress, device-resident and event-timed on the engine's stream, the writer's scratch
reserved ahead; `batch` -- mi355lz4_compress_batch_device on the same blocks (4-byte headers, the same linked switch): the ceiling,
and the difference is what the frame layer costs; `host_writer` -- lz4FrameCompress frame by frame (host memory in, host memory
out: what the parent commit offers), host-timed over a sample of the inputs and scaled to all of them (the record says how
many).  One warm-up call per form, then REPS rounds in which the forms alternate; a record holds the times and their median.
Every frame written is read back through mi355lz4_frames_load / _decode and compared with its source.
    timeout -k 10 900 python3 scripts/cframes_rate.py [OUT.json [COMMIT]]
OUT.json defaults to profiles/cframes_rate.json."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "streamly-lz4_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import streamly_lz4_amd as S  # noqa: E402

dev = "cuda:0"
eng = S.Engine(0)
BL, REPS = 65536, 5


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64))).to(dev)


def stats(v):
    return {"ms": v, "median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)}


def alternate(forms, reps=REPS):
    """forms: {name: (fn, "device" | "host")}: device forms are event-timed on the engine's stream, host forms on the host's clock
    around the call and a synchronise"""
    for fn, _ in forms.values():
        fn()
    eng.synchronize()
    ts = {k: [] for k in forms}
    for _ in range(reps):
        for name, (fn, how) in forms.items():
            if how == "device":
                a, b = S.Event(), S.Event()
                eng.record(a)
                fn()
                eng.record(b)
                eng.synchronize()
                ts[name].append(S.Engine.elapsed_ms(a, b))
            else:
                eng.synchronize()
                t0 = time.perf_counter()
                fn()
                eng.synchronize()
                ts[name].append(1000.0 * (time.perf_counter() - t0))
    return {k: stats(v) for k, v in ts.items()}


def run_shape(name, n_inputs, blocks_per_input, linked, first_block, sample, flag_sets):
    n_blocks = n_inputs * blocks_per_input
    per = blocks_per_input * BL
    total = n_blocks * BL
    src = torch.empty(total, dtype=torch.uint8, device=dev)
    eng.generate("text", src, BL, n_blocks, first_block=first_block)
    eng.synchronize()
    rec = {"inputs": n_inputs, "blocks": n_blocks, "input_bytes": total, "linked": bool(linked)}
    in_off, in_len = i64(np.arange(n_inputs) * per), i64([per] * n_inputs)
    stride = S.slot_stride(BL, 4)
    slots = torch.empty(n_blocks * stride, dtype=torch.uint8, device=dev)
    flen32 = torch.zeros(n_blocks, dtype=torch.int32, device=dev)
    w = S.FrameWriter(eng)
    w.reserve(n_inputs, per, total, 4)
    sample = min(sample, n_inputs)
    pick = [int(x) for x in np.linspace(0, n_inputs - 1, sample).astype(np.int64)]
    host_inputs = [src[i * per:(i + 1) * per].cpu().numpy().tobytes() for i in pick]
    for flags in flag_sets:
        flags |= S.CFRAMES_LINKED if linked else 0
        bound = S.cframes_bound(per, 4, flags)
        dst = torch.empty(n_inputs * bound, dtype=torch.uint8, device=dev)
        dst_off, dst_cap = i64(np.arange(n_inputs) * bound), i64([bound] * n_inputs)
        flen = torch.zeros(n_inputs, dtype=torch.int64, device=dev)

        def cframes():
            w.compress(src, in_off, in_len, per, total, dst, dst_off, dst_cap, flen, block_size_id=4, flags=flags)

        def batch():
            eng.set_linked_compress(bool(linked))
            eng.compress_batch_device(src, n_blocks, BL, slots, stride, flen32, header_kind=4)
            eng.set_linked_compress(False)

        def host_writer():
            for d in host_inputs:
                S.lz4FrameCompress(d, eng, linkedBlocks=bool(linked), contentChecksum=bool(flags & S.CFRAMES_CONTENT_CHECKSUM),
                                   contentSize=bool(flags & S.CFRAMES_CONTENT_SIZE), blockChecksum=bool(flags & S.CFRAMES_BLOCK_CHECKSUM))

        forms = {"cframes": (cframes, "device"), "batch": (batch, "device")}
        if flags == flag_sets[0] | (S.CFRAMES_LINKED if linked else 0):
            forms["host_writer"] = (host_writer, "host")
        r = alternate(forms)
        # what was written reads back to the source
        cframes()
        eng.synchronize()
        lens = flen.cpu().numpy()
        assert int(lens.min()) > 0, lens[:4]
        fr = S.Frames(eng)
        sizes = fr.load(dst, dst_off, flen)
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        res = torch.zeros(n_inputs, dtype=torch.int64, device=dev)
        fr.decode(out, in_off, res)
        eng.synchronize()
        r["reads_back"] = sizes == [per] * n_inputs and res.cpu().tolist() == sizes and bool(torch.equal(out, src))
        fr.close()
        del out
        r["frame_bytes"] = int(lens.sum())
        if "host_writer" in r:
            r["host_writer"]["sampled_inputs"] = sample
            r["host_writer"]["scaled_to_all_ms"] = r["host_writer"]["median_ms"] * n_inputs / sample
        r["cframes_GBps"] = total / r["cframes"]["median_ms"] / 1e6
        r["batch_GBps"] = total / r["batch"]["median_ms"] / 1e6
        r["frame_layer_ms"] = r["cframes"]["median_ms"] - r["batch"]["median_ms"]
        rec["flags_%d" % flags] = r
        del dst
        torch.cuda.empty_cache()
    w.close()
    print(name, json.dumps(rec), flush=True)
    return rec


record = {"shape": {"block": BL, "kind": "text", "reps": REPS}}
CS = S.CFRAMES_CONTENT_SIZE
record["independent_2560x1MiB"] = run_shape("independent", 2560, 16, False, 0, 64, (CS,))
torch.cuda.empty_cache()
record["linked_16384x64KiB"] = run_shape("linked-small", 16384, 1, True, 100000, 512, (CS,))
torch.cuda.empty_cache()
record["linked_1x1GiB"] = run_shape("linked-1GiB", 1, 16384, True, 200000, 1, (CS, CS | S.CFRAMES_CONTENT_CHECKSUM))

record["device"] = torch.cuda.get_device_name(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cframes_rate.json")
if len(sys.argv) > 2:
    record["commit"] = sys.argv[2]
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(record, f, indent=1)
eng.close()
