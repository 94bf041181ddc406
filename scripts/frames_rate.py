"""Development aid: batches of standard LZ4 frames through mi355lz4_frames_load / mi355lz4_frames_decode, timed in
one session against what the library offered before and against the ceiling:
  (1) 2560 independent frames of 1 MiB of text in 64 KiB blocks;
  (2) 16384 linked frames of 64 KiB;
  (3) one linked frame of 1 GiB with a content checksum, verified and with MI355LZ4_FRAMES_SKIP_CONTENT_CHECKSUM.
Per shape: `decode` -- mi355lz4_frames_decode, device-resident and event-timed on the engine's stream; `load` -- mi355lz4_frames_load,
which waits for the stream, so it is timed on the host's clock; `batch` -- mi355lz4_decompress_batch_device on the same blocks
already indexed (4-byte headers, fixedUncomp 65536; linked for (3)): the ceiling; `host_frames` -- lz4FrameDecompress frame by
frame on the same bytes (host memory in, host memory out: what the parent commit offers), host-timed, over a sample of the
frames of (1) and (2) and scaled to all of them (the record says how many).  One warm-up call per form, then REPS rounds in which
the forms alternate; a record holds the times and their median.  Everything the frame calls wrote is compared with its source.
    timeout -k 10 900 python3 scripts/frames_rate.py [OUT.json [COMMIT]]
OUT.json defaults to profiles/frames_rate.json."""
import json
import os
import struct
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


def header(linked, csum):
    flg = 0x40 | (0 if linked else 0x20) | (4 if csum else 0)
    desc = bytes([flg, 0x40])
    return struct.pack("<I", 0x184D2204) + desc + bytes([(S.lib.slz4_xxh32(np.frombuffer(desc, dtype=np.uint8).ctypes.data_as(S._u8p), 2, 0) >> 8) & 0xFF])


def many_frames(n_frames, blocks_per_frame, linked, first_block):
    """n_frames frames of blocks_per_frame text blocks of 64 KiB each, assembled on the host from one compress_batch_device
    call's slots (a slot with a 4-byte header is a frame block as it stands): (buf, frame offsets, frame lengths, block
    offsets, source)"""
    n = n_frames * blocks_per_frame
    src = torch.empty(n * BL, dtype=torch.uint8, device=dev)
    eng.generate("text", src, BL, n, first_block=first_block)
    stride = S.slot_stride(BL, 4)
    slots = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    flen = torch.zeros(n, dtype=torch.int32, device=dev)
    eng.compress_batch_device(src, n, BL, slots, stride, flen, header_kind=4)
    eng.synchronize()
    hs, hl = slots.cpu().numpy().reshape(n, stride), flen.cpu().numpy()
    assert int(hl.min()) > 4 and int(hl.max()) - 4 < BL              # every block shrank: none would be stored
    head, end = np.frombuffer(header(linked, False), dtype=np.uint8), np.zeros(4, dtype=np.uint8)
    parts, f_off, f_len, b_off, pos = [], [], [], [], 0
    for f in range(n_frames):
        f_off.append(pos)
        parts.append(head)
        pos += head.size
        for k in range(f * blocks_per_frame, (f + 1) * blocks_per_frame):
            b_off.append(pos)
            parts.append(hs[k, :hl[k]])
            pos += int(hl[k])
        parts.append(end)
        pos += 4
        f_len.append(pos - f_off[-1])
    buf = np.concatenate(parts)
    del slots, hs
    return buf, f_off, f_len, b_off, src


def run_shape(name, buf, f_off, f_len, b_off, src, linked_batch, sample, flags_list=(0,)):
    n_frames, n_blocks = len(f_off), len(b_off)
    total = int(src.numel())
    dbuf = torch.from_numpy(buf).to(dev)
    d_off, d_len, d_boff = i64(f_off), i64(f_len), i64(b_off)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    out2 = torch.empty(total, dtype=torch.uint8, device=dev)
    res = torch.zeros(n_frames, dtype=torch.int64, device=dev)
    res32 = torch.zeros(n_blocks, dtype=torch.int32, device=dev)
    ooff_b = torch.arange(n_blocks + 1, dtype=torch.int64, device=dev) * BL
    rec = {"frames": n_frames, "blocks": n_blocks, "content_bytes": total, "frame_bytes": int(buf.size)}
    sample = min(sample, n_frames)
    pick = [int(x) for x in np.linspace(0, n_frames - 1, sample).astype(np.int64)]
    frames_host = [buf[f_off[i]:f_off[i] + f_len[i]].tobytes() for i in pick]

    def host_frames():
        for f in frames_host:
            S.lz4FrameDecompress(f, eng)

    for flags in flags_list:
        fr = S.Frames(eng)
        sizes = fr.load(dbuf, d_off, d_len, flags=flags)
        per = total // n_frames
        assert sizes == [per] * n_frames, sizes[:4]
        ooff = torch.arange(n_frames, dtype=torch.int64, device=dev) * per
        forms = {
            "decode": (lambda: fr.decode(out, ooff, res), "device"),
            "load": (lambda: fr.load(dbuf, d_off, d_len, flags=flags), "host"),
            "batch": (lambda: eng.decompress_batch_device(dbuf, buf.size, d_boff, n_blocks, out2, ooff_b, res32, header_kind=4,
                                                          fixed_uncomp=BL, linked=linked_batch), "device" if not linked_batch else "host"),
        }
        if flags == flags_list[0]:
            forms["host_frames"] = (host_frames, "host")
        r = alternate(forms)
        fr.decode(out, ooff, res)
        eng.synchronize()
        r["decodes"] = bool(torch.equal(out, src)) and res.cpu().tolist() == sizes and bool(torch.equal(out2, src))
        if "host_frames" in r:
            r["host_frames"]["sampled_frames"] = sample
            r["host_frames"]["scaled_to_all_ms"] = r["host_frames"]["median_ms"] * n_frames / sample
        r["decode_GBps"] = total / r["decode"]["median_ms"] / 1e6
        r["load_plus_decode_GBps"] = total / (r["decode"]["median_ms"] + r["load"]["median_ms"]) / 1e6
        r["batch_GBps"] = total / r["batch"]["median_ms"] / 1e6
        rec["flags_%d" % flags] = r
        fr.close()
    print(name, json.dumps(rec), flush=True)
    return rec


record = {"shape": {"block": BL, "kind": "text", "reps": REPS}}

buf, f_off, f_len, b_off, src = many_frames(2560, 16, False, 0)
record["independent_2560x1MiB"] = run_shape("independent", buf, f_off, f_len, b_off, src, False, 64)
del buf, src
torch.cuda.empty_cache()

buf, f_off, f_len, b_off, src = many_frames(16384, 1, True, 100000)
record["linked_16384x64KiB"] = run_shape("linked-small", buf, f_off, f_len, b_off, src, False, 512)
del buf, src
torch.cuda.empty_cache()

# one linked frame of 1 GiB, written by the library's own frame writer (linked blocks, content checksum)
n = 16384
src = torch.empty(n * BL, dtype=torch.uint8, device=dev)
eng.generate("text", src, BL, n, first_block=200000)
eng.synchronize()
frame = S.lz4FrameCompress(src.cpu().numpy().tobytes(), eng, linkedBlocks=True, contentChecksum=True)
buf = np.frombuffer(frame, dtype=np.uint8)
b_off, pos = [], 7
while True:
    word = struct.unpack_from("<I", frame, pos)[0]
    if word == 0:
        break
    assert not word >> 31
    b_off.append(pos)
    pos += 4 + word
del frame
record["linked_1x1GiB"] = run_shape("linked-1GiB", buf, [0], [buf.size], b_off, src, True, 1,
                                    flags_list=(0, S.FRAMES_SKIP_CONTENT_CHECKSUM))

record["device"] = torch.cuda.get_device_name(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "frames_rate.json")
if len(sys.argv) > 2:
    record["commit"] = sys.argv[2]
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(record, f, indent=1)
eng.close()
