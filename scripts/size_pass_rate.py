"""Development aid: what the decoded-size pass (mi355lz4_decoded_size_device) costs, and what the host-buffer decode of
size-less blocks gains from it.  One JSON record, printed and written to profiles/size_pass_rate.json (or the path given as
the first argument):
  device  65 536 x 64 KiB blocks of lzsynth / text / random and 160 x 64 KiB lzsynth, headerKind 4: the size pass (ms, GB/s
          of compressed bytes read) next to mi355lz4_decompress_batch_device of the same blocks on the same stream;
  linked  2048 x 64 KiB blocks of one linked stream (lzsynth, text): how many the size pass leaves without a size;
  host    mi355lz4_decompress_batch, headerKind 4, cap = the exact total: 65 536 ragged blocks (1 .. 65 536 B) at
          fixedUncomp 64 KiB and 2048 blocks of <= 4 KiB at 4 MiB -- wall time of three calls after a warm-up and the device
          memory the call took (free memory before the first call minus after).
The host part uses nothing the parent of the size pass lacks, so the same file measures both sides of the change; the device
part is skipped where the library has no size pass.  Device times are the median of `reps` event-timed calls after a warm-up.
    python3 scripts/size_pass_rate.py [OUT.json] [device|host ...]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "streamly-lz4_amd"))
import torch  # noqa: E402
import streamly_lz4_amd as S  # noqa: E402

dev = "cuda:0"
eng = S.Engine(0)
reps = 9
HAVE = hasattr(S.lib, "mi355lz4_decoded_size_device") and hasattr(eng, "decoded_size_device")


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


def compressed(kind, bl, n, lens=None):
    """n blocks of `kind` compressed on the device, headerKind 4: (slots, stride, framedLen, blockOff, src)"""
    src = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    eng.generate(kind, src, bl, n)
    stride = S.slot_stride(bl, 4)
    slots = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    flen = torch.zeros(n, dtype=torch.int32, device=dev)
    eng.compress_batch_device(src, n, bl, slots, stride, flen, header_kind=4, src_len=lens)
    eng.synchronize()
    return slots, stride, flen, torch.arange(n, dtype=torch.int64, device=dev) * stride, src


def device_case(kind, bl, n):
    slots, stride, flen, boff, src = compressed(kind, bl, n)
    comp = int(flen.sum().item()) - 4 * n
    size = torch.zeros(n, dtype=torch.int32, device=dev)
    ooff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    dst = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    at = torch.arange(n + 1, dtype=torch.int64, device=dev) * bl
    rec = {"kind": kind, "block": bl, "blocks": n, "compressed_bytes": comp}
    rec["size_ms"] = timed(lambda: eng.decoded_size_device(slots, n * stride, boff, n, size, ooff, 4, bl))
    assert size.cpu().tolist() == [bl] * n and int(ooff[-1].item()) == n * bl, "sizes"
    rec["size_GBps_compressed"] = comp / rec["size_ms"] / 1e6
    rec["decode_ms"] = timed(lambda: eng.decompress_batch_device(slots, n * stride, boff, n, dst, at, res, 4, bl))
    assert res.cpu().tolist() == [bl] * n and torch.equal(dst, src), "round trip"
    rec["decode_GBps_out"] = n * bl / rec["decode_ms"] / 1e6
    rec["size_over_decode"] = rec["size_ms"] / rec["decode_ms"]
    return rec


def host_case(n, hi, F, seed):
    """ragged blocks of 1..hi bytes, dense headerKind-4 stream in host memory; three timed calls with cap = the exact total"""
    rng = np.random.default_rng(seed)
    lens_h = rng.integers(1, hi + 1, size=n).astype(np.int32)
    bl = 65536 if hi > 4096 else 4096
    slots, stride, flen, _, src = compressed("lzsynth", bl, n, torch.from_numpy(lens_h).to(dev))
    dense = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    doff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    eng.compact_device(slots, stride, flen, n, dense, n * stride, doff)
    eng.synchronize()
    framed = dense[: int(doff[-1].item())].cpu().numpy()
    want = np.concatenate([src[i * bl:i * bl + int(lens_h[i])].cpu().numpy() for i in range(0, n, max(1, n // 64))])
    del slots, dense, src
    torch.cuda.empty_cache()
    total = int(lens_h.astype(np.int64).sum())
    out = np.empty(total, dtype=np.uint8)
    blen = np.zeros(n, dtype=np.int32)
    out_len, got = C.c_size_t(), C.c_int()
    u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)

    heng = S.Engine(0)                                             # a fresh engine: what it reserves is this shape's

    def call():
        rc = S.lib.mi355lz4_decompress_batch(heng.ctx, framed.ctypes.data_as(u8p), framed.size, 4, F, 0, None, 0,
                                             out.ctypes.data_as(u8p), total, C.byref(out_len), blen.ctypes.data_as(i32p), n,
                                             C.byref(got))
        assert rc == 0 and out_len.value == total and got.value == n, (rc, out_len.value)

    free0 = torch.cuda.mem_get_info(0)[0]
    call()                                                         # warm-up: the engine's buffers are reserved here
    taken = free0 - torch.cuda.mem_get_info(0)[0]
    assert np.array_equal(blen, lens_h)
    at = np.concatenate([[0], np.cumsum(lens_h.astype(np.int64))[:-1]])
    first = np.concatenate([out[int(at[i]):int(at[i]) + int(lens_h[i])] for i in range(0, n, max(1, n // 64))])
    assert np.array_equal(first, want), "decoded bytes"
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    heng.close()
    return {"blocks": n, "max_block": hi, "fixed_uncomp": F, "framed_bytes": int(framed.size), "decoded_bytes": total,
            "wall_ms": ts, "wall_ms_median": sorted(ts)[1], "spread_ms": max(ts) - min(ts), "device_bytes_reserved": int(taken)}


def linked_case(kind, bl, n):
    """how many blocks of a linked stream the size pass leaves without a size (the rule's last clause: a match with extension
    bytes that ends in the last 64 bytes and reaches into the dictionary) -- one such block and the host call falls back"""
    src = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    eng.generate(kind, src, bl, n)
    eng.synchronize()
    raw = src.cpu().numpy().tobytes()
    eng.set_linked_compress(True)
    try:
        framed, _ = eng.compress_batch([raw[i * bl:(i + 1) * bl] for i in range(n)], header_kind=4)
    finally:
        eng.set_linked_compress(False)
    size = eng.decoded_sizes(framed, header_kind=4, max_uncomp=bl)
    assert all(int(v) in (bl, -0x7F000005) for v in size), "sizes"
    return {"kind": kind, "block": bl, "blocks": n, "unknown": int((size < 0).sum())}


parts = sys.argv[2:] or ["device", "host"]
records = {"size_pass": HAVE}
if "device" in parts and HAVE:
    records["device"] = [device_case(k, 65536, 65536) for k in ("lzsynth", "text", "random")] + [device_case("lzsynth", 65536, 160)]
    records["linked"] = [linked_case(k, 65536, 2048) for k in ("lzsynth", "text")]
if "host" in parts:
    records["host"] = [host_case(65536, 65536, 65536, 1), host_case(2048, 4096, 4 << 20, 2)]
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "size_pass_rate.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(records, f, indent=1)
print(json.dumps(records))
eng.close()
