"""Development aid: what block checksums (mi355lz4_set_block_checksum) cost on the device.  One JSON record, printed and
written to profiles/block_checksum_rate.json (or the path given as the first argument):
  xxh32_device over the compressed blocks of the bench's decompress config (65 536 x 64 KiB lzsynth(16, 2048));
  decompress and compress of that config, switch on vs off;
  160 x 64 KiB decompress (the small-call shape) and 3 x 4 MiB decompress, on vs off, and the chain cost per 16 bytes
  that the 3 x 4 MiB call implies (the added time / the compressed bytes of ONE block / 16: the blocks hash side by side).
Times are the median of `reps` event-timed calls on the engine's stream after a warm-up.
    python3 scripts/block_checksum_rate.py [OUT.json] [CASE ...]"""
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
reps = 15


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


def setup(kind, bl, n):
    src = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    eng.generate(kind, src, bl, n)
    out = {}
    for ck in (False, True):
        eng.set_block_checksum(ck)
        stride = S.slot_stride_ex(bl, 8, ck)
        slots = torch.empty(n * stride, dtype=torch.uint8, device=dev)
        flen = torch.zeros(n, dtype=torch.int32, device=dev)
        eng.compress_batch_device(src, n, bl, slots, stride, flen)
        boff = torch.arange(n, dtype=torch.int64, device=dev) * stride
        out[ck] = (slots, stride, flen, boff)
    eng.synchronize()
    return src, out


def rates(kind, bl, n, with_compress):
    src, st = setup(kind, bl, n)
    dst = torch.empty(n * bl, dtype=torch.uint8, device=dev)
    ooff = torch.arange(n + 1, dtype=torch.int64, device=dev) * bl
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    rec = {"kind": kind, "block": bl, "blocks": n}
    for ck in (False, True):
        slots, stride, flen, boff = st[ck]
        eng.set_block_checksum(ck)
        tag = "on" if ck else "off"
        rec["decompress_ms_" + tag] = timed(lambda: eng.decompress_batch_device(slots, n * stride, boff, n, dst, ooff, res))
        assert res.cpu().tolist() == [bl] * n and torch.equal(dst, src), "round trip (%s)" % tag
        if with_compress:
            rec["compress_ms_" + tag] = timed(lambda: eng.compress_batch_device(src, n, bl, slots, stride, flen))
    flen_off = st[False][2]
    comp = int(flen_off.sum().item()) - 8 * n
    rec["compressed_bytes"] = comp
    rec["decompress_added_ms"] = rec["decompress_ms_on"] - rec["decompress_ms_off"]
    rec["decompress_slowdown_pct"] = 100.0 * rec["decompress_added_ms"] / rec["decompress_ms_off"]
    if with_compress:
        rec["compress_slowdown_pct"] = 100.0 * (rec["compress_ms_on"] - rec["compress_ms_off"]) / rec["compress_ms_off"]
    # the kernel alone over the compressed blocks
    slots, stride, flen, boff = st[True]
    off = boff + 8
    ln = (flen - 12).to(torch.int32)
    h = torch.zeros(n, dtype=torch.int32, device=dev)
    rec["xxh32_device_ms"] = timed(lambda: eng.xxh32_device(slots, off, ln, n, 0, h))
    rec["xxh32_device_GBps"] = comp / rec["xxh32_device_ms"] / 1e6
    rec["largest_block_compressed"] = int(ln.max().item())
    return rec


CASES = {
    "config2": ("lzsynth", 65536, 65536, True),
    "small_160x64k": ("lzsynth", 65536, 160, False),
    "three_4MiB": ("text", 4 << 20, 3, False),
}
only = sys.argv[2:] or list(CASES)           # e.g. one case under rocprofv3 --kernel-trace, to see the call's kernels
records = {name: rates(*CASES[name]) for name in only}
if "three_4MiB" in records:
    t = records["three_4MiB"]
    # two numbers: what the switch adds to the decode call, and what the xxh32 kernel alone takes, per 16 bytes of the
    # longest block (the blocks hash side by side)
    t["call_added_ns_per_16B"] = t["decompress_added_ms"] * 1e6 / (t["largest_block_compressed"] / 16.0)
    t["kernel_ns_per_16B"] = t["xxh32_device_ms"] * 1e6 / (t["largest_block_compressed"] / 16.0)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "block_checksum_rate.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(records, f, indent=1)
print(json.dumps(records))
eng.close()
