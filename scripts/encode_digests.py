"""Development aid: one sha256 per call over everything the six window and page calls write for tests/encode_cases.py -- the byte
identity list of a refactor of their kernels (docs/MEASUREMENT_LOG.md section 24; section 17 made such a list for the other encoders).
Run it on two builds of the library (MI355LZ4_LIB names the other one) and compare the lines:
    timeout -k 10 300 python3 scripts/encode_digests.py [OUT.txt]
The calls: mi355lz4_compress_fastdict_device, _fastdict_multi_device, _streams_fast_device (two calls, the second continuing the
slots the first left), _pages_device, _pages_fast_device, _pages_fastdict_device.  A digest covers the call's result arrays
(framedLen[]; nPages[], consumed[] and the page arrays' entries below nPages) and every written slot or page up to its length.  The
batch calls run twice: over the cases of up to 64 KiB (two windows per step) and over all of them (one).  The dictionary is the
first 192 bytes of every case, which the blocks do match into; the set's second member is its first 100 bytes, and the blocks name
-1, member 0 and member 1 in turn.  The pages are of 1, 12, 13, 64, 1000 and 4096 bytes in turn, eight to an input at the most."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import streamly_lz4_amd as S  # noqa: E402
import encode_cases as EC  # noqa: E402

dev = "cuda:0"
eng = S.Engine(0)
PAGE_SIZES, MAX_PAGES = (1, 12, 13, 64, 1000, 4096), 8
lines = []


def dtensor(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def say(name, count, what, h):
    lines.append("%-42s %s %4d  sha256 %s" % (name, what, count, h.hexdigest()))
    print(lines[-1], flush=True)


def batch(datas):
    """the blocks back to back on the device: (src, srcOff, srcLen, n, maxBlockLen)"""
    lens = np.array([len(d) for d in datas], dtype=np.int32)
    off = np.concatenate(([0], np.cumsum(lens[:-1], dtype=np.int64))).astype(np.int64)
    src = dtensor(np.frombuffer(b"".join(datas) + bytes(64), dtype=np.uint8).copy())
    return src, dtensor(off), dtensor(lens), len(datas), int(lens.max())


def slots_digest(name, n, stride, kind, call):
    slots = torch.full((n * stride,), 0xA5, dtype=torch.uint8, device=dev)
    flen = torch.full((n,), -77, dtype=torch.int32, device=dev)
    call(slots, flen, kind)
    eng.synchronize()
    f, s = flen.cpu().numpy(), slots.cpu().numpy()
    h = hashlib.sha256(f.tobytes())
    for i in range(n):
        h.update(s[i * stride: i * stride + max(int(f[i]), 0)].tobytes())
    say(name, n, "blocks", h)


def pages_digest(name, b, kind, call):
    src, off, ln, n, _ = b
    stride = kind + max(PAGE_SIZES)
    ps = dtensor(np.array([PAGE_SIZES[i % len(PAGE_SIZES)] for i in range(n)], dtype=np.int32))
    pages = torch.full((n * MAX_PAGES * stride,), 0xA5, dtype=torch.uint8, device=dev)
    sl, cl = (torch.full((n * MAX_PAGES,), -77, dtype=torch.int32, device=dev) for _ in range(2))
    cnt, cons = (torch.full((n,), -77, dtype=torch.int32, device=dev) for _ in range(2))
    call(src, off, ln, n, ps, MAX_PAGES, pages, stride, sl, cl, cnt, cons, kind)
    eng.synchronize()
    pg, sl, cl, cnt, cons = (t.cpu().numpy() for t in (pages, sl, cl, cnt, cons))
    h = hashlib.sha256(cnt.tobytes() + cons.tobytes())
    total = 0
    for i in range(n):
        for k in range(max(int(cnt[i]), 0)):
            at = i * MAX_PAGES + k
            h.update(sl[at: at + 1].tobytes() + cl[at: at + 1].tobytes())
            h.update(pg[at * stride: at * stride + kind + max(int(cl[at]), 0)].tobytes())
            total += 1
    say(name, total, "pages ", h)


cases = [c.data for c in EC.cases()]
small = [d for d in cases if len(d) <= 65536]
dict_bytes = b"".join(d[:192] for d in cases)
d0 = dtensor(np.frombuffer(dict_bytes, dtype=np.uint8).copy())
hd0, hd1 = S.HcDict(eng), S.HcDict(eng)
hd0.load(d0)
hd1.load(d0, 100)
dset = S.DictSet(eng, [hd0, hd1])

for tag, datas in (("64K", small), ("all", cases)):
    b = batch(datas)
    src, off, ln, n, mx = b
    idx = dtensor(np.array([i % 3 - 1 for i in range(n)], dtype=np.int32))
    for accel, kind in ((1, 8), (9, 4)):
        stride = S.slot_stride_ex(mx, kind, kind == 4)
        eng.set_block_checksum(kind == 4)                              # (the kind-4 rows carry trailers as well)
        slots_digest("fastdict %s accel %d kind %d" % (tag, accel, kind), n, stride, kind,
                     lambda s, f, k: eng.compress_fastdict_device(hd0, src, n, mx, s, stride, f, accel=accel, header_kind=k, src_off=off, src_len=ln))
        slots_digest("fastdict_multi %s accel %d kind %d" % (tag, accel, kind), n, stride, kind,
                     lambda s, f, k: eng.compress_fastdict_multi_device(dset, idx, src, n, mx, s, stride, f, accel=accel, header_kind=k,
                                                                        src_off=off, src_len=ln))
        # streams of seven blocks; the second call finds the tails the first one saved
        first = list(range(0, n, 7)) + [n]
        fs = S.FastCompressStreams(eng, len(first) - 1)
        for go in (1, 2):
            slots_digest("streams_fast %s accel %d kind %d call %d" % (tag, accel, kind, go), n, stride, kind,
                         lambda s, f, k: eng.compress_streams_fast_device(fs, src, n, mx, first, list(range(len(first) - 1)), s, stride, f,
                                                                          accel=accel, header_kind=k, src_off=off, src_len=ln))
        h = hashlib.sha256()
        for slot in range(len(first) - 1):
            count, held = fs.peek(slot)
            h.update(b"%d:" % count + held)
        say("streams_fast %s accel %d slots" % (tag, accel), len(first) - 1, "slots ", h)
        fs.close()
        eng.set_block_checksum(False)

b = batch(cases)
for kind in (8, 0):
    pages_digest("pages kind %d" % kind, b, kind, lambda *a: eng.compress_pages_device(*a[:-1], header_kind=a[-1]))
    for accel in (1, 9):
        pages_digest("pages_fast accel %d kind %d" % (accel, kind), b, kind,
                     lambda *a: eng.compress_pages_fast_device(*a[:-1], header_kind=a[-1], accel=accel))
        pages_digest("pages_fastdict accel %d kind %d" % (accel, kind), b, kind,
                     lambda *a: eng.compress_pages_fastdict_device(hd0, *a[:-1], header_kind=a[-1], accel=accel))

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
dset.close()
hd0.close()
hd1.close()
eng.close()
