"""Development aid: does a call of the wavefront-per-block decoder (decoder 2) run in ROUNDS of as many blocks as the GPU has wave slots?
Times one launch, HIP events, best of 8, for block counts around the multiples of 7168 (28 waves x 256 CUs) and of 8192 (32 waves),
on the bench's lzsynth stream and on text; each library runs in a process of its own (MI355LZ4_LIB).
    python scripts/par_call_staircase.py [name=lib.so ...]      (no argument: the built library)
One line per library, kind and block count: ms per call, GB/s, and ms per 1024 blocks since the count before."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = 7168
COUNTS = sorted(set([k * SLOTS for k in range(1, 10)] + [k * SLOTS + 1024 for k in range(1, 10)] + [8192, 16384, 61440, 65536, 66560]))
BL = 65536
REPS = 8


def child():
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "streamly-lz4_amd"))
    import torch, streamly_lz4_amd as S
    name = sys.argv[2]
    dev = torch.device("cuda:0"); eng = S.Engine(0); eng.set_decoder(2)
    NB = max(COUNTS)
    for kind in ("lzsynth", "text"):
        src = torch.empty(NB * BL, dtype=torch.uint8, device=dev); eng.generate(kind, src, BL, NB)
        stride = S.slot_stride(BL, 8)
        slots = torch.empty(NB * stride, dtype=torch.uint8, device=dev); flen = torch.empty(NB, dtype=torch.int32, device=dev)
        dense = torch.empty(NB * stride, dtype=torch.uint8, device=dev); doff = torch.empty(NB + 1, dtype=torch.int64, device=dev)
        ooff = torch.arange(NB + 1, dtype=torch.int64, device=dev) * BL
        out = torch.empty(NB * BL, dtype=torch.uint8, device=dev); res = torch.empty(NB, dtype=torch.int32, device=dev)
        eng.compress_batch_device(src, NB, BL, slots, stride, flen)
        eng.compact_device(slots, stride, flen, NB, dense, NB * stride, doff); eng.synchronize()
        ends = doff.cpu().tolist()
        e = [S.Event() for _ in range(2)]
        prev_n, prev_t = 0, 0.0
        for nb in COUNTS:
            out.zero_(); res.zero_(); td = 1e9
            for it in range(REPS):
                eng.record(e[0]); eng.decompress_batch_device(dense, ends[nb], doff, nb, out, ooff, res); eng.record(e[1]); eng.synchronize()
                td = min(td, eng.elapsed_ms(e[0], e[1]))
            ok = bool((res[:nb] == BL).all().item()) and torch.equal(out[:nb * BL], src[:nb * BL])
            print("%s %s blocks %6d = %.3f x 7168 = %.3f x 8192: %.4f ms %7.1f GB/s, %+.4f ms per 1024 blocks since %d, ok=%s"
                  % (name, kind, nb, nb / 7168.0, nb / 8192.0, td, nb * BL / td / 1e6, (td - prev_t) * 1024.0 / (nb - prev_n), prev_n, ok), flush=True)
            prev_n, prev_t = nb, td
        del src, slots, dense, out
    eng.close()


def main():
    libs = sys.argv[1:] or ["built=" + os.path.join(ROOT, "streamly-lz4_amd", "lib", "libmi355lz4.so")]
    for spec in libs:
        name, _, lib = spec.partition("=")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=dict(os.environ, MI355LZ4_LIB=os.path.abspath(lib)), timeout=300)
        if r.returncode != 0:
            sys.exit("par_call_staircase: %s ended with %d; nothing further is started" % (name, r.returncode))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child()
    else:
        main()
