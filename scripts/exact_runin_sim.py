"""Host-only: how often a run-in of R blocks from a zeroed hash table reaches the true table of a linked stream --
the evidence behind the reference-exact compress mode's speculation.

The true stream is the oracle's: orc_cstream_init once, orc_compress_fast_continue per block, each block its own
allocation.  For a block j, a second stream is started at block j-R with a zeroed table but the true currentOffset,
dictSize and dictionary, compresses R blocks, and its table is compared with the true one at block j after both are
canonicalised (entries below currentOffset - 65536, which no position of block j can use, read 0).  Where they agree
the script also checks that block j's compressed bytes agree.  Prints one JSON line:
    python3 scripts/exact_runin_sim.py [--blocks N] [--pieces K] [--runins 1,2,3,4,6,8,12] [--kinds text,pysrc,lzsynth]"""
import argparse
import ctypes as C
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle import Oracle, build  # noqa: E402

_u8p = C.POINTER(C.c_uint8)


class CStream(C.Structure):           # oracle/lz4_oracle.h, orc_cstream
    _fields_ = [("table", C.c_uint32 * 4096), ("currentOffset", C.c_uint32), ("dict", C.c_void_p), ("dictSize", C.c_uint32)]


lib = C.CDLL(build(), mode=os.RTLD_LOCAL)
lib.orc_compress_fast_continue.restype = C.c_int
lib.orc_compress_fast_continue.argtypes = [C.POINTER(CStream), _u8p, _u8p, C.c_int, C.c_int, C.c_int]
lib.orc_compress_bound.restype = C.c_int


def blocks_of(kind, n, bl):
    if kind == "pysrc":
        buf = bytearray()
        for f in sorted(glob.glob(os.path.join(os.path.dirname(os.__file__), "**", "*.py"), recursive=True)):
            buf += open(f, "rb").read()
            if len(buf) >= n * bl:
                break
        raw = (bytes(buf) * (1 + n * bl // max(len(buf), 1)))[: n * bl]
    else:
        raw = Oracle().gen(kind, n, bl).tobytes()
    out = []
    for i in range(n):                # separate allocations, readable slack behind each
        a = np.zeros(bl + 64, dtype=np.uint8)
        a[:bl] = np.frombuffer(raw[i * bl:(i + 1) * bl], dtype=np.uint8)
        out.append(a)
    return out


def step(s, a, bl, dst):
    return lib.orc_compress_fast_continue(C.byref(s), a.ctypes.data_as(_u8p), dst.ctypes.data_as(_u8p), bl,
                                          lib.orc_compress_bound(bl), 1)


def canon(s):
    t = np.ctypeslib.as_array(s.table).copy()
    if s.currentOffset > 65536:
        t[t < s.currentOffset - 65536] = 0
    return t


def run(kind, n, bl, runins, pieces):
    arr = blocks_of(kind, n, bl)
    dst = np.zeros(lib.orc_compress_bound(bl) + 64, dtype=np.uint8)
    true_s = CStream()
    lib.orc_cstream_init(C.byref(true_s))
    states, outs = [], []              # the true stream before every block
    for a in arr:
        snap = CStream()
        C.pointer(snap)[0] = true_s
        states.append(snap)
        r = step(true_s, a, bl, dst)
        outs.append(dst[:r].tobytes())
    rmax = max(runins)
    targets = np.linspace(rmax, n - 1, num=min(pieces, n - rmax)).astype(int)
    res = {}
    for R in runins:
        equal = bytes_ok = 0
        for j in targets:
            s = CStream()
            C.pointer(s)[0] = states[j - R]
            C.memset(s.table, 0, 4 * 4096)                       # zeroed table, true offsets and dictionary
            for k in range(j - R, j):
                step(s, arr[k], bl, dst)
            if np.array_equal(canon(s), canon(states[j])):
                equal += 1
                r = step(s, arr[j], bl, dst)
                bytes_ok += dst[:r].tobytes() == outs[j]
        res[str(R)] = {"tables_equal": equal / len(targets),
                       "bytes_equal_where_tables_equal": bytes_ok / equal if equal else None}
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=300)
    ap.add_argument("--block", type=int, default=65536)
    ap.add_argument("--pieces", type=int, default=250)
    ap.add_argument("--runins", default="1,2,3,4,6,8,12")
    ap.add_argument("--kinds", default="text,pysrc,lzsynth")
    a = ap.parse_args()
    runins = [int(x) for x in a.runins.split(",")]
    out = {k: run(k, a.blocks, a.block, runins, a.pieces) for k in a.kinds.split(",")}
    print(json.dumps({"block": a.block, "blocks": a.blocks, "pieces": a.pieces, "accel": 1, "results": out}))
