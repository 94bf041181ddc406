"""Writes tests/golden/partial_vectors.json: what the reference's LZ4_decompress_safe_partial (cbits/lz4.c:2179-2185) returns and
writes for mutated blocks.  Needs oracle/_ref/liblz4ref.so (make oracle, where the reference sources are present); the file it
writes holds data only and is what the tests read.

    python tests/golden/make_partial_golden.py

The blocks: text-like inputs of 64, 300, 1500 and 4096 bytes, compressed by the reference (LZ4_compress_default), with 1-3 bytes
of the compressed block replaced.  Targets are random in 0 .. n + 40, the capacity is one of {target, n, n + 64}.  Every case is
run twice, over an output buffer of 0x00 and one of 0xEE: a case whose result or prefix differs between the two depends on what
lay in the buffer before (an offset of 0 copies bytes onto themselves, :2112-2113) and is dropped; more than 1 % of drops fail
the script.  About 600 cases are kept, at least 100 with a negative result and at least 300 with a non-negative one.

Layout of the file (to keep it small, a case names its base block and its mutations, and its prefix is stored as the runs in
which it differs from the base's input; tests/partial_cases.py expands both):
    bases: [{n, data (hex), block (hex)}]
    cases: [{base, mut: [[pos, byte], ...], target, cap, result, diff: [[pos, hex], ...]}]"""
import ctypes as C
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SIZES = (64, 300, 1500, 4096)
CANDIDATES = 6000
KEEP = 600
WORDS = ("the of and to in is that it was for on are as with his they at be this from have or by one had not but what all "
         "were when we there can an your which their said if do will each about how up out them then she many some so these "
         "would other into has more her two like him see time could no make than first been its who now people my made over "
         "did down only way find use may water long little very after words called just where most know").split()


def text_like(n, seed):
    rnd = random.Random(seed)
    out = []
    size = 0
    while size < n:
        w = rnd.choice(WORDS) + rnd.choice((" ", " ", " ", ", ", ".\n"))
        out.append(w)
        size += len(w)
    return "".join(out).encode()[:n]


def load_reference():
    L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "liblz4ref.so"))
    L.LZ4_compressBound.restype = C.c_int
    L.LZ4_compressBound.argtypes = [C.c_int]
    L.LZ4_compress_default.restype = C.c_int
    L.LZ4_compress_default.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    L.LZ4_decompress_safe_partial.restype = C.c_int
    L.LZ4_decompress_safe_partial.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    return L


def ref_compress(L, data):
    cap = L.LZ4_compressBound(len(data))
    dst = C.create_string_buffer(cap)
    r = L.LZ4_compress_default(data, dst, len(data), cap)
    assert r > 0
    return dst.raw[:r]


def ref_partial(L, block, target, cap, fill=0):
    """(result, the first max(result, 0) bytes) of LZ4_decompress_safe_partial over a buffer pre-filled with `fill`."""
    room = max(min(target, cap), 0) + 64
    dst = C.create_string_buffer(bytes([fill]) * room, room)
    src = C.create_string_buffer(block + bytes(64), len(block) + 64)      # (what lies behind the block is defined)
    r = L.LZ4_decompress_safe_partial(src, dst, len(block), target, cap)
    return r, dst.raw[:max(r, 0)]


def diff_runs(prefix, data):
    """the runs in which prefix differs from data (bytes behind data's end differ from nothing: they are runs too)"""
    runs = []
    i = 0
    while i < len(prefix):
        if i < len(data) and prefix[i] == data[i]:
            i += 1
            continue
        j = i
        while j < len(prefix) and not (j < len(data) and prefix[j] == data[j]):
            j += 1
        runs.append([i, prefix[i:j].hex()])
        i = j
    return runs


def candidates(L, bases, rnd):
    dropped = 0
    out = []
    for k in range(CANDIDATES):
        b = k % len(bases)
        n, block = bases[b]["n"], bytearray(bytes.fromhex(bases[b]["block"]))
        mut = []
        for _ in range(rnd.randint(1, 3)):
            pos = rnd.randrange(len(block))
            val = (block[pos] + rnd.randint(1, 255)) & 255
            block[pos] = val
            mut.append([pos, val])
        target = rnd.randint(0, n + 40)
        cap = rnd.choice((target, n, n + 64))
        r0, p0 = ref_partial(L, bytes(block), target, cap, 0x00)
        r1, p1 = ref_partial(L, bytes(block), target, cap, 0xEE)
        if r0 != r1 or p0 != p1:
            dropped += 1
            continue
        out.append({"base": b, "mut": mut, "target": target, "cap": cap, "result": r0,
                    "diff": diff_runs(p0, bytes.fromhex(bases[b]["data"]))})
    return out, dropped


def main():
    L = load_reference()
    rnd = random.Random(20260117)
    bases = []
    for i, n in enumerate(SIZES):
        data = text_like(n, 1000 + i)
        bases.append({"n": n, "data": data.hex(), "block": ref_compress(L, data).hex()})
    cands, dropped = candidates(L, bases, rnd)
    print("candidates %d, dropped (depend on the buffer's contents) %d" % (CANDIDATES, dropped))
    assert dropped * 100 <= CANDIDATES, "more than 1 %% of the cases depend on what lay in the output buffer: %d" % dropped
    neg = [c for c in cands if c["result"] < 0]
    pos = [c for c in cands if c["result"] >= 0]
    rnd.shuffle(neg)
    rnd.shuffle(pos)
    n_neg = min(len(neg), KEEP // 4)
    cases = neg[:n_neg] + pos[:KEEP - n_neg]
    rnd.shuffle(cases)
    assert sum(c["result"] < 0 for c in cases) >= 100, "fewer than 100 cases with a negative result"
    assert sum(c["result"] >= 0 for c in cases) >= 300, "fewer than 300 mutated cases with a non-negative result"
    path = os.path.join(HERE, "partial_vectors.json")
    with open(path, "w") as f:
        json.dump({"note": "LZ4_decompress_safe_partial of the reference on mutated blocks (make_partial_golden.py)",
                   "bases": bases, "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d cases (%d negative), %d bytes" % (path, len(cases), sum(c["result"] < 0 for c in cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
