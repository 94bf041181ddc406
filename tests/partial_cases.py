"""The partial-decode fixture (tests/golden/partial_vectors.json, written by tests/golden/make_partial_golden.py), expanded:
every case as (block, target, cap, result, prefix) -- the mutated compressed block, the arguments, and what the reference's
LZ4_decompress_safe_partial returned and wrote."""
import json
import os
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "partial_vectors.json")

PartialCase = namedtuple("PartialCase", "block target cap result prefix base mutations")


def load_raw():
    with open(PATH) as f:
        return json.load(f)


def expand(raw):
    bases = [(b["n"], bytes.fromhex(b["data"]), bytes.fromhex(b["block"])) for b in raw["bases"]]
    out = []
    for c in raw["cases"]:
        n, data, block = bases[c["base"]]
        blk = bytearray(block)
        for pos, val in c["mut"]:
            blk[pos] = val
        r = c["result"]
        # the prefix: the base's input where no run says otherwise (a run may reach past the input's end)
        pre = bytearray(max(r, 0))
        m = min(len(pre), len(data))
        pre[:m] = data[:m]
        for pos, hx in c["diff"]:
            run = bytes.fromhex(hx)
            pre[pos:pos + len(run)] = run
        assert len(pre) == max(r, 0)
        out.append(PartialCase(bytes(blk), c["target"], c["cap"], r, bytes(pre), c["base"], c["mut"]))
    return out


def load():
    return expand(load_raw())


# ---- well-formed blocks: the targets the GPU test asks for (tests/test_partial_decode_host.py holds the law they are checked
# against -- result = min(target, cap, n), bytes = the prefix -- to the reference for exactly these) ----------------------------

def targets_for(n, boundaries=(), rng=None, n_random=32, alone=()):
    """targets of a block of n decoded bytes: 0, 1, 2; every given sequence boundary and the bytes next to it (`alone`: without
    them); n - 40 .. n + 1 and n + 100; 16-byte flush boundaries and the 32 KiB segment seams with the bytes next to them; a few
    dozen random ones"""
    t = {0, 1, 2, n + 100}
    t.update(alone)
    for b in boundaries:
        t.update((b - 1, b, b + 1))
    t.update(range(n - 40, n + 2))
    for b in (16, 32, 48, 64, 128, 256, 1024, 4096, 6144, (n // 2) & ~15, n & ~15):
        t.update((b - 1, b, b + 1))
    for b in range(32768, n + 32768, 32768):
        t.update((b - 1, b, b + 1))
    if rng is not None:
        t.update(rng.randint(0, n + 40) for _ in range(n_random))
        for _ in range(6):                                   # flush boundaries in general: random multiples of 16
            b = 16 * rng.randint(0, n // 16)
            t.update((b - 1, b, b + 1))
    return sorted(x for x in t if 0 <= x <= n + 100)


# The decoders' own marks in output bytes (decode_par.hpp: PAR_WIN 1024, PAR_HIST 2000, PAR_BATCH_OUT 2560, PAR_RING 6144;
# decode_cu.hpp: CU_CBIG 16384, CU_CMAX 22528, CU_OUTMAX 32768 = the segment seam)
MARKS = (1024, 2000, 2560, 5120, 6144, 7680, 16384, 22528)


def sampled_boundaries(block, n, rng):
    """A bounded, deterministic sample of a big block's sequence boundaries (a hand-built block of 64 KiB has thousands; every
    one of them with its neighbours would be a million entries over all blocks).  Returns (with_neighbours, alone):
      with_neighbours  the first 8 and the last 8 boundaries, and the boundary next below and next above every mark: the
                       decoders' window, history, batch and ring sizes (MARKS), every multiple of 32 KiB (the workgroup form's
                       segment seam) and n / 2 -- the block's named edge lies at one of these or at its end;
      alone            24 boundaries drawn at random."""
    import bisect
    bs = boundaries_of(block)
    near = set(bs[:8] + bs[-8:])
    for m in list(MARKS) + list(range(32768, n + 1, 32768)) + [n // 2]:
        i = bisect.bisect_left(bs, m)
        near.update(bs[max(i - 1, 0):i + 1])
    alone = set(rng.sample(bs, min(24, len(bs)))) - near
    return sorted(near), sorted(alone)


def caps_for(t, n, k):
    """the capacity that goes with the k-th target: below, at and above the target in turn"""
    return (max(t - 3, 0), t, n, n + 64, max(t // 2, 0), t + 1)[k % 6]


def hand_built_blocks():
    """[(name, block, data)]: lz4_synth's valid blocks without a dictionary and without an offset of 0, with what they decode to"""
    import lz4_synth as Z
    out = []
    for c in Z.independent_cases() + Z.end_family() + Z.length_family():
        if not c.valid:
            continue
        try:
            seqs = Z.parse(c.block)
        except ValueError:
            continue
        if any(s[3] == 0 for s in seqs):
            continue
        r, data = Z.plain_decode(c.block, c.cap)
        if r < 0:
            continue
        out.append(("%s/%s" % (c.family, c.name), c.block, data))
    return out


def boundaries_of(block):
    import lz4_synth as Z
    b = set()
    for tp, ls, lit, off, ml, op in Z.parse(block):
        b.add(op)
        b.add(op + lit)
        if ml is not None:
            b.add(op + lit + ml)
    return sorted(b)
