"""The inputs of tests/test_write_confinement_gpu.py, built without a GPU so that tests/test_guarded.py can pin what they
contain: which families are present, how many of the corrupted blocks really fail, which capacities occur.  Expected results
always come from the oracle.

Test infrastructure only (imported by tests, like lz4_synth.py)."""
import random

import lz4_synth as S
from reference_cases import huge_length_blocks

# the length list of test_parity_gpu.test_decode_matches_oracle
ORACLE_LENGTHS = (1, 5, 12, 13, 63, 64, 65, 300, 4096, 65536, 100001, 262144)
BIG_LENGTHS = (1 << 20, 4 << 20)
SMALL_CLASS = 70000                 # blocks are batched by capacity class: a headerKind-4 call has one fixedUncomp


class DCase:
    """One framed block of a decode call: the payload, the capacity its header states (headerKind 8) and, where it is known,
    the size of the data it was compressed from."""
    __slots__ = ("family", "name", "payload", "cap", "raw_len", "corrupted")

    def __init__(self, family, name, payload, cap, raw_len=None, corrupted=False):
        self.family, self.name, self.payload, self.cap, self.raw_len, self.corrupted = family, name, payload, cap, raw_len, corrupted

    def __repr__(self):
        return "DCase(%s/%s, %d -> %d)" % (self.family, self.name, len(self.payload), self.cap)


def oracle_written(oracle):
    out = []
    for kind in ("lzsynth", "text", "random"):
        for bl in ORACLE_LENGTHS:
            for accel in (1, 400):
                data = oracle.gen(kind, 1, bl, first_block=bl + accel).tobytes()
                out.append(DCase("oracle", "%s %d accel %d" % (kind, bl, accel), oracle.compress_block(data, accel), bl, bl))
    return out


def synth():
    return [DCase("synth:" + c.family, c.name, c.block, c.cap, None, not c.valid) for c in S.independent_cases()]


def fuzz_small(oracle, n_cases=240, seed=2024):
    """the corruption modes of test_parity_gpu.test_decode_fuzz_vs_oracle: 0 untouched, 1 truncated, 2 bytes overwritten,
    3 bytes appended, 4 capacity off by up to 20"""
    rng = random.Random(seed)
    out = []
    for it in range(n_cases):
        kind = rng.choice(["lzsynth", "text", "random"])
        n = rng.choice([1, 12, 13, 20, 64, 65, 100, 300, 2000, 9000])
        data = oracle.gen(kind, 1, n, first_block=it).tobytes()
        comp = bytearray(oracle.compress_block(data, rng.choice([1, 1, 9])))
        mode = it % 5
        if mode == 1:
            comp = comp[: rng.randrange(1, len(comp) + 1)]
        elif mode == 2:
            for _ in range(rng.randrange(1, 4)):
                comp[rng.randrange(len(comp))] = rng.randrange(256)
        elif mode == 3:
            comp += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 6)))
        cap = n if mode != 4 else max(0, n + rng.randrange(-20, 20))
        out.append(DCase("fuzz_small:%d" % mode, "%s %d" % (kind, n), bytes(comp), cap, n, mode != 0))
    return out


def _corrupt_large(rng, comp, cap, mode):
    """the corruption modes of test_fuzz_large_gpu.py"""
    comp = bytearray(comp)
    if mode == 0:                                   # single bit
        comp[rng.randrange(len(comp))] ^= 1 << rng.randrange(8)
    elif mode == 1:                                 # a few random bytes
        for _ in range(rng.randrange(1, 5)):
            comp[rng.randrange(len(comp))] = rng.randrange(256)
    elif mode == 2:                                 # truncation
        comp = comp[: rng.randrange(1, len(comp))]
    elif mode == 3:                                 # a run of 0xFF (length-extension storms) or zeros (offset 0)
        p = rng.randrange(len(comp))
        comp[p:p + rng.randrange(1, 40)] = bytes([rng.choice([0xFF, 0x00])]) * min(40, len(comp) - p)
    elif mode == 4:                                 # capacity too small / too large
        cap = max(0, cap + rng.choice([-1, -7, -64, -1000, 5, 300]))
    return bytes(comp), cap                         # mode 5: untouched


def fuzz_large(oracle, n_cases=240, seed=99):
    rng = random.Random(seed)
    base = []
    for kind in ("lzsynth", "text"):
        for bl in (4096, 20000, 65536):
            d = oracle.gen(kind, 1, bl, first_block=7).tobytes()
            base.append((kind, d, oracle.compress_block(d, 1)))
    out = []
    for t in range(n_cases):
        kind, d, comp = base[t % len(base)]
        mode = (t // len(base)) % 6
        p, cap = _corrupt_large(rng, comp, len(d), mode)
        out.append(DCase("fuzz_large:%d" % mode, "%s %d" % (kind, len(d)), p, cap, len(d), mode != 5))
    return out


def big(oracle, seed=5):
    """1 MiB and 4 MiB blocks, clean and under every corruption mode of fuzz_large"""
    rng = random.Random(seed)
    out = []
    for bl in BIG_LENGTHS:
        d = oracle.gen("text", bl // 65536, 65536, first_block=11).tobytes()
        comp = oracle.compress_block(d, 1)
        for mode in (5, 0, 2, 3, 4):
            p, cap = _corrupt_large(rng, comp, bl, mode)
            out.append(DCase("big:%d" % mode, "text %d" % bl, p, cap, bl, mode != 5))
    return out


def huge():
    return [DCase("huge", name, payload, cap, None, True) for name, payload, cap in huge_length_blocks()]


def malformed(golden):
    """golden.json's malformed blocks, each with the capacity recorded there (an empty payload cannot be framed: compLen 0 is a
    header rejection)"""
    return [DCase("malformed", m["name"], bytes.fromhex(m["payload_hex"]), m["cap"], None, True)
            for m in golden["malformed"] if m["payload_hex"]]


def decode_cases(oracle, golden):
    return oracle_written(oracle) + synth() + fuzz_small(oracle) + fuzz_large(oracle) + big(oracle) + huge() + malformed(golden)


def capacity_classes(cases):
    """{"small": [...], "large": [...]}: a call's blocks share a capacity class (and, with headerKind 4, one fixedUncomp)"""
    return {"small": [c for c in cases if c.cap <= SMALL_CLASS], "large": [c for c in cases if c.cap > SMALL_CLASS]}


CAPMODES = ("absent", "larger", "smaller")


def region_sizes(cases, kind, capmode):
    """(the call's fixedUncomp, [(outCap[i] or None, cap_i)]) of one decode call over `cases`: cap_i, the bytes block i may write,
    is outCap[i], else the header's uncompLen (headerKind 8) or fixedUncomp (4), and 0 where the header's uncompLen exceeds
    outCap[i].  The GPU test builds its guarded output layout from these sizes, tests/test_guarded.py pins their alignments."""
    fixed = max(c.cap for c in cases) if kind == 4 else 0
    out = []
    for i, c in enumerate(cases):
        if capmode == "absent":
            ocap = None
        elif capmode == "larger":
            ocap = c.cap + (1, 7, 64, 300)[i % 4]
        else:
            ocap = max(0, c.cap - (1, 7, 64)[i % 3])
        if kind == 8 and ocap is not None and c.cap > ocap:
            out.append((ocap, 0))                                   # rejected for its uncompLen: the block may write nothing
        else:
            out.append((ocap, ocap if ocap is not None else (c.cap if kind == 8 else fixed)))
    return fixed, out


def code_class(code, comp_len):
    """where in the block the reference gave up (its code is -(ip - src) - 1, cbits/lz4.c:2163): at the first token, inside the
    block, in its last 16 bytes or at its very end"""
    if code >= 0:
        return "ok"
    ip = -code - 1
    if ip == 0:
        return "first token"
    if ip >= comp_len:
        return "end"
    return "tail" if ip >= comp_len - 16 else "inside"


# ---- encoder inputs ----------------------------------------------------------------------------------------------------------------

ENC_LENGTHS = (0, 1, 12, 13, 65535, 65536, 65537)


def encode_blocks(oracle, n_fuzz=40, seed=11):
    """ragged blocks of one compress call: the edge lengths compressible and incompressible (an incompressible block fills its
    slot to the worst case), then test_fuzz_encode_gpu._make's structured inputs"""
    from test_fuzz_encode_gpu import _make
    rng = random.Random(seed)
    blocks = []
    for n in ENC_LENGTHS:
        for kind in ("random", "text"):
            blocks.append(oracle.gen(kind, 1, max(n, 1), first_block=100 + n)[:n].tobytes())
    blocks += [_make(rng, oracle, t) for t in range(n_fuzz)]
    # the slots are sized for the call's longest block: only an incompressible block of THAT length fills a slot to the worst case
    blocks.append(oracle.gen("random", 1, max(len(b) for b in blocks), first_block=seed).tobytes())
    return blocks
