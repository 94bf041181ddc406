"""The sessions on which the legacy face (include/lz4.h, csrc/legacy.cpp) is compared with the reference's own functions,
call by call.

A decode session is [(step name, block, capacity)] through ONE LZ4_streamDecode_t, every destination a buffer of its own (the
reference then takes its "switching to another buffer" branch from the second decoded block on, cbits/lz4.c:2347-2355: the
previous output is the external dictionary).  A compress session is [(step name, data, srcSize, dstCapacity, acceleration)]
through ONE LZ4_stream_t.  tests/golden/make_legacy_golden.py runs the reference on them and records return codes and digests in
tests/golden/legacy_sessions.json; tests/test_legacy_sessions_host.py holds the oracle's session model against that record,
tests/test_legacy_sessions_gpu.py the legacy face.  All three take the sessions from here: blocks are written by lz4_synth from
fixed seeds, data comes from the oracle's generators, nothing is stored.

Test infrastructure only (imported by tests, like reference_cases.py).
"""
import hashlib
import json
import os
import random

import lz4_synth as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "legacy_sessions.json")

SWING_SIZES = (100, 70000, 5, 300000, 65536, 1048576, 13, 65537, 200)     # D5: outputs through one context
SRC_SWING = (100, 300000, 5, 1048576, 64)                                # C4: sources through one context
C2_LENGTHS = (0, 1, 12, 13, 65535, 65536, 65537, 1048576)
C2_KINDS = ("text", "lzsynth", "random", "run")
C2_ACCELS = (-2 ** 31, -1, 0, 1, 9, 65537, 65538, 2 ** 31 - 1)
HUGE = 0x7E000001                                                       # LZ4_MAX_INPUT_SIZE + 1: only ever named


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def record(results):
    """what a session's [(code, bytes)] is recorded and compared by: the codes, and a digest per step that returned more than 0"""
    return {"codes": [int(c) for c, _ in results], "sha256": [sha(b) if c > 0 else None for c, b in results]}


# ---- decode sessions ----------------------------------------------------------------------------------------------------------

def _sized(b, size, last=12):
    """fills builder b up to a block of exactly `size` output bytes (the last `last` of them literals)"""
    target = size - last
    if target - 60 - b.op > 0:
        b.fill(out_bytes=target - 60 - b.op)
    b.pad_out(target)
    blk, n = b.block(last)
    assert n == size, (n, size)
    return blk


def plain_block(seed, size):
    """a self-contained block of exactly `size` output bytes"""
    return _sized(S.Builder(random.Random(seed)), size)


def dependent_block(seed, size, dict_len):
    """A block of exactly `size` bytes behind a predecessor of dict_len bytes: a match that starts at the first byte of the
    predecessor it can reach (its first byte, or offset 65535), a match that straddles the predecessor's end, and, where the
    predecessor is long enough, a match at offset 65535 further on.  A wrong dictionary -- another block's bytes, the wrong 64 KiB
    of the right one, one of another length -- changes the bytes or the code."""
    rng = random.Random(seed)
    b = S.Builder(rng, dict_len)
    if size < 13 or not dict_len:                     # too short for a match (MFLIMIT), or nothing in front
        if size < 13:
            return S.write_block([], b.lit(size))
        return _sized(b, size)
    if size == 13:                                    # room for one match: it straddles the predecessor's end
        s = min(dict_len, 4)
        b.add(1, 1 + s, 7)
        return b.block(5)[0]
    b.add(3, 3 + min(dict_len, 65535 - 3), 8)         # the first byte it can reach
    s = min(dict_len, 5)
    b.add(2, b.op + 2 + s, s + 6)                     # s bytes of the predecessor's end, then its own
    if dict_len + b.op + 2 >= 65535 and size > 200:
        b.add(2, 65535, 9)
    if size > 140000 and dict_len >= 65535:           # deep in the block: offset 65535 still reaches 16 bytes of the predecessor
        at = 65535 - 16
        b.fill(out_bytes=at - 60 - b.op, max_off=60000).pad_out(at - 2)
        b.add(2, 65535, 30)
    return _sized(b, size)


def d1_sessions():
    """every independent case in a fresh context: the first-call branch (:2327-2333)"""
    return [("D1 %s/%s" % (c.family, c.name), [(c.name, c.block, c.cap)]) for c in S.independent_cases()]


def d2_sessions():
    """the same blocks, in order, through one context behind a priming block: the ext-dict branch.  Blocks that reach in
    front of their own start may decode now; after every block that decodes, the dictionary is that block's output.  (The cases
    stand on their own, so one block that reaches the priming block -- its first byte, or the last 64 KiB of it at offset 65535 --
    goes in front of them.)"""
    out = []
    for prime in (70000, 100):
        steps = [("priming block of %d" % prime, plain_block(20 + prime, prime), prime),
                 ("reaches the priming block", dependent_block(30 + prime, 3000, prime), 3000)]
        steps += [("%s/%s" % (c.family, c.name), c.block, c.cap) for c in S.independent_cases()]
        out.append(("D2 behind %d bytes" % prime, steps))
    return out


def d3_sessions():
    return [("D3 stream %d" % k, [(name, blk, cap) for name, blk, cap, _ in st])
            for k, st in enumerate(S.dictionary_streams())]


def d4_session():
    """the context after a result <= 0: it is as it was (:2331, :2353)"""
    nA = 5000
    A = plain_block(41, nA)
    needs_a = dependent_block(42, 4000, nA)
    needs_b = dependent_block(43, 3000, 4000)
    cut = dependent_block(44, 6000, 3000)
    short = dependent_block(45, 2500, 3000)
    again = dependent_block(46, 3500, 3000)
    return ("D4 context after a failure", [
        ("block A", A, nA),
        ("malformed: literal length runs past the block", bytes([0xF0, 0xFF, 0xFF]), 1000),
        ("needs A", needs_a, 4000),
        ("decodes to 0 bytes", b"\x00", 100),
        ("needs the last output", needs_b, 3000),
        ("truncated", cut[:len(cut) // 2], 6000),
        ("capacity one too small", short, 2499),
        ("needs the last output again", again, 3500),
        # (regression cases go here, one line each)
    ])


def d5_session():
    """outputs that swing between 5 bytes and 1 MiB: the decoder's two device buffers and its staging regrow while the
    dictionary lives in the other buffer; dictionaries shorter than, equal to and longer than 64 KiB"""
    steps, prev = [], 0
    for k, size in enumerate(SWING_SIZES):
        steps.append(("%d bytes behind %d" % (size, prev), dependent_block(60 + k, size, prev), size))
        prev = size
    return ("D5 buffer swings", steps)


def d6_sessions():
    """capacities around what a block of 3000 bytes needs, 0 included, and srcSize 0 -- without a dictionary (a fresh context
    per capacity) and with one in force (one context: the block reaches its predecessor, which is 3000 bytes every time)"""
    n = 3000
    alone, dep = plain_block(71, n), dependent_block(72, n, n)
    caps = [("exact", n), ("+1", n + 1), ("+64", n + 64), ("-1", n - 1), ("12", 12), ("1", 1), ("0", 0)]
    edge = [("[0x00] capacity 0", b"\x00", 0), ("[0x00] capacity 1", b"\x00", 1), ("srcSize 0 capacity 100", b"", 100),
            ("srcSize 0 capacity 0", b"", 0)]
    out = [("D6 no dictionary, capacity %s" % name, [("capacity %s" % name, alone, cap)]) for name, cap in caps]
    out += [("D6 no dictionary, %s" % name, [(name, blk, cap)]) for name, blk, cap in edge]
    steps = [("priming block", plain_block(73, n), n)]
    steps += [("capacity %s" % name, dep, cap) for name, cap in caps] + edge
    steps.append(("exact again", dep, n))
    out.append(("D6 dictionary in force", steps))
    return out


def decode_sessions():
    """{"D1": [(session name, [(step name, block, cap)])], ...}"""
    return {"D1": d1_sessions(), "D2": d2_sessions(), "D3": d3_sessions(), "D4": [d4_session()], "D5": [d5_session()],
            "D6": d6_sessions()}


def model_session(oracle, steps):
    """lz4_synth.linked_expect's rule on a session's steps: [(code, bytes)]"""
    res = S.linked_expect(oracle, [(name, blk, cap, None) for name, blk, cap in steps])
    return [(code, dec if code > 0 else b"") for code, dec in res]


# ---- compress sessions --------------------------------------------------------------------------------------------------------

def gen_input(oracle, kind, n, seed=0):
    if kind == "run":
        return b"\x5a" * n
    return oracle.gen(kind, 1, max(n, 1), first_block=300 + seed)[:n].tobytes()


def bound(n):
    return n + n // 255 + 16


def c1_sessions(oracle):
    """Forced outcomes: [(session name, [(step name, data, srcSize, dstCapacity, accel)], forced)].  forced = the legacy face
    returns the reference's code (and, above 0, its bytes); otherwise both return more than 0 and the bytes are each codec's own.
    One context each: a refused size leaves the reference's context unusable."""
    rnd4k, rnd70k = gen_input(oracle, "random", 4096), gen_input(oracle, "random", 70000)
    out = [
        ("C1 srcSize 0, capacity 1", [("empty", b"", 0, 1, 1)], True),
        ("C1 srcSize 0, capacity 0", [("empty", b"", 0, 0, 1)], True),
        ("C1 4096 random bytes, capacity = srcSize", [("random", rnd4k, 4096, 4096, 1)], True),
        ("C1 70000 random bytes, capacity = srcSize", [("random", rnd70k, 70000, 70000, 1)], True),
        ("C1 srcSize -1", [("negative", b"x" * 64, -1, 64, 1)], True),
        ("C1 srcSize LZ4_MAX_INPUT_SIZE + 1", [("huge", b"x" * 64, HUGE, 64, 1)], True),
    ]
    steps = []
    for kind in C2_KINDS:
        for n in (0, 1, 13, 4096, 70000):
            steps.append(("%s %d at bound" % (kind, n), gen_input(oracle, kind, n), n, bound(n), 1))
    out.append(("C1 at LZ4_compressBound", steps, False))
    return out
