"""The decoded-size pass's acceptance rule in plain Python, and the blocks both of its test files run it over.

model_size(block, max_uncomp) is what mi355lz4_decoded_size_device must answer for a block whose header is fine: lz4_synth.parse
(the chain is well formed) plus the end-of-block rules, the bound, and the clauses that make "decode into exactly s bytes" the
same as "decode into any larger capacity" (csrc/size_walk.hpp states them; tests/test_decoded_size_host.py holds the oracle to
that equivalence for every block the model accepts).

Test infrastructure only (imported by tests, like lz4_synth.py).
"""
import random

import lz4_synth as Z

UNKNOWN = -0x7F000005          # MI355LZ4_BLK_E_SIZE_UNKNOWN
E_COMPLEN = -0x7F000001
E_TRUNCATED = -0x7F000002
TAIL = 64                      # the reference's FASTLOOP_SAFE_DISTANCE


def model_size(block, max_uncomp):
    block = bytes(block)
    try:
        seqs = Z.parse(block)
    except ValueError:
        return UNKNOWN
    if not seqs or seqs[-1][3] is not None:            # empty, or it ends with a match
        return UNKNOWN
    last = seqs[-1]
    s = last[5] + last[2]
    if s > max_uncomp:
        return UNKNOWN
    for tp, _, lit, off, ml, op in seqs[:-1]:
        pos = op + lit
        # cbits/lz4.c:214-221: the last match starts 12 bytes before the end or earlier (pos <= s - 12 is what the decoder asks,
        # :1991, and what the compressor's mflimitPlusOne allows: it does write such blocks), the last 5 bytes are literals,
        # and a block of under 13 bytes has no match
        if s < Z.MFLIMIT + 1 or pos > s - Z.MFLIMIT or pos + ml > s - Z.LASTLITERALS:
            return UNKNOWN
        if off == 0:
            return UNKNOWN
        # a match with extension bytes that ends within the last 64 bytes and reaches in front of the block: the code of
        # a bad offset there depends on the capacity (cbits/lz4.c:1853 against :2073)
        if (block[tp] & 15) == 15 and off > pos and pos + ml >= s - TAIL:
            return UNKNOWN
    if s == 0 and block != b"\x00":                    # cbits/lz4.c:1781-1785
        return UNKNOWN
    return s


FUZZ_LENGTHS = (13, 14, 20, 64, 65, 100, 300, 2000, 9000, 40000, 65535, 65536)
FUZZ_KINDS = ("text", "lzsynth", "random", "zero")


def gen(oracle, kind, n, seed=0):
    return bytes(n) if kind == "zero" else oracle.gen(kind, 1, n, first_block=seed).tobytes()


def fuzz_blocks(oracle, count=600, seed=2718):
    """[(original length, unmutated block, mutated block)]: oracle-compressed blocks of 13..65536 bytes of text / lzsynth /
    random / zeros with a single byte changed, a short span overwritten, a few bytes changed, the tail cut or bytes appended."""
    rng = random.Random(seed)
    out = []
    for it in range(count):
        kind = rng.choice(FUZZ_KINDS)
        n = rng.choice(FUZZ_LENGTHS)
        comp = oracle.compress_block(gen(oracle, kind, n, it), rng.choice((1, 1, 9)))
        m = bytearray(comp)
        mode = rng.randrange(6)
        if mode in (0, 1):
            m[rng.randrange(len(m))] = rng.randrange(256)
        elif mode == 2:
            at = rng.randrange(len(m))
            for k in range(at, min(len(m), at + rng.randrange(2, 9))):
                m[k] = rng.randrange(256)
        elif mode == 3:
            for _ in range(rng.randrange(2, 4)):
                m[rng.randrange(len(m))] = rng.randrange(256)
        elif mode == 4:
            m = m[: rng.randrange(1, len(m) + 1)]
        else:
            m += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 6)))
        out.append((n, comp, bytes(m)))
    return out


def frame4(blocks, trailer=None, gap=0, seed=5):
    """headerKind 4 framing: ([compLen][block]([trailer(block) as 4 bytes]))*, with up to `gap` foreign bytes in front of every
    block when asked; returns (bytes, block offsets)"""
    rng = random.Random(seed)
    buf, offs = bytearray(), []
    for b in blocks:
        if gap:
            buf += bytes(rng.randrange(256) for _ in range(rng.randrange(1, gap + 1)))
        offs.append(len(buf))
        buf += len(b).to_bytes(4, "little") + bytes(b)
        if trailer:
            buf += int(trailer(bytes(b))).to_bytes(4, "little")
    if gap:
        buf += bytes(rng.randrange(256) for _ in range(gap))
    return bytes(buf), offs
