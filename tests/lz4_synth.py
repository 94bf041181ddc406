"""Hand-built LZ4 blocks: written sequence by sequence, not by a compressor.

A greedy hash compressor writes a narrow part of the valid-block space; where its sequences fall relative to the decoders'
internal limits depends on the data.  The families below place lengths, offsets, tokens, match ends and literal ends on those
limits on purpose -- decode_par.hpp: PAR_WIN, PAR_HIST, PAR_BATCH_OUT, PAR_RING, one extension byte; decode_cu.hpp: 16-byte
chunks, 256-byte super-chunks, CU_CAND, CU_SLOTS, CU_NMAX, CU_OUTMAX, CU_CMAX / CU_CBIG, the 512-byte sequential tail, two
extension bytes -- and each case says which edge it aims at.  tests/test_lz4_synth.py checks the writer against plain_decode,
the oracle and the reference, and that every named edge is hit; tests/test_synth_decode_gpu.py feeds the cases to the GPU
decoders.  Expected results always come from the oracle: plain_decode only checks the writer.

Two generators aim at the DICTIONARY form of the lane-parallel decoder (decode_par.hpp, decode_block_par<false, true>: the
calls with a prepared dictionary, the streams continued across calls and the linked second pass), which the families above
never reach.  seam_cuts() cuts every block above at sequence boundaries: the suffix behind a boundary at output position k,
decoded with the first k bytes as its dictionary, yields the rest, and every structural edge of the case now lies behind a
dictionary -- far matches that the `ok` expression takes (wholly inside the dictionary, spos >= dictLo && spos + ml <= 0) or
hands to decode_block_seq (straddling the seam) in whatever lane, batch and ring position the case had put them.
seam_family() places ONE probe match on the dictionary's edges -- 0..17 bytes in front of its end with every copy width (the
PAR_FAR_WIDE condition spos + 16 <= 0 from both sides, the second load re-anchored at min(16, ml - 16)), straddling its end
by 1..17 bytes, on dictLo and one byte in front of it -- at chosen lanes of a batch, behind PAR_BATCH_OUT and PAR_RING, near
the block's end (outEnd + 64 >= cap) and in blocks too small for the batch loop (cap < 128, srcLen < 64).
tests/test_seam_decode_gpu.py feeds both to the GPU.

Test infrastructure only (imported by tests, like corpus.py).
"""
import random

MINMATCH = 4
LASTLITERALS = 5      # the last 5 bytes of a block are literals
MFLIMIT = 12          # the last match starts at least 12 bytes before the block's end

# the decoders' limits (decode_par.hpp, decode_cu.hpp)
PAR_WIN = 1024
PAR_HIST = 2000
PAR_BATCH_OUT = 2560
PAR_RING = 6144
CU_CHUNK = 16
CU_SUPER = 256
CU_CBIG = 16384
CU_CMAX = 22528
CU_OUTMAX = 32768
CU_TAIL = 512

SHIFTS = (-2, -1, 0, 1, 2)
LIT_LENS = (0, 1, 14, 15, 16, 269, 270, 271, 524, 525, 526, 3000)
ML_LENS = (4, 18, 19, 20, 272, 273, 274, 275, 528, 529, 530, 40000)
SMALL_OFFSETS = tuple(range(1, 10)) + (15, 16, 17, 31, 32, 33)
RING_OFFSETS = tuple(B + d for B in (PAR_HIST, PAR_BATCH_OUT, PAR_RING) for d in (-1, 0, 1))   # 1999..2001, 2559..2561, 6143..6145
SEGMENT_OFFSETS = (32767, 32768, 32769, 65535)
CAP_SLACK = (0, 1, 4, 5, 11, 12, 13, 63, 64, 65, 127, 128, 129)

# Named edges that the families must hit (test_lz4_synth.py recomputes them from the written blocks):
#   output positions (a match end or a literal end at B + s for s in SHIFTS), compressed positions (a token at B + s)
OUT_EDGES = {"cu_segment_32k": [CU_OUTMAX], "par_batch_out": [PAR_BATCH_OUT * k for k in (1, 2, 3, 5, 8)]}
IN_EDGES = {"cu_cbig_16k": [CU_CBIG], "cu_cmax_22k": [CU_CMAX], "par_win": [PAR_WIN * k for k in (1, 2, 3, 7)],
            "cu_chunk_16": [CU_CHUNK * k for k in (3, 17, 64)], "cu_super_256": [CU_SUPER * k for k in (1, 2, 5)]}


def _ext(n):
    """extension bytes of a length field whose nibble is 15 (n = the length - 15)"""
    return b"\xff" * (n // 255) + bytes([n % 255])


def seq_size(lit, ml):
    """compressed bytes of a sequence with lit literals and a match of ml bytes"""
    m = ml - MINMATCH
    return 3 + lit + (len(_ext(lit - 15)) if lit >= 15 else 0) + (len(_ext(m - 15)) if m >= 15 else 0)


def write_block(seqs, last_literals=b"", final=True):
    """seqs: [(literals, offset, match_len)] -> the block, every length written the way the format defines it (nibble, then
    255-runs).  Nothing is checked: offset 0, offsets past the output start or the dictionary, a last match too close to the end,
    too few last literals can all be written.  final=False leaves out the last-literals token (a block that ends with a match)."""
    out = bytearray()
    for lit, off, ml in seqs:
        lit = bytes(lit)
        m = ml - MINMATCH
        if m < 0 or not 0 <= off <= 0xFFFF:
            raise ValueError("match length %d / offset %d cannot be written" % (ml, off))
        out.append((min(len(lit), 15) << 4) | min(m, 15))
        if len(lit) >= 15:
            out += _ext(len(lit) - 15)
        out += lit
        out += off.to_bytes(2, "little")
        if m >= 15:
            out += _ext(m - 15)
    if final:
        n = len(last_literals)
        out.append(min(n, 15) << 4)
        if n >= 15:
            out += _ext(n - 15)
        out += bytes(last_literals)
    return bytes(out)


def parse(block):
    """[(token_pos, lit_start, lit_len, offset, match_len, out_pos)] of a block, read from its bytes; the last sequence (the
    last literals) has offset and match_len None; a block that ends with a match has no such entry.  Raises ValueError where
    the block ends inside a field."""
    res, ip, op, n = [], 0, 0, len(block)

    def length(ip, v):
        if v == 15:
            while True:
                if ip >= n:
                    raise ValueError("length runs past the block")
                b = block[ip]
                ip += 1
                v += b
                if b != 255:
                    break
        return ip, v

    while ip < n:
        tp = ip
        t = block[ip]
        ip, lit = length(ip + 1, t >> 4)
        ls = ip
        ip += lit
        if ip == n:
            res.append((tp, ls, lit, None, None, op))
            return res
        if ip + 2 > n:
            raise ValueError("offset past the block")
        off = block[ip] | (block[ip + 1] << 8)
        ip, ml = length(ip + 2, t & 15)
        ml += MINMATCH
        res.append((tp, ls, lit, off, ml, op))
        op += lit + ml
    return res


def plain_decode(block, cap, dict_bytes=b""):
    """(decoded length, bytes) of a VALID block, or (-1, b"") where the format's rules (as the reference's safe decoder applies
    them against a capacity of cap bytes) reject it.  A byte-at-a-time decoder that shares nothing with the oracle: it checks
    the writer.  Exact negative codes come from oracle.decompress_block."""
    dict_bytes = bytes(dict_bytes)[-65536:] if dict_bytes else b""
    out = bytearray()
    ip, n = 0, len(block)
    try:
        while True:
            t = block[ip]
            ip += 1
            lit = t >> 4
            if lit == 15:
                while True:
                    b = block[ip]
                    ip += 1
                    lit += b
                    if b != 255:
                        break
            end = len(out) + lit
            if end > cap - MFLIMIT or ip + lit > n - (2 + 1 + LASTLITERALS):
                # the last literals: they end the input exactly and fit
                if ip + lit != n or end > cap:
                    return -1, b""
                out += block[ip:ip + lit]
                return len(out), bytes(out)
            out += block[ip:ip + lit]
            ip += lit
            off = block[ip] | (block[ip + 1] << 8)
            ip += 2
            ml = t & 15
            if ml == 15:
                while True:
                    if ip > n - LASTLITERALS:
                        return -1, b""
                    b = block[ip]
                    ip += 1
                    ml += b
                    if b != 255:
                        break
            ml += MINMATCH
            if off > len(out) + len(dict_bytes):
                return -1, b""
            if len(out) + ml > cap - LASTLITERALS:
                return -1, b""
            if off == 0:                              # the reference (v1.9.3) writes zeros for offset 0
                out += bytes(ml)
                continue
            s = len(out) - off
            if s >= 0 and off >= ml:                  # (the source lies in the output and ends before the match starts: a slice)
                out += out[s:s + ml]
                continue
            for _ in range(ml):                       # one byte at a time: overlapping matches repeat their source
                s = len(out) - off
                out.append(out[s] if s >= 0 else dict_bytes[len(dict_bytes) + s])
    except IndexError:
        return -1, b""


class Case:
    """One block: family, name (the edge it aims at), the block's bytes, the capacity to decode it with, whether it was written to
    be valid, whether the workgroup-per-block decoder is meant to keep it (why 0, a first segment with sequences)."""
    __slots__ = ("family", "name", "block", "cap", "valid", "form")

    def __init__(self, family, name, block, cap, valid=True, form=False):
        self.family, self.name, self.block, self.cap, self.valid, self.form = family, name, block, cap, valid, form

    def __repr__(self):
        return "Case(%s/%s, %d -> %d)" % (self.family, self.name, len(self.block), self.cap)


class Builder:
    """Sequences of one block with their running positions: ip = compressed bytes written so far, op = output bytes."""

    def __init__(self, rng, dict_len=0):
        self.rng, self.dict_len = rng, dict_len
        self.seqs, self.ip, self.op = [], 0, 0

    def lit(self, n):
        # (printable bytes, as in text: random bytes read as tokens start more speculative chains than compressor output has)
        return bytes(self.rng.randrange(0x20, 0x7F) for _ in range(n))

    def add(self, lit, off, ml):
        if isinstance(lit, int):
            lit = self.lit(lit)
        self.seqs.append((lit, off, ml))
        self.ip += seq_size(len(lit), ml)
        self.op += len(lit) + ml
        return self

    def fill(self, out_bytes=None, in_bytes=None, max_off=4000, max_ml=40):
        """plain self-contained sequences (0-8 literals, a match of 4..max_ml bytes inside the block) until op or ip has grown by
        about as much"""
        op0, ip0 = self.op, self.ip
        while (out_bytes is not None and self.op - op0 < out_bytes) or (in_bytes is not None and self.ip - ip0 < in_bytes):
            lit = self.rng.randrange(9) if self.op else 8
            off = self.rng.randint(1, min(self.op + lit, max_off))
            self.add(lit, off, self.rng.randint(4, max_ml))
        return self

    def pad_in(self, target):
        """plain sequences until ip == target exactly (target - ip must be 0 or >= 3)"""
        d = target - self.ip
        if d < 0 or d in (1, 2):
            raise ValueError("cannot pad %d compressed bytes" % d)
        while d:
            lit = d - 3 if d <= 17 else (14 if d >= 20 else 8)
            self.add(lit, self.rng.randint(1, min(self.op + lit, 4000)), self.rng.randint(4, 18))
            d = target - self.ip
        return self

    def pad_out(self, target):
        """plain sequences until op == target exactly (target - op must be 0 or >= 4)"""
        d = target - self.op
        if d < 0 or d in (1, 2, 3):
            raise ValueError("cannot pad %d output bytes" % d)
        while d:
            ml = d if d <= 18 else (16 if d >= 22 else 12)
            self.add(0, self.rng.randint(1, min(self.op, 4000)), ml)
            d = target - self.op
        return self

    def block(self, last=12):
        tail = self.lit(last) if isinstance(last, int) else last
        return write_block(self.seqs, tail), self.op + len(tail)


def _case(family, name, b, valid=True, form=True, last=12):
    blk, n = b.block(last)
    return Case(family, name, blk, n, valid, form)


def length_family(seed=1):
    """literal runs and matches at the boundaries between 0, 1, 2 and 3+ extension bytes (decode_par takes one -- up to 269 / 273
    --, the workgroup form's parse two -- up to 524 / 528), alone and both in one sequence"""
    rng = random.Random(seed)
    cases = []
    for L in LIT_LENS:
        b = Builder(rng).fill(out_bytes=1500)
        b.add(L, rng.randint(1, 1000), 6).fill(out_bytes=600).add(L, rng.randint(1, 1000), 300).fill(out_bytes=1500)
        cases.append(_case("lengths", "lit %d" % L, b))
    for M in ML_LENS:
        b = Builder(rng).fill(out_bytes=1500)
        b.add(3, rng.randint(1, 1000), M).fill(out_bytes=600).add(0, rng.choice((1, 7, 600)), M).fill(out_bytes=1500)
        cases.append(_case("lengths", "match %d" % M, b))
    for L, M in ((269, 273), (270, 274), (524, 528), (525, 529), (526, 530), (14, 18), (15, 19)):
        b = Builder(rng).fill(out_bytes=1500)
        for _ in range(4):
            b.add(L, rng.randint(1, min(2000, b.op + L)), M).fill(out_bytes=300)
        cases.append(_case("lengths", "lit %d + match %d" % (L, M), b))
    return cases


def offset_family(seed=2):
    """self-overlapping matches across the 4/8/16-byte copy widths; offsets at the lane-parallel ring's history, batch and ring
    sizes, at the workgroup form's 32 KiB segment, 65535; offsets that reach exactly the output's first byte, and one past it"""
    rng = random.Random(seed)
    cases = []
    for off in SMALL_OFFSETS:
        b = Builder(rng).fill(out_bytes=800)
        for ml in sorted({off + 1, 2 * off + 3, 3 * off + 17, 40, 100, 273, 500}):
            b.add(rng.choice((0, 1, 5)), off, max(ml, 4)).fill(out_bytes=64)
        b.fill(out_bytes=800)
        cases.append(_case("offsets", "offset %d" % off, b))
    for group in (RING_OFFSETS[:3], RING_OFFSETS[3:6], RING_OFFSETS[6:], SEGMENT_OFFSETS):
        b = Builder(rng).fill(out_bytes=max(group) + 200, max_off=8000)
        for off in group:
            for ml in (4, 20, 100, 273):
                b.add(rng.randrange(4), off, ml).fill(out_bytes=rng.randint(40, 3000), max_off=8000)
        b.fill(out_bytes=2000)
        cases.append(_case("offsets", "offsets %s" % "/".join(map(str, group)), b))
    # exactly to the output's first byte (valid) and one further (invalid: no dictionary), early and deep in the block
    for at in (40, 3000, 40000):
        for past in (0, 1):
            b = Builder(rng).fill(out_bytes=at)
            L = 3
            b.add(L, b.op + L + past, 24).fill(out_bytes=3000)
            cases.append(_case("offsets", "offset to output start%s @%d" % (" + 1" if past else "", at), b, valid=not past,
                               form=not past))
    return cases


def placement_family(seed=3):
    """tokens, match ends and literal ends exactly on the decoders' boundaries, shifted by -2..2 bytes"""
    rng = random.Random(seed)
    cases = []
    for s in SHIFTS:
        # output: the workgroup form's 32 KiB segment -- a match ending on it, and a literal run ending on it
        for what in ("match end", "literal end"):
            b = Builder(rng).fill(out_bytes=CU_OUTMAX - 400)
            if what == "match end":
                b.pad_out(CU_OUTMAX + s - 2 - 20).add(2, rng.randint(1, 3000), 20)
            else:
                b.pad_out(CU_OUTMAX + s - 7).add(7, rng.randint(1, 3000), 8)
            b.fill(out_bytes=6000)
            cases.append(_case("placement", "%s at 32 KiB %+d" % (what, s), b))
        # output: multiples of PAR_BATCH_OUT
        b = Builder(rng)
        for k, B in enumerate(OUT_EDGES["par_batch_out"]):
            b.fill(out_bytes=B - b.op - 200).pad_out(B + s - (k % 3) - 10).add(k % 3, rng.randint(1, 2000), 10)
        b.fill(out_bytes=3000)
        cases.append(_case("placement", "match ends at PAR_BATCH_OUT multiples %+d" % s, b))
        # compressed: tokens on the staging limits, PAR_WIN multiples, chunk and super-chunk boundaries
        for edge in ("cu_cbig_16k", "cu_cmax_22k", "par_win", "cu_chunk_16", "cu_super_256"):
            b = Builder(rng)
            for B in IN_EDGES[edge]:
                if B + s - b.ip > 60:
                    b.fill(in_bytes=B + s - b.ip - 40)
                b.pad_in(B + s).add(rng.randrange(6), rng.randint(1, min(b.op + 1, 3000)), rng.randint(4, 60))
            b.fill(in_bytes=3000)
            cases.append(_case("placement", "token at %s %+d" % (edge, s), b))
        # compressed: a token exactly 512 bytes (+ shift) before the block's end, where the sequential tail takes over
        b = Builder(rng).fill(in_bytes=3000)
        tok = b.ip
        b.add(4, rng.randint(1, 2000), 30)
        b.pad_in(tok + CU_TAIL - s - 13)            # behind it: the last literals' token and its 12 literals
        cases.append(_case("placement", "token at block end - 512 %+d" % s, b))
    return cases


def self_similar_block(k, m=None, lead=3000):
    """A literal run, one leading match with a real offset, then thousands of copies of one token byte t = (L << 4) | m with
    L = k - 3: every byte of that stretch parses as the same plain sequence of k bytes (L literals t, offset t * 257, a match of
    m + 4), so the speculative chains that start at the k phases never merge; then 16 trailing literals."""
    L = k - 3
    if m is None:
        m = {3: 1, 4: 2, 5: 2, 6: 3, 7: 3, 8: 3}[k]
    t = (L << 4) | m
    off = t * 257
    rng = random.Random(100 + k)
    b = Builder(rng)
    b.add(lead, rng.randint(1, lead), max(4, off - lead + 64))       # enough output in front of the first copy
    body = bytes([t]) * (k * (30000 // k))
    blk = write_block(b.seqs, b"", final=False) + body + write_block([], b.lit(16))
    n = b.op + (len(body) // k) * (L + m + 4) + 16
    return blk, n


def adversarial_family():
    """Parse-adversarial blocks: self-similar token streams (k = 3..8 disjoint speculative chains; k >= 5 is more than the
    workgroup form's 4 candidates per super-chunk; period 3 puts six tokens in some 16-byte chunks, more than its 5 slots); the
    densest valid streams: 3-byte sequences without literals, more of them in 32 KiB than a segment's 4096 records"""
    cases = []
    for k in range(3, 9):
        blk, n = self_similar_block(k)
        cases.append(Case("adversarial", "self-similar period %d" % k, blk, n, True, False))
    rng = random.Random(4)
    for ml in (4, 5, 8):
        b = Builder(rng).add(16, 16, 4)
        while b.op < 60000:
            b.add(0, rng.randint(1, min(b.op, 64)), ml)
        cases.append(_case("adversarial", "dense 3-byte sequences ml %d" % ml, b, form=False))
    return cases


def depth_family(seed=5):
    """Dependence depth: offset-1 runs across segment and batch boundaries (one byte, 32 768 deep in a segment), and chains in
    which every match copies the match in front of it, thousands deep.  (Both are runs of one repeated 3- to 5-byte sequence:
    self-similar token streams whose speculative chains may outnumber the workgroup form's candidates, so only the mixed
    chains are meant to stay in that form.)"""
    rng = random.Random(seed)
    cases = []
    for start in (CU_OUTMAX - 3000, 2 * PAR_BATCH_OUT - 700, 0):
        b = Builder(rng)
        if start:
            b.fill(out_bytes=start)
        b.add(1, 1, 4)
        while b.op < start + 40000:
            b.add(0, 1, rng.choice((4, 17, 273, 500, 528)))
        b.fill(out_bytes=2000)
        cases.append(_case("depth", "offset-1 run from %d" % start, b, form=False))
    for m, count in ((8, 3000), (5, 3500), (16, 2500), (4, 4000)):
        b = Builder(rng).add(m, m, m)                          # literals, then a first copy of them
        for _ in range(count):
            b.add(0, m, m)                                     # every match copies the one in front of it
        b.fill(out_bytes=1000)
        cases.append(_case("depth", "chain of %d matches of %d" % (count, m), b, form=False))
    # a byte copied onwards by matches at varying offsets (a chain that crosses segments, in pieces)
    b = Builder(rng).fill(out_bytes=600)
    while b.op < 90000:
        b.add(rng.randrange(3), min(b.op, rng.choice((1, 3, 7, 30, 200, 2000))), rng.randint(20, 400))
    cases.append(_case("depth", "mixed deep chains", b))
    return cases


def end_family(seed=6):
    """End rules and capacities: valid blocks at capacity n + slack (the reference's loops switch at cap 64 and 128 bytes before
    the end), the last match starting 11, 12 or 13 bytes before the end, 0..6 last literals, a block that ends with a match, and
    blocks too small for the workgroup form"""
    rng = random.Random(seed)
    cases = []
    bases = []
    for out in (6000, 70000):
        b = Builder(rng).fill(out_bytes=out)
        bases.append(("filler %d" % out, b.block(12)))
    b = Builder(rng).fill(out_bytes=3000).add(1, 1, 600)
    bases.append(("long last match", b.block(5)))
    for out in (0, 8, 60, 120, 300):
        b = Builder(rng)
        if out:
            b.add(8, rng.randint(1, 8), 4).fill(out_bytes=out)
        bases.append(("tiny %d" % out, b.block(12)))
    bases.append(("literals only 700", (write_block([], Builder(rng).lit(700)), 700)))
    bases.append(("empty", (write_block([], b""), 0)))
    for name, (blk, n) in bases:
        for slack in CAP_SLACK:
            cases.append(Case("caps", "%s cap +%d" % (name, slack), blk, n + slack, True, False))
    # the last match starts 11, 12, 13 bytes before the end (with 4- and 6-byte matches); 0..6 last literals
    for ml in (4, 6):
        for before in (11, 12, 13):
            b = Builder(rng).fill(out_bytes=4000).add(2, rng.randint(1, 3000), ml)
            last = before - ml
            blk, n = b.block(last)
            cases.append(Case("ends", "last match %d before end (ml %d)" % (before, ml), blk, n, before >= MFLIMIT and last >= LASTLITERALS))
    for last in range(7):
        b = Builder(rng).fill(out_bytes=4000).add(2, rng.randint(1, 3000), 16)
        blk, n = b.block(last)
        cases.append(Case("ends", "%d last literals" % last, blk, n, last >= LASTLITERALS))
    b = Builder(rng).fill(out_bytes=4000).add(2, 100, 16)
    cases.append(Case("ends", "no last literals token", write_block(b.seqs, final=False), b.op, False))
    # offset 0 inside a block (a sequence neither decoder's parallel parse takes; the reference writes zeros for it)
    for at in (2000, 30000):
        b = Builder(rng).fill(out_bytes=at).add(3, 0, 8).fill(out_bytes=2000)
        blk, n = b.block(12)
        cases.append(Case("ends", "offset 0 @%d" % at, blk, n, True))
    return cases


def bail_block(seed=7, out=65536):
    """Literal runs of 600 bytes (three extension bytes: a step of the sequential decoder each), between them a little plain
    output: segments of under 2 KiB, again and again.  Variant 0 takes such a block back to the lane-parallel decoder
    (decode_cu.hpp `bail`, why 6); it compresses far below 15/16, so the kernel does not skip it up front."""
    rng = random.Random(seed)
    b = Builder(rng).fill(out_bytes=300)
    while b.op < out - 2000:
        b.add(600, rng.randint(1, 500), 4)
        # (lengths with one extension byte at most: a second one would keep the sequential decoder going, decode_seq.hpp)
        b.add(2, rng.randint(1, 500), 200).add(1, rng.randint(1, 500), 250).add(3, rng.randint(1, 500), 100)
    b.fill(out_bytes=out - 12 - b.op)
    return b.block(12)


def independent_cases():
    return (length_family() + offset_family() + placement_family() + adversarial_family() + depth_family() + end_family())




# ---- dictionary (linked streams) ---------------------------------------------------------------------------------------------

def dictionary_streams(seed=8):
    """Linked streams, each [(name, block, cap, valid)]: a block's dictionary is the output of the last block in front of it
    that decoded.  Matches reach the predecessor's output exactly at its first byte (offset = position + dictLen, with
    predecessors shorter than 64 KiB), one byte further (an error), straddle the dictionary's end by 1..16 bytes, and sit at
    offsets near 65535 with predecessors shorter and longer than 64 KiB."""
    rng = random.Random(seed)
    streams = []
    for sizes in ((20000, 30000, 9000, 50000, 40000), (70000, 66000, 80000, 65536)):
        b = Builder(rng).fill(out_bytes=sizes[0] - 12)
        blk, n = b.block(12)
        st = [("independent", blk, n, True)]
        for size in sizes[1:]:
            dict_len = n
            reach = min(dict_len, 65535)
            b = Builder(rng, dict_len)
            if dict_len + 3 <= 65535:
                b.add(3, 3 + dict_len, 20)                        # exactly the dictionary's first byte
            for s in range(1, 17):                                # straddling the dictionary's end by s bytes
                lit = rng.randrange(3)
                b.add(lit, b.op + lit + s, max(4, s + rng.choice((1, 4, 20))))
            for off in (65535, 65534, 65000, reach):              # near 65535 (and the dictionary's first byte when it is short)
                if b.op + 2 < off <= reach + b.op + 2 - 8:
                    b.add(2, off, 8)
            at = 65535 - 2 - reach + 16                           # where offset 65535 reaches 16 bytes into the dictionary
            if b.op < at < size - 3000:
                b.fill(out_bytes=at - 40 - b.op, max_off=60000).pad_out(at)
                b.add(2, 65535, 30)                              # deep in the block, still reaching the dictionary
            b.fill(out_bytes=size - 12 - b.op, max_off=60000)
            blk, n = b.block(12)
            st.append(("dictionary of %d bytes" % dict_len, blk, n, True))
        streams.append(st)
    # one byte past the dictionary's first byte (an error), then a block whose dictionary is the last block that decoded
    b = Builder(rng).fill(out_bytes=30000)
    blk, n = b.block(12)
    st = [("independent", blk, n, True)]
    b = Builder(rng, n).add(3, 3 + n + 1, 20).fill(out_bytes=5000)
    blk2, n2 = b.block(12)
    st.append(("dictLen + 1", blk2, n2, False))
    b = Builder(rng, n).add(3, 3 + n, 20).add(1, 1 + 200, 12).fill(out_bytes=5000)
    blk3, n3 = b.block(12)
    st.append(("dictionary behind a failed block", blk3, n3, True))
    streams.append(st)
    return streams


def linked_expect(oracle, stream):
    """the oracle's block-by-block linked decode of [(name, block, cap, valid)]: [(code, bytes or None)]; a block's dictionary is
    the output of the last block in front of it that decoded to at least one byte"""
    d, res = None, []
    for _, blk, cap, _ in stream:
        code, dec = oracle.decompress_block(blk, cap, d)
        res.append((code, dec if code >= 0 else None))
        if code > 0:
            d = dec
    return res


def framed(blocks_caps):
    """8-byte headers (compressed length, decoded length = the block's capacity) in front of every block"""
    return b"".join(len(b).to_bytes(4, "little") + int(c).to_bytes(4, "little") + bytes(b) for b, c in blocks_caps)


# ---- big linked blocks with sparse dependence (linked path 6) ------------------------------------------------------------------

BIG = 1 << 20
SPARSE_STEP = 65535


def _filler_seqs(rng, n, prefix=b""):
    """prefix, then n output bytes that depend on nothing in front of them: plain sequences (0..8 printable literals, a match of
    4..40 bytes whose source lies inside these n bytes), as Builder.fill writes them"""
    seqs, done = [], 0
    while n - done > 60:
        lit = bytes(rng.randrange(0x20, 0x7F) for _ in range(rng.randrange(9) if done else 8))
        ml = rng.randint(4, 40)
        seqs.append((lit, rng.randint(1, min(done + len(lit), 4000)), ml))
        done += len(lit) + ml
    rest = n - done                                   # 1..60: literals, then matches of 4..18 bytes
    lit = bytes(rng.randrange(0x20, 0x7F) for _ in range(rest % 4))
    rest -= len(lit)
    while rest:
        ml = rest if rest <= 18 else (16 if rest >= 20 else 12)
        seqs.append((lit, rng.randint(1, min(done + len(lit), 4000)), ml))
        done += len(lit) + ml
        rest -= ml
        lit = b""
    seqs[0] = (prefix + seqs[0][0], seqs[0][1], seqs[0][2])
    return seqs


def sparse_dependence_stream(nblk=5, stop_after=None, seed=9):
    """A linked stream of nblk blocks of 1 MiB (framed bytes' blocks).  Block 0 starts with 4 non-zero literals; every later
    block starts with a 4-byte match into its predecessor's tail, which a decode against 64 KiB of zeros gets wrong.  Those 4
    bytes are carried forward by a 4-byte match at offset 65535 once per 65535 bytes to the block's end (the last copy 16 bytes
    before it), where the next block picks them up.  Everything between them is self-contained: 65531 bytes that do not depend
    on the dictionary, just under the 64 KiB after which a later pass of the big-block path may stop early (decode_cu.hpp,
    `again`).  stop_after: the 4 bytes are carried only up to this output position, and the block ends in 40 independent
    literals, which the next block's first match copies from: that path's early stop then fires legitimately."""
    rng = random.Random(seed)
    n_dep = BIG // SPARSE_STEP
    last_pos = n_dep * SPARSE_STEP                    # = BIG - 16
    tail = 40 if stop_after is not None else BIG - last_pos - 4
    blocks = []
    for i in range(nblk):
        seqs, prefix, op = [], b"", 4
        if i == 0:
            prefix, op = bytes([0x11, 0x22, 0x33, 0x44]), 0
        else:
            seqs.append((b"", tail + 4 if stop_after is None else tail, 4))
        for k in range(1, n_dep + 1):
            pos = k * SPARSE_STEP
            if stop_after is not None and pos > stop_after:
                break
            seqs += _filler_seqs(rng, pos - op - len(prefix), prefix)
            seqs.append((b"", SPARSE_STEP, 4))
            prefix, op = b"", pos + 4
        if stop_after is not None:
            seqs += _filler_seqs(rng, BIG - tail - op)
        blocks.append(write_block(seqs, bytes(rng.randrange(1, 256) for _ in range(tail))))
    return blocks


# ---- blocks cut at a sequence boundary: the rest of the block behind a dictionary -------------------------------------------------

CUT_POSITIONS = (15, 16, 17, 64, 1000, 65535, 65536, 70000)
CUT_SMALL_CAP = 262144
_CUTS = {}


def literal_block(data):
    """a literals-only block of any length: it decodes to data"""
    return write_block([], bytes(data))


def _cut_indices(seqs):
    """which sequences of a parsed block to cut in front of: the first, the middle and the last one, and the ones that start
    nearest to the output positions CUT_POSITIONS"""
    n = len(seqs)
    idx = {0, n // 2, n - 1}
    ops = [q[5] for q in seqs]
    for p in CUT_POSITIONS:
        idx.add(min(range(n), key=lambda i: (abs(ops[i] - p), i)))
    return sorted(idx)


def seam_cuts(cases=None, seed=10):
    """[(name, dict_bytes, block, cap, valid)]: every case with a match, cut in front of chosen sequences (_cut_indices).  LZ4
    offsets are relative: where the block B decodes to X and a sequence starts at token position tp and output position k,
    B[tp:] decoded with the dictionary X[:k] into cap - k bytes yields X[k:], and every match that reached in front of k now
    reads the dictionary.  A case that plain_decode rejects is cut the same way with k printable bytes as its dictionary; such
    a cut is valid where plain_decode takes it (the offending sequence was cut off).  The name ends in the case's k."""
    key = seed if cases is None else None
    if key is not None and key in _CUTS:
        return _CUTS[key]
    rng = random.Random(seed)
    cuts = []
    for c in (independent_cases() if cases is None else cases):
        seqs = parse(c.block)
        if not any(q[3] is not None for q in seqs):
            continue
        code, X = plain_decode(c.block, c.cap)
        for i in _cut_indices(seqs):
            tp, k = seqs[i][0], seqs[i][5]
            if k > c.cap:
                continue
            blk = c.block[tp:]
            if code >= 0:
                d, valid = X[:k], True
            else:
                d = bytes(rng.randrange(0x20, 0x7F) for _ in range(k))
                valid = plain_decode(blk, c.cap - k, d)[0] >= 0
            cuts.append(("%s/%s @%d" % (c.family, c.name, k), d, blk, c.cap - k, valid))
    if key is not None:
        _CUTS[key] = cuts
    return cuts


def seam_cuts_small(seed=10):
    """the cuts with a capacity of at most CUT_SMALL_CAP bytes"""
    return [c for c in seam_cuts(seed=seed) if c[3] <= CUT_SMALL_CAP]


# ---- one probe match on the dictionary's edges, at chosen places of a block ---------------------------------------------------------

SEAM_DICT_LENS = (1, 4, 15, 16, 17, 31, 100, 4095, 65534, 65535, 65536, 65537, 70000)
SEAM_ML = (4, 5, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 48, 273, 274)
SEAM_GAPS = tuple(range(18))                  # e: bytes between the match's end and the dictionary's end
SEAM_STRADDLES = tuple(range(1, 18))          # s: the match starts s bytes in front of the dictionary's end
SEAM_INDICES = (0, 1, 31, 62, 63, 64, 65)     # the probe's sequence index (lanes 0, 1, 31, 62, 63 of a batch, 0 and 1 of the next)
SEAM_DEPTHS = (PAR_BATCH_OUT + 8, 2 * PAR_BATCH_OUT, PAR_RING + 8)
SEAM_END_DISTANCES = (12, 63, 64, 65, 127, 128, 129)
SEAM_TINY_CAPS = (13, 20, 64, 127, 128, 129)
# what the places other than index 0 and the depths take: (spos + ml, ml) of matches inside the dictionary -- the 4-, 8- and
# 16-byte copies and the two-load one, e = 0, 15, 16 -- and (s, ml) of straddling ones
SEAM_SUBSET_INSIDE = ((0, 4), (-15, 8), (-16, 16), (-15, 33), (-16, 7), (0, 17))
SEAM_SUBSET_STRADDLE = ((1, 5), (15, 19), (16, 17))
_SEAM, _SEAM_DICTS = {}, {}


def seam_dictionary(dict_len):
    """the seam family's dictionary of dict_len bytes (any byte value, from a seed of its own; ONE generator for all its bytes:
    a generator per byte made every dictionary one repeated byte, which a match read from the wrong place also yields)"""
    if dict_len not in _SEAM_DICTS:
        rng = random.Random(7000 + dict_len)
        _SEAM_DICTS[dict_len] = bytes(rng.getrandbits(8) for _ in range(dict_len))
    return _SEAM_DICTS[dict_len]


def seam_probes(dict_len):
    """[(label, spos, match_len, valid)] for a dictionary of dict_len bytes: spos = the match's source relative to the block's
    first output byte"""
    reach = min(dict_len, 65535)
    probes = []
    for e in SEAM_GAPS:
        for ml in SEAM_ML:
            if ml + e <= reach:
                probes.append(("inside e %d ml %d" % (e, ml), -(ml + e), ml, True))
    for s in SEAM_STRADDLES:
        if s <= reach:
            for ml in (s + 1, s + 4, s + 20, 300):
                probes.append(("straddle s %d ml %d" % (s, max(ml, MINMATCH)), -s, max(ml, MINMATCH), True))
    for ml in (4, 20):
        probes.append(("first byte ml %d" % ml, -reach, ml, True))
    if dict_len + 1 <= 65535:
        probes.append(("one in front", -dict_len - 1, 20, False))
    return probes


def _probe(b, spos, ml):
    """the probe sequence at the builder's position: 2 literals (none where the offset would not fit otherwise); False where
    the offset does not fit 16 bits"""
    lit = 2 if b.op + 2 - spos <= 0xFFFF else 0
    if b.op + lit - spos > 0xFFFF:
        return False
    b.add(lit, b.op + lit - spos, ml)
    return True


def _fillers(b, n):
    """n minimal self-contained sequences: 1..4 literals and a match of 4..8 bytes from the block's own output"""
    for _ in range(n):
        lit = b.rng.randrange(1, 5) if b.op else 4
        b.add(lit, b.rng.randint(1, b.op + lit), b.rng.randint(4, 8))
    return b


def seam_family(seed=12):
    """[(name, dict_len, block, cap, valid)]: one probe match per block on the dictionary's edges (seam_probes), everything else
    in the block self-contained.  Places: as sequence 0, 1, 31, 62, 63, 64, 65 of the block; behind PAR_BATCH_OUT + 8,
    2 * PAR_BATCH_OUT and PAR_RING + 8 output bytes; with the match ending 12 .. 129 bytes before the block's end; as the only
    match of blocks of 13 .. 129 bytes and of blocks with fewer than 64 compressed bytes.  Index 0 and the depths take every
    probe, each (e, ml) and (s, ml) with one dictionary length that has room for it, in rotation, and the first-byte and
    one-in-front probes with every length; the other places take SEAM_SUBSET_* with every length.  Not a full product: the
    test recomputes what is hit."""
    if seed in _SEAM:
        return _SEAM[seed]
    rng = random.Random(seed)
    out = []

    def emit(dl, place, label, b, valid, last=12):
        blk, n = b.block(last)
        out.append(("d%d/%s/%s" % (dl, place, label), dl, blk, n, valid))

    # every probe at index 0 and at the depths
    table = {dl: seam_probes(dl) for dl in SEAM_DICT_LENS}
    labels = []
    for dl in SEAM_DICT_LENS:
        for p in table[dl]:
            if p[0] not in labels:
                labels.append(p[0])
    for pi, depth in enumerate((0,) + SEAM_DEPTHS):
        for j, label in enumerate(labels):
            have = [dl for dl in SEAM_DICT_LENS if any(p[0] == label for p in table[dl])]
            if label.startswith(("inside", "straddle")):
                have = [have[(j + pi) % len(have)]]
            for dl in have:
                _, spos, ml, valid = next(p for p in table[dl] if p[0] == label)
                b = Builder(rng, dl)
                if depth:
                    b.fill(out_bytes=depth - 100).pad_out(depth)
                if not _probe(b, spos, ml):
                    continue
                b.fill(out_bytes=400)
                emit(dl, "depth %d" % depth if depth else "index 0", label, b, valid)
    # the subset at the other places
    for dl in SEAM_DICT_LENS:
        reach = min(dl, 65535)
        subset = [("inside e %d ml %d" % (-end, ml), end - ml, ml) for end, ml in SEAM_SUBSET_INSIDE if ml - end <= reach]
        subset += [("straddle s %d ml %d" % (s, ml), -s, ml) for s, ml in SEAM_SUBSET_STRADDLE if s <= reach]
        for label, spos, ml in subset:
            for i in SEAM_INDICES[1:]:
                b = _fillers(Builder(rng, dl), i)
                if _probe(b, spos, ml):
                    emit(dl, "index %d" % i, label, b.fill(out_bytes=400), True)
            for dist in SEAM_END_DISTANCES:
                b = Builder(rng, dl).fill(out_bytes=700)
                if _probe(b, spos, ml):
                    emit(dl, "end %d" % dist, label, b.pad_out(b.op + dist - 12), True)
            for cap in SEAM_TINY_CAPS:
                lit = min(2, cap - 12)
                if lit + ml + LASTLITERALS <= cap:
                    b = Builder(rng, dl).add(lit, lit - spos, ml)
                    emit(dl, "cap %d" % cap, label, b, True, last=cap - b.op)
            if ml >= 16:
                b = Builder(rng, dl).add(3, 3 - spos, ml)
                emit(dl, "short input", label, b, True, last=40)
    _SEAM[seed] = out
    return out
