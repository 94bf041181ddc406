"""Inputs of the frame batch's second test pass (tests/test_frames_corpus_host.py, tests/test_frames_corpus_gpu.py): the
structural corpus and the seam corpus of tests/lz4_synth.py inside frames, frames of more blocks than a wavefront has lanes,
inputs of hundreds of frames, errors placed in different 64-block chunks of one frame, a sweep of stored blocks over size and
alignment, blocks at the four block maxima, and seeded mutations.  Everything is regenerated from seeds; a family is
[(name, input bytes)] with unique names, and what is expected of an input is always frames_model.model's answer.

Checksums cost the pure-Python xxh32 twice (here and in the model), so a frame carries block and content checksums where its
content is at most 64 KiB, every eighth larger frame of a family does, and the content-size flag alternates.

Test infrastructure only (imported by tests, like lz4_synth.py).
"""
import random

import frames_cases as FC
import frames_model as M
import lz4_synth as Z

SMALL = 65536                     # frames of at most this much content carry both checksums
PIECES = (1, 13, 100, 700, 5000, 65536)
WIDE_COUNTS = (63, 64, 65, 127, 128, 129, 300)
DAMAGE_AT = (0, 63, 64, 65, 128, -1)
STORED_N = (1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 527, 528, 529, 1023, 1040, 65535, 65536)
STORED_EDGE = (511, 512, 513, 527, 528, 529)
MUTATION_SEED = 2028
STORED_SEED = 0                   # the order of the sweep's call: with it every residue meets every size around 512 (the host test)


def decode(block, window=b"", strict=True):
    """the bytes a block decodes to behind `window` (offsets may reach into it), or None where a field runs past the block or
    the block ends with a match -- and, if strict, where an offset is 0 or reaches in front of the window; if not, such a match
    stands for zeros, so that the length is what the size rule finds.  Only the builders use it, for the content a frame's
    checksum and size fields are made of: the host test holds it to the model's sizes and bytes."""
    try:
        seqs = Z.parse(bytes(block))
    except ValueError:
        return None
    if not seqs or seqs[-1][3] is not None:
        return None
    out = bytearray(window[-65536:])
    base = len(out)
    for _tp, ls, lit, off, ml, _op in seqs:
        out += block[ls:ls + lit]
        if off is None:
            break
        s = len(out) - off
        if off == 0 or s < 0:
            if strict:
                return None
            out += bytes(ml)
        elif off >= ml:
            out += out[s:s + ml]
        else:
            out += (bytes(out[s:]) * (ml // off + 1))[:ml]
    return bytes(out[base:])


def content_of(blocks, linked):
    """content of a frame of [("c" | "s", bytes)]; a block that does not decode counts as nothing"""
    out = bytearray()
    for kind, b in blocks:
        if kind == "s":
            out += b
        else:
            out += decode(b, bytes(out[-65536:]) if linked else b"", strict=False) or b""
    return bytes(out)


class _Sums:
    """which frames of a family carry checksums (the module's docstring), and the alternating content-size flag"""

    def __init__(self):
        self.big = self.k = 0

    def flags(self, n):
        self.k += 1
        both = n <= SMALL
        if not both:
            both = self.big % 8 == 0
            self.big += 1
        return dict(bsum=both, csum=both, csize=bool(self.k & 1))


def frame(blocks, linked, bid, sums, content=None):
    c = content_of(blocks, linked) if content is None else content
    return FC.build(blocks, c, bid=bid, linked=linked, **sums.flags(len(c))).data


# ---------------------------------------------------------------------------
# A. the structural corpus in frames
# ---------------------------------------------------------------------------
_FRONT_STORED = FC.content("random", 333, 901)
_FRONT_LITERALS = FC.content("text", 1500, 902)


def corpus_independent():
    """every lz4_synth.independent_cases() block as the only block of an independent frame: block-size code 5, and code 4 for
    the 236 whose capacity fits 64 KiB"""
    sums, out = _Sums(), []
    for k, c in enumerate(Z.independent_cases()):
        for bid in (5, 4) if c.cap <= 65536 else (5,):
            out.append(("A/indep-b%d/%d %s/%s" % (bid, k, c.family, c.name), frame([("c", c.block)], False, bid, sums)))
    return out


def corpus_linked():
    """the same blocks as the third block of a linked frame, behind a stored block and a literal-only block of other bytes"""
    sums, out = _Sums(), []
    for k, c in enumerate(Z.independent_cases()):
        blocks = [("s", _FRONT_STORED), ("c", FC.lit_block(_FRONT_LITERALS)), ("c", c.block)]
        content = content_of(blocks, True)
        for bid in (5, 4) if c.cap <= 65536 else (5,):
            out.append(("A/linked-b%d/%d %s/%s" % (bid, k, c.family, c.name), frame(blocks, True, bid, sums, content)))
    return out


# ---------------------------------------------------------------------------
# B. the seam corpus as linked frames
# ---------------------------------------------------------------------------
def ragged(d, rng):
    """the dictionary as blocks of ragged sizes, alternately stored and literal-only"""
    blocks, at = [], 0
    while at < len(d):
        n = min(rng.choice(PIECES), len(d) - at)
        piece = d[at:at + n]
        blocks.append(("s", piece) if len(blocks) % 2 == 0 else ("c", FC.lit_block(piece)))
        at += n
    return blocks


def _seam(tag, cases, seed):
    rng, sums, out = random.Random(seed), _Sums(), []
    for k, (name, d, blk) in enumerate(cases):
        blocks = ragged(d, rng) + [("c", blk)]
        content = d + (decode(blk, d, strict=False) or b"")
        out.append(("B/%s/%d %s" % (tag, k, name), frame(blocks, True, 5, sums, content)))
    return out


def seam_cut_frames(seed=7):
    return _seam("cut", [(n, d, blk) for n, d, blk, _cap, _v in Z.seam_cuts()], seed)


def seam_family_frames(seed=7):
    return _seam("family", [(n, Z.seam_dictionary(dl), blk) for n, dl, blk, _cap, _v in Z.seam_family()], seed + 1)


def one_in_front_behind_a_frame(seed=7):
    """every "one in front" probe of the 100-byte dictionary as the SECOND frame of an input: the byte in front of its frame is
    the last byte of a frame that decodes to real bytes"""
    rng, out = random.Random(seed + 2), []
    first = FC.content("text", 777, 903)
    for k, (name, dl, blk, _cap, _v) in enumerate(Z.seam_family()):
        if dl == 100 and "one in front" in name:
            d = Z.seam_dictionary(dl)
            f1 = FC.build([("s", first[:300]), ("c", FC.lit_block(first[300:]))], first, linked=bool(k & 1), bsum=True, csum=True).data
            f2 = FC.build(ragged(d, rng) + [("c", blk)], d, bid=5, linked=True).data
            out.append(("B/behind/%d %s" % (k, name), f1 + f2))
    return out


# ---------------------------------------------------------------------------
# C. frames wider than a wavefront, inputs of many frames
# ---------------------------------------------------------------------------
def wide_blocks(oracle, n, seed, size=200):
    """n blocks of about `size` bytes of text, each compressed against nothing; every fourth stored, some of those empty, and
    some the one-byte block that decodes to nothing"""
    rng, blocks = random.Random(seed), []
    for i in range(n):
        data = FC.content("text", size - 50 + rng.randrange(100), seed * 1000 + i)
        if i % 4 == 3:
            blocks.append(("s", b"" if i % 16 == 7 else data))
        elif i % 10 == 5:
            blocks.append(("c", b"\x00"))
        else:
            blocks.append(("c", oracle.compress_block(data)))
    return blocks


def flag_frame(blocks, k, bid=4, **kw):
    """the frame of these blocks with flag combination k: 1 linked, 2 block checksums, 4 content checksum, 8 content size"""
    linked = bool(k & 1)
    return FC.build(blocks, content_of(blocks, linked), bid=bid, linked=linked, bsum=bool(k & 2), csum=bool(k & 4), csize=bool(k & 8), **kw)


def truly_linked_blocks(oracle, data, block_len):
    """the blocks of the oracle's linked stream: every block compressed with the data in front of it as dictionary"""
    st = oracle.frame_compress(data, block_len, 1, 8, True)
    blocks, at = [], 0
    while at < len(st):
        n = int.from_bytes(st[at:at + 4], "little")
        blocks.append(("c", st[at + 8:at + 8 + n]))
        at += 8 + n
    return blocks


def wide_frames(oracle):
    out = []
    for n in WIDE_COUNTS:
        for k in range(16):
            out.append(("C/wide/%d blocks flags %d" % (n, k), flag_frame(wide_blocks(oracle, n, 40 + n), k).data))
    for j, (n, bl) in enumerate(((70, 300), (129, 150), (300, 400))):
        data = FC.content("text", n * bl, 950 + j)
        blocks = truly_linked_blocks(oracle, data, bl)
        assert len(blocks) == n and content_of(blocks, True) == data
        out.append(("C/wide/truly linked %d blocks" % n, FC.build(blocks, data, linked=True, bsum=bool(j & 1), csum=True, csize=True).data))
    return out


# the five kinds of error a pair is made of; the first three sit at a block, the last two at the frame's end mark
KINDS = ("bsum", "load", "decode", "csize", "csum")
_LOAD_BLOCKS = (Z.write_block([(b"abcd", 0, 8)], last_literals=b"twelve bytes"), Z.write_block([(b"abcdefgh", 4, 8)], final=False))


def damaged(oracle, n, linked, damages, seed, trailer=True):
    """a frame of n blocks with block checksums, content checksum and content size, damaged: damages = [(kind, block index)]
    (the index of "csize" and "csum" is not used).  "load": a block the size rule refuses (offset 0, or it ends with a match);
    "decode": a block whose size stands and whose match reaches in front of the frame (of the block, in an independent frame);
    "bsum": one bit of the block's checksum; "csize": the declared size one off; "csum": one bit of the content checksum.  The
    declared size and the content checksum are right for what is left of the frame, so that each damage is one error."""
    blocks = wide_blocks(oracle, n, seed)
    pieces = [b if kind == "s" else (decode(b) or b"") for kind, b in blocks]
    for j, (kind, at) in enumerate(damages):
        at %= n
        if kind == "load":
            blocks[at], pieces[at] = ("c", _LOAD_BLOCKS[(at + j) & 1]), b""
        elif kind == "decode":
            blocks[at], pieces[at] = ("c", Z.write_block([(b"wxyz", 65535 if linked else 140, 20)], last_literals=b"twelve bytes")), bytes(36)
    content = b"".join(pieces)
    assert len(content) < 65000                              # (offset 65535 reaches in front of the frame from every block)
    kinds = [k for k, _ in damages]
    built = FC.build(blocks, content, linked=linked, bsum=True, csum=trailer, csize=True,
                     declared=len(content) + (1 if "csize" in kinds else 0))
    data = bytearray(built.data)
    for kind, at in damages:
        if kind == "bsum":
            data[built.pos["block"][at % n][2] + 1] ^= 0x10
        elif kind == "csum":
            data[built.pos["cc"] + 2] ^= 0x04
    return bytes(data)


def single_damages(oracle):
    out = []
    for linked in (True, False):
        for kind in ("bsum", "load", "decode"):
            for at in DAMAGE_AT:
                out.append(("C/one/%s %s at %d" % ("L" if linked else "I", kind, at), damaged(oracle, 300, linked, [(kind, at)], 61)))
    return out


def pair_damages(oracle):
    """[(name, input, (first kind, second kind))]: two errors, the first at the smaller byte position, in different 64-block
    chunks of one 200-block frame -- or, where the first is one of the kinds that sit at a frame's end, in two frames"""
    out = []
    places = ((5, 70), (64, 191), (63, 128))
    j = 0
    for linked in (True, False):
        tag = "L" if linked else "I"
        for x in KINDS:
            for y in KINDS:
                if x in ("csize", "csum") and y in ("csize", "csum") and x == y:
                    continue
                a, b = places[j % len(places)]
                j += 1
                if x in ("csize", "csum"):
                    # the frame-level error first: a frame of its own in front of the frame with the second error
                    data = damaged(oracle, 70, linked, [(x, 0)], 62) + damaged(oracle, 200, linked, [(y, b)], 63)
                else:
                    data = damaged(oracle, 200, linked, [(x, a), (y, b)], 63)
                out.append(("C/pair/%s %s then %s" % (tag, x, y), data, (x, y)))
    return out


def many_frames(oracle):
    """inputs of 70 and 200 frames: one-block and 65-block frames, linked and independent, skippable frames between them; with
    decode-time failures in frames 3 and 150; with a cut and with a bad magic behind 100 good frames"""
    def frames(n, seed, bad=()):
        """[(frame index, or None for a skippable frame, bytes)]"""
        parts = []
        for f in range(n):
            wide = f % 9 == 3
            linked = (f // 2) & 1
            if f in bad:
                fr = damaged(oracle, 65 if wide else 3, bool(linked), [("decode", -1)], seed + f, trailer=bool(f & 1))
            else:
                blocks = wide_blocks(oracle, 65, seed + f, 150) if wide else [("c", oracle.compress_block(FC.content("text", 200 + f, seed + f)))]
                fr = flag_frame(blocks, linked | 2 | ((f % 3 == 0) << 2) | ((f % 5 == 0) << 3)).data
            parts.append((f, fr))
            if f % 7 == 2:
                parts.append((None, FC.skippable(bytes(f % 40), f % 16)))
        return parts

    def join(parts):
        return b"".join(p for _, p in parts)
    good = frames(200, 7000)
    whole = join(good)
    at = sum(len(p) for f, p in good[:[f for f, _ in good].index(100)])      # where frame 100 starts: 100 good frames in front
    end = at + len(dict(good)[100])
    assert whole[at:at + 4] == FC.le32(M.MAGIC)
    return [("C/many/70 frames", join(frames(70, 6000))),
            ("C/many/200 frames", whole),
            ("C/many/200 frames, 3 and 150 fail", join(frames(200, 7000, bad=(3, 150)))),
            ("C/many/cut in frame 100", whole[:end - 3]),
            ("C/many/bad magic at frame 100", whole[:at] + b"\x05" + whole[at + 1:])]


# ---------------------------------------------------------------------------
# D. stored-block sweep
# ---------------------------------------------------------------------------
def stored_sweep():
    """[(name, input, (N, P, linked, bytes from the input's start to the second block's data))]: a frame [stored block of P
    bytes, stored block of N bytes]; the sizes on both sides of wave_copy_bytes' 512-byte threshold come with all four
    combinations of block checksums and content size, which also moves the source by 4, 8 and 12 bytes"""
    out = []
    for N in STORED_N:
        for P in range(16):
            for linked in (True, False):
                for v in (range(4) if N in STORED_EDGE else (P & 3,)):
                    data = FC.content("random", P + N, 100000 + N * 16 + P)
                    b = FC.build([("s", data[:P]), ("s", data[P:])], data, linked=linked, bsum=bool(v & 1), csize=bool(v & 2), csum=N <= 1040)
                    out.append(("D/N %d P %d %s v%d" % (N, P, "L" if linked else "I", v), b.data, (N, P, linked, b.pos["block"][1][1])))
    return out


def run_layout(datas, sizes):
    """where test_frames_gpu.run(..., residues=True) puts the inputs and the outputs, relative to its two buffers (which the
    allocator aligns to far more than 16 bytes): ([inOff], [outOff])"""
    offs, pos = [], 5
    for i, d in enumerate(datas):
        pos += (i % 16 - pos) % 16
        offs.append(pos)
        pos += len(d) + 3
    outs, at = [], 32
    for i, s in enumerate(sizes):
        at += (i * 7) % 16
        outs.append(at)
        at += max(s, 0) + 32
    return offs, outs


# ---------------------------------------------------------------------------
# E. block maxima
# ---------------------------------------------------------------------------
def maximal_block(n, off=8):
    """a compressed block that decodes to exactly n bytes"""
    return Z.write_block([(b"abcdefgh", off, n - 20)], last_literals=b"twelve bytes")


def block_maxima():
    sums, out = _Sums(), []
    for bid in (4, 5, 6, 7):
        bmax = 1 << (8 + 2 * bid)
        for linked in (False, True):
            tag = "b%d %s" % (bid, "L" if linked else "I")
            out.append(("E/%s compressed max" % tag, frame([("c", maximal_block(bmax))], linked, bid, sums)))
            out.append(("E/%s compressed max + 1" % tag, frame([("c", maximal_block(bmax + 1))], linked, bid, sums, b"")))
        stored = FC.content("text", bmax, 300 + bid)
        out.append(("E/b%d stored max" % bid, frame([("s", stored)], bool(bid & 1), bid, sums)))
        whole = FC.build([("s", stored[:100])], stored[:100], bid=bid, linked=False)
        w = whole.pos["block"][0][0]
        out.append(("E/b%d block word max + 1" % bid, whole.data[:w] + FC.le32(0x80000000 | (bmax + 1)) + whole.data[w + 4:]))
        out.append(("E/b%d compressed block word max + 1" % bid, whole.data[:w] + FC.le32(bmax + 1) + whole.data[w + 4:]))
    for bid in (4, 5):
        bmax = 1 << (8 + 2 * bid)
        blocks = [("c", maximal_block(bmax)), ("c", maximal_block(bmax, 65535)), ("c", maximal_block(bmax, 40000))]
        out.append(("E/b%d three maximal blocks linked" % bid, frame(blocks, True, bid, sums)))
    return out


# ---------------------------------------------------------------------------
# F. seeded mutations
# ---------------------------------------------------------------------------
MODES = ("truncate", "bit anywhere", "bit in a size word", "data byte", "bit in the descriptor", "append")


def mutation_bases(oracle):
    out = []
    for k in range(16):
        for n, size in ((70, 300), (5, 3000)):
            out.append(("%dx%d flags %d" % (n, size, k), flag_frame(wide_blocks(oracle, n, 80 + k, size), k)))
    return out


def mutations(oracle, seed=MUTATION_SEED, per_base=24):
    """[(name, input, mode)]: per_base mutations of every base, the six modes in turn"""
    rng, out = random.Random(seed), []
    for bname, b in mutation_bases(oracle):
        for m in range(per_base):
            mode = MODES[m % len(MODES)]
            d = bytearray(b.data)
            blk = b.pos["block"][rng.randrange(len(b.pos["block"]))]
            while mode == "data byte" and int.from_bytes(b.data[blk[0]:blk[0] + 4], "little") & 0x7FFFFFFF < 3:
                blk = b.pos["block"][rng.randrange(len(b.pos["block"]))]
            if mode == "truncate":
                d = d[:rng.randrange(len(d))]
            elif mode == "bit anywhere":
                d[rng.randrange(len(d))] ^= 1 << rng.randrange(8)
            elif mode == "bit in a size word":
                d[blk[0] + rng.randrange(4)] ^= 1 << rng.randrange(8)
            elif mode == "data byte":
                d[blk[1] + rng.randrange(3)] = rng.randrange(256)
            elif mode == "bit in the descriptor":
                d[rng.randrange(b.pos["desc"], b.pos["hc"])] ^= 1 << rng.randrange(8)
            else:
                d += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 9)))
            out.append(("F/%s/%d %s" % (bname, m, mode), bytes(d), mode))
    return out


# ---------------------------------------------------------------------------
# the families by name, built once a process; the order of a call
# ---------------------------------------------------------------------------
FAMILIES = {
    "A-independent": lambda o: corpus_independent(),
    "A-linked": lambda o: corpus_linked(),
    "B-cuts": lambda o: seam_cut_frames(),
    "B-family": lambda o: seam_family_frames(),
    "B-behind": lambda o: one_in_front_behind_a_frame(),
    "C-wide": wide_frames,
    "C-one": single_damages,
    "C-pairs": pair_damages,
    "C-many": many_frames,
    "D": lambda o: stored_sweep(),
    "E": lambda o: block_maxima(),
    "F": mutations,
}
_BUILT = {}


def family(name, oracle):
    """[(name, input bytes, ...)] of a family, the same list object every time"""
    if name not in _BUILT:
        _BUILT[name] = FAMILIES[name](oracle)
        names = [c[0] for c in _BUILT[name]]
        assert len(names) == len(set(names))
    return _BUILT[name]


def shuffled(cases, seed):
    """the cases in the order of one call: shuffled with a fixed seed"""
    cases = list(cases)
    random.Random(seed).shuffle(cases)
    return cases


def stored_residues(ordered):
    """({(N, destination address mod 16)}, {(N, source address mod 16)}) of the sweep's second blocks, for the cases in the
    order of their call"""
    offs, outs = run_layout([c[1] for c in ordered], [c[2][0] + c[2][1] for c in ordered])
    dst = {(c[2][0], (o + c[2][1]) % 16) for c, o in zip(ordered, outs)}
    src = {(c[2][0], (o + c[2][3]) % 16) for c, o in zip(ordered, offs)}
    return dst, src
