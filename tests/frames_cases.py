"""Inputs of the frame batch tests: contents regenerated from seeds, the golden frames liblz4 wrote (tests/golden/
frames_vectors.json, made by tests/golden/make_frames_golden.py), hand-built frames at the window's edges, and one corruption per
code at a named position.

Test infrastructure only (imported by tests, like lz4_synth.py).
"""
import base64
import hashlib
import json
import os
import zlib

import frames_model as M
import lz4_synth as Z

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "frames_vectors.json")

# ---------------------------------------------------------------------------
# contents, from seeds (pure Python: the same bytes wherever the tests run)
# ---------------------------------------------------------------------------
_SENTENCES = [
    b"the quick brown fox jumps over the lazy dog near the river bank. ",
    b"a journey of a thousand miles begins with a single step forward. ",
    b"all that glitters is not gold, and not all who wander are lost. ",
    b"frames carry blocks, blocks carry sequences, sequences carry bytes. ",
    b"to be or not to be, that is the question the decoder never asks. ",
    b"an offset points back into the window, a length says how far to copy. ",
    b"the end mark is a word of zeros and the checksum follows it closely. ",
    b"sixty four kibibytes of history are all a linked block may look at. ",
    b"when in doubt, count the literals, then the match, then count again. ",
    b"a stored block is a block that refused to shrink and says so proudly. ",
    b"every wave walks its own frame while its neighbours walk theirs. ",
    b"nothing is sized by what a header claims, only by what is there. ",
]


def _lcg(seed):
    x = (seed * 2862933555777941757 + 3037000493) & 0xFFFFFFFFFFFFFFFF
    while True:
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        yield x >> 33


def content(kind, n, seed):
    """text: a dozen sentences, mostly in turn, now and then any of them or a number (compresses well, so that the frames are small); random: a hash stream (incompressible);
    rep: one sentence over and over (as compressible as the format allows)."""
    if kind == "random":
        out = bytearray()
        i = 0
        while len(out) < n:
            out += hashlib.sha256(b"frames %d %d" % (seed, i)).digest()
            i += 1
        return bytes(out[:n])
    if kind == "rep":
        s = _SENTENCES[seed % len(_SENTENCES)]
        return (s * (n // len(s) + 1))[:n]
    g = _lcg(seed)
    out = bytearray()
    k = seed
    while len(out) < n:
        r = next(g)
        k = r if r & 0x3C0 == 0 else k + 1              # mostly the next sentence, now and then any
        out += _SENTENCES[k % len(_SENTENCES)]
        if r & 0x3C00 == 0:
            out += b"%d. " % (r >> 14)
    return bytes(out[:n])


# ---------------------------------------------------------------------------
# the golden frames: written once by liblz4, stored as segments -- a zlib'd literal, or a slice of the regenerated content
# (a stored block is one)
# ---------------------------------------------------------------------------
FLUSH_AT = (1000, 5000, 20000, 70000)


def pieces_of(data):
    cuts = [0] + [c for c in FLUSH_AT if c < len(data)] + [len(data)]
    return [data[a:b] for a, b in zip(cuts, cuts[1:])]


def _flag_sets(pick):
    """(linked, block checksum, content checksum, content size, level, writer) for the 16 flag combinations, or those pick keeps;
    the level and the writer alternate so that every value of every option meets every value of every other one somewhere"""
    out = []
    for k in range(16):
        if pick is not None and k not in pick:
            continue
        linked, bsum, csum, csize = k & 1, (k >> 1) & 1, (k >> 2) & 1, (k >> 3) & 1
        level = 9 if ((k >> 1) ^ (k >> 3)) & 1 else 0
        writer = "pieces" if (k ^ (k >> 2)) & 1 else "frame"
        out.append((linked, bsum, csum, csize, level, writer))
    return out


def golden_specs():
    """[(id, kind, n, seed, block id, linked, bsum, csum, csize, level, writer)]"""
    specs = []

    def add(kind, n, bid, combos, both_writers=False, both_levels=False):
        for (linked, bsum, csum, csize, level, writer) in combos:
            for w in (("frame", "pieces") if both_writers else (writer,)):
                for lv in ((0, 9) if both_levels else (level,)):
                    ident = "%s%d-b%d-%s%s%s%s-l%d-%s" % (kind, n, bid, "L" if linked else "I", "B" if bsum else "", "C" if csum else "",
                                                          "S" if csize else "", lv, w)
                    specs.append((ident, kind, n, len(specs) + 1, bid, linked, bsum, csum, csize, lv, w))

    for n in (0, 1, 12, 13):
        add("text", n, 4, _flag_sets(None), both_writers=True, both_levels=(n == 13))
    for n in (65535, 65536, 65537):
        add("text", n, 4, _flag_sets((0, 3, 5, 10, 12, 15)))
    add("text", 3 * 65536 + 5, 4, _flag_sets((1, 2, 4, 11, 13, 14)))
    add("random", 70000, 4, _flag_sets((0, 3, 5, 6, 9, 10, 12, 15)))
    add("rep", 4 * (1 << 20) + 99, 7, _flag_sets((6, 9)))
    # flushes inside a linked frame: the window spans several short blocks
    add("text", 90000, 4, [(1, 0, 1, 0, 0, "pieces"), (1, 1, 1, 1, 9, "pieces")])
    return specs


def encode_segments(frame, data):
    """the frame as segments: stored blocks that are slices of the content become references"""
    frames, err = M.walk(frame)
    assert err is None
    cuts = []
    at = 0
    for f in frames:
        for (p, stored, payload, _ck) in f.blocks:
            if stored and len(payload) >= 64:
                i = data.find(payload, at)
                if i >= 0:
                    cuts.append((p + 4, len(payload), i))
            at += len(payload) if stored else 0
    segs, pos = [], 0
    for (start, n, src) in cuts:
        if start > pos:
            segs.append(["z", base64.b64encode(zlib.compress(frame[pos:start], 9)).decode()])
        segs.append(["c", src, n])
        pos = start + n
    if pos < len(frame) or not segs:
        segs.append(["z", base64.b64encode(zlib.compress(frame[pos:], 9)).decode()])
    return segs


def decode_segments(segs, data):
    out = bytearray()
    for s in segs:
        out += zlib.decompress(base64.b64decode(s[1])) if s[0] == "z" else data[s[1]: s[1] + s[2]]
    return bytes(out)


_golden_cache = None


def golden():
    """[(id, frame bytes, content bytes)], contents regenerated and checked against the stored hashes"""
    global _golden_cache
    if _golden_cache is None:
        with open(GOLDEN) as f:
            doc = json.load(f)
        res = []
        for v in doc["vectors"]:
            data = content(v["kind"], v["n"], v["seed"])
            assert hashlib.sha256(data).hexdigest()[:16] == v["sha"], v["id"]
            res.append((v["id"], decode_segments(v["segs"], data), data))
        _golden_cache = res
    return _golden_cache


# ---------------------------------------------------------------------------
# hand-built frames
# ---------------------------------------------------------------------------
def le32(v):
    return int(v & 0xFFFFFFFF).to_bytes(4, "little")


def header(bid=4, linked=True, bsum=False, csum=False, csize=None, flg_or=0, bd_or=0, version=1, hc_xor=0):
    flg = (version << 6) | (0 if linked else 0x20) | (0x10 if bsum else 0) | (8 if csize is not None else 0) | (4 if csum else 0) | flg_or
    desc = bytes([flg, (bid << 4) | bd_or]) + (int(csize).to_bytes(8, "little") if csize is not None else b"")
    return le32(M.MAGIC) + desc + bytes([((M.xxh32(desc) >> 8) & 0xFF) ^ hc_xor])


class Built:
    """A frame and where its parts lie: pos["magic"], pos["desc"], pos["hc"], pos["block"][i] = (size word, data, checksum or
    None), pos["end"], pos["cc"]"""

    def __init__(self, data, pos, content_bytes):
        self.data, self.pos, self.content = data, pos, content_bytes


def build(blocks, content_bytes, bid=4, linked=True, bsum=False, csum=False, csize=False, declared=None, **hdr):
    """blocks: [("c", compressed bytes) | ("s", stored bytes)]"""
    n = len(content_bytes) if declared is None else declared
    out = bytearray(header(bid, linked, bsum, csum, n if (csize or declared is not None) else None, **hdr))
    pos = {"magic": 0, "desc": 4, "hc": len(out) - 1, "block": []}
    for kind, b in blocks:
        w = len(out)
        out += le32(len(b) | (0x80000000 if kind == "s" else 0)) + bytes(b)
        ck = None
        if bsum:
            ck = len(out)
            out += le32(M.xxh32(b))
        pos["block"].append((w, w + 4, ck))
    pos["end"] = len(out)
    out += le32(0)
    pos["cc"] = None
    if csum:
        pos["cc"] = len(out)
        out += le32(M.xxh32(content_bytes))
    return Built(bytes(out), pos, bytes(content_bytes))


def skippable(payload, k=0):
    return le32(0x184D2A50 + k) + le32(len(payload)) + bytes(payload)


def lit_block(data):
    return Z.write_block([], last_literals=data)


def _decode_linked(blocks):
    """the content of a linked frame of hand-built blocks, by lz4_synth's byte-at-a-time decoder"""
    out = bytearray()
    for kind, b in blocks:
        if kind == "s":
            out += b
        elif b:
            r, got = Z.plain_decode(b, 1 << 22, bytes(out[-65536:]))
            assert r >= 0
            out += got
    return bytes(out)


def valid_cases(oracle):
    """[(name, input bytes, content)]"""
    cases = []
    a100, b50 = content("text", 100, 71), content("random", 50, 72)
    third = Z.write_block([(b"wxyz", 140, 20)], last_literals=b"twelve bytes")
    for first in ("s", "c"):
        blocks = [(first, a100 if first == "s" else lit_block(a100)), ("c", lit_block(b50)), ("c", third)]
        c = _decode_linked(blocks)
        assert c[154:174] == a100[14:34]
        cases.append(("through-short-block-%s" % first, build(blocks, c, csum=True, csize=True).data, c))
    big = content("random", 65536, 73)
    far = Z.write_block([(b"q", 65535, 8)], last_literals=b"0123456789ab")
    blocks = [("s", big), ("c", far)]
    c = _decode_linked(blocks)
    assert c[65537:65545] == big[2:10]
    cases.append(("offset-65535-across-seam", build(blocks, c, csum=True).data, c))
    w400 = content("text", 400, 74)
    long_match = Z.write_block([(b"", 350, 300)], last_literals=b"5last")
    blocks = [("c", oracle.compress_block(w400)), ("c", long_match)]
    c = _decode_linked(blocks)
    assert len(c) == 705
    cases.append(("long-match-from-window-ends-5-before-end", build(blocks, c, bsum=True, csum=True, csize=True).data, c))
    t3000 = content("text", 3000, 75)
    blocks = [("c", oracle.compress_block(t3000)), ("s", b""), ("s", b50)]
    for linked in (True, False):
        cases.append(("empty-stored-block-%s" % ("L" if linked else "I"),
                      build(blocks, t3000 + b50, linked=linked, bsum=True, csum=True).data, t3000 + b50))
    empty = build([], b"", csum=True).data
    cases.append(("empty-frame", empty, b""))
    cases.append(("skippable-only", skippable(b"abc") + skippable(b"", 15) + skippable(bytes(300), 7), b""))
    cases.append(("empty-input", b"", b""))
    f1 = build([("c", oracle.compress_block(t3000))], t3000, linked=False, csize=True).data
    f2 = build([("s", b50)], b50, bsum=True).data
    cases.append(("three-frames-two-skippables", f1 + skippable(b"x" * 17, 3) + f2 + skippable(b"") + empty, t3000 + b50))
    cases.append(("declared-size-zero", build([], b"", csize=True).data, b""))
    return cases


def corrupt_cases(oracle):
    """[(name, input bytes, code or None: the model decides)]"""
    E = M
    t3000, r100, t2000 = content("text", 3000, 81), content("random", 100, 82), content("text", 2000, 83)
    blocks = [("c", oracle.compress_block(t3000)), ("s", r100), ("c", oracle.compress_block(t2000))]
    body = t3000 + r100 + t2000
    base = build(blocks, body, linked=False, bsum=True, csum=True, csize=True)
    plain = build(blocks, body, linked=False, csum=True)                      # no block checksums, no content size
    d, p = base.data, base.pos

    def flip(data, at, x=0x01):
        b = bytearray(data)
        b[at] ^= x
        return bytes(b)

    def hdr(**kw):
        return build(blocks, body, linked=False, bsum=True, csum=True, csize=True, **kw).data

    w0, d0, c0 = p["block"][0]
    w1, d1, c1 = p["block"][1]
    cases = [
        ("magic-flipped", flip(d, 1), E.E_MAGIC),
        ("version-00", hdr(version=0), E.E_HEADER),
        ("reserved-flg-bit", hdr(flg_or=2), E.E_HEADER),
        ("dictid-bit", hdr(flg_or=1), E.E_HEADER),
        ("bd-code-3", build(blocks, body, bid=3, linked=False).data, E.E_HEADER),
        ("reserved-bd-bit", hdr(bd_or=1), E.E_HEADER),
        ("header-checksum", hdr(hc_xor=0x40), E.E_HEADER_CHECKSUM),
        ("block-word-max-plus-1", d[:w1] + le32(0x80000000 | 65537) + d[w1 + 4:], E.E_BLOCK_SIZE),
        ("cut-in-magic", d[:3], E.E_TRUNCATED),
        ("cut-in-descriptor", d[:5], E.E_TRUNCATED),
        ("cut-in-content-size", d[:10], E.E_TRUNCATED),
        ("cut-in-block-word", d[:w1 + 2], E.E_TRUNCATED),
        ("cut-in-block-data", d[:d0 + 50], E.E_TRUNCATED),
        ("cut-in-block-checksum", d[:c0 + 2], E.E_TRUNCATED),
        ("cut-before-end-mark", d[:p["end"]], E.E_TRUNCATED),
        ("cut-in-content-checksum", d[:p["cc"] + 1], E.E_TRUNCATED),
        ("block-checksum-flipped", flip(d, c1), E.E_BLOCK_CHECKSUM),
        ("data-byte-flipped-literal", flip(plain.data, plain.pos["block"][0][1] + 2), None),
        ("data-byte-flipped-stored", flip(plain.data, plain.pos["block"][1][1] + 5), E.E_CONTENT_CHECKSUM),
        ("data-byte-flipped-late", flip(plain.data, plain.pos["block"][2][1] + 40, 0xFF), None),
        ("declared-one-too-large", build(blocks, body, linked=False, bsum=True, csum=True, declared=len(body) + 1).data, E.E_CONTENT_SIZE),
        ("declared-one-too-small", build(blocks, body, linked=False, bsum=True, csum=True, declared=len(body) - 1).data, E.E_CONTENT_SIZE),
        ("content-checksum-flipped", flip(d, p["cc"] + 3), E.E_CONTENT_CHECKSUM),
        ("trailing-garbage", d + b"garbage!", E.E_MAGIC),
        ("trailing-three-bytes", d + b"\x04\x22\x4d", E.E_TRUNCATED),
        ("two-errors-earlier-wins", flip(d, c0) + b"\x05" + d[1:], E.E_BLOCK_CHECKSUM),
        ("offset-zero", build([("c", Z.write_block([(b"abcd", 0, 8)], last_literals=b"twelve bytes"))], b"", csize=False).data, E.E_BLOCK),
        ("block-ends-with-match", build([("c", Z.write_block([(b"abcdefgh", 4, 8)], final=False))], b"").data, E.E_BLOCK),
    ]
    # a match that reaches in front of the frame's first byte: the size stands, the decode does not
    a100 = content("text", 100, 84)
    third = Z.write_block([(b"wxyz", 140, 20)], last_literals=b"twelve bytes")
    cases.append(("reaches-in-front-of-the-frame", build([("s", a100), ("c", third)], b"").data, E.E_BLOCK))
    cases.append(("reaches-in-front-of-an-independent-block",
                  build([("s", a100), ("c", lit_block(a100[:50])), ("c", third)], b"", linked=False).data, E.E_BLOCK))
    # a linked frame's window is its own: the frame in front is not in it
    cases.append(("window-ends-at-the-frame", build([("s", a100 + a100)], a100 + a100).data + build([("c", third)], b"").data, E.E_BLOCK))
    return cases
