"""Deterministic inputs aimed at the encoders' structural edges: the format's end rules (no match within the last 12 bytes, 5
last literals), the length codes' extension bytes, overlapping and far offsets, the sequence queue of encode_wave.hpp and
its 16-bit packing, incompressible data.  cases() returns them as plain bytes from a fixed seed; tests/test_encode_cases.py
pins the list on the CPU, tests/test_encode_edges_gpu.py feeds it to every GPU encoder.

must_match marks the cases in which ANY working match finder at acceleration 1 finds a match: runs and periods of 64 bytes
or more, repeated halves of 256 bytes or more, the forced-length `codes`.  It is not set
  - on anything under 64 bytes, nor on the `offsets` distance cases (the reference itself finds nothing in some of them);
  - on the forced match of exactly 4 bytes: the byte behind it differs from the byte behind its source, so a finder that
    hashes five bytes -- the reference's own LZ4_compress_fast_continue (LZ4_hash5 on 64-bit hosts), and encode_wave.hpp's
    tags -- never sees the two positions in one bucket.  Such a finder works; it has no matches of exactly 4 bytes, and the
    oracle finds none in this case (tests/test_encode_cases.py).  The other forced lengths are all of 5 bytes and more.

Test infrastructure only.
"""
import collections
import random

Case = collections.namedtuple("Case", "family name data must_match")

SEED = 20240611
FAMILIES = ("lengths", "ends", "codes", "offsets", "queue", "incompressible")
MAX_TOTAL = 8 << 20

LENGTHS = (list(range(81)) + [127, 128, 129, 191, 192, 193, 199, 200, 201, 4095, 4096, 4097, 8191, 8192, 8193,
                              65535, 65536, 65537, 131071, 131072, 131073])
MATCH_CODES = (4, 5, 18, 19, 20, 273, 274, 275, 528, 529, 65535 + 4, 70000)
LITERAL_CODES = (14, 15, 16, 269, 270, 271, 524, 525, 70000)
PERIODS = (1, 2, 3, 4, 7, 8, 15, 16, 17, 63, 64, 65)
DISTANCES = (65534, 65535, 65536, 65537, 131072)


def _rand(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


def _other(rng, *not_these):
    """a byte that differs from the given ones"""
    while True:
        b = rng.getrandbits(8)
        if b not in not_these:
            return bytes([b])


def _text(rng, n):
    """n bytes of word soup: a vocabulary of 300 words, so every few bytes repeat something close by"""
    words = [bytes(97 + rng.getrandbits(8) % 26 for _ in range(2 + rng.getrandbits(8) % 8)) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += words[rng.getrandbits(16) % len(words)]
        out += b". " if rng.getrandbits(4) == 0 else b" "
    return bytes(out[:n])


def _lengths(rng):
    text = _text(rng, max(LENGTHS))
    for n in LENGTHS:
        yield Case("lengths", "zeros %d" % n, bytes(n), n >= 64)
        yield Case("lengths", "period 3 %d" % n, (b"abc" * (n // 3 + 1))[:n], n >= 64)
        yield Case("lengths", "text %d" % n, text[:n], False)


def _ends(rng):
    for k in range(5, 20):                       # the second copy would start k bytes before the end
        s, filler = _rand(rng, 16), _rand(rng, 40)
        data = s + filler + (s + _rand(rng, 3))[:k]
        yield Case("ends", "copy starts at n-%d" % k, data, False)
    for k in range(9):                           # the second copy ends k bytes before the end
        s, filler = _rand(rng, 16), _rand(rng, 40)
        yield Case("ends", "copy ends at n-%d" % k, s + filler + s + _rand(rng, k), False)
    yield Case("ends", "run to the very end", _rand(rng, 20) + b"\x5a" * 280, True)
    half = _rand(rng, 300)
    yield Case("ends", "half repeated to the very end", half + half, True)


def _forced_match(rng, L):
    """a match of exactly L bytes: the bytes in front of and behind the two copies differ, so neither the forward
    extension nor catching up can lengthen it"""
    if L <= 1000:
        m = _rand(rng, L)
        c0, c1 = _rand(rng, 1), _rand(rng, 1)
        d0, d1 = _other(rng, c0[0]), _other(rng, c1[0])
        return _rand(rng, 32) + c0 + m + c1 + _rand(rng, 20) + d0 + m + d1 + _rand(rng, 16)
    # beyond 65535 bytes the source cannot lie a whole match away: a period of 251 bytes, 251 + L bytes long
    pat = _rand(rng, 251)
    body = (pat * ((251 + L) // 251 + 1))[:251 + L]
    stop = _other(rng, pat[(251 + L) % 251])
    return _other(rng, pat[250]) + body + stop + _rand(rng, 16)


def _forced_literals(rng, n):
    """two matches with exactly n random literals between them"""
    m1, c0, c1 = _rand(rng, 8), _rand(rng, 1), _rand(rng, 1)
    d0 = _other(rng, c0[0])
    if n <= 1000:
        m2, e0, e1 = _rand(rng, 8), _rand(rng, 1), _rand(rng, 1)
        run = _other(rng, c1[0]) + _rand(rng, n - 2) + _other(rng, e0[0])
        return (_rand(rng, 32) + c0 + m1 + c1 + _rand(rng, 8) + e0 + m2 + e1 + _rand(rng, 8) + d0 + m1 + run + m2 +
                _other(rng, e1[0]) + _rand(rng, 16))
    # a long run: the second match's source lies inside it (a source in front of it would be too far away), and the
    # match is long: a finder that has missed for 70 000 bytes takes steps of about 46 bytes, enters the source's positions
    # that far apart and probes the copy as sparsely, so the two meet only once their phases have drifted together
    m2, e0, e1 = _rand(rng, 6000), _rand(rng, 1), _rand(rng, 1)
    inner = e0 + m2 + e1
    run = _other(rng, c1[0]) + _rand(rng, n - len(inner) - 102) + inner + _rand(rng, 100) + _other(rng, e0[0])
    assert len(run) == n
    return _rand(rng, 32) + c0 + m1 + c1 + _rand(rng, 8) + d0 + m1 + run + m2 + _other(rng, e1[0]) + _rand(rng, 16)


def _codes(rng):
    for L in MATCH_CODES:
        yield Case("codes", "match of %d" % L, _forced_match(rng, L), L >= 5)
    for n in LITERAL_CODES:
        yield Case("codes", "literal run of %d" % n, _forced_literals(rng, n), True)


def _offsets(rng):
    for p in PERIODS:
        pat = _rand(rng, p)
        yield Case("offsets", "period %d" % p, _rand(rng, 9) + (pat * (1000 // p + 1))[:1000] + _rand(rng, 15), True)
    for d in DISTANCES:                          # a 64-byte string again at distance d, text between
        s = _rand(rng, 64)
        yield Case("offsets", "distance %d" % d, _text(rng, 100) + s + _text(rng, d - 64) + s + _text(rng, 100), False)


def _last_start(rng, n, filler):
    """the last match the format allows: it starts at n - 12 and ends at n - 5.  Its 7 bytes stand a second time 3000
    bytes earlier; 30 random bytes in front of both keep the matches of the filler away from them."""
    s = _rand(rng, 7)
    at = n - 12
    src = at - 3000
    head = filler(rng, src - 30) + _rand(rng, 30) + s
    mid = _other(rng) + filler(rng, at - len(head) - 31) + _rand(rng, 29) + _other(rng, head[src - 1])
    data = head + mid + s + _rand(rng, 5)
    assert len(data) == n and data[at:at + 7] == data[src:src + 7]
    return data


def _queue(rng):
    # minimum matches every 8 bytes: far more than 64 sequences per batch of windows, flush after flush.  Matches of 4 bytes
    # (the format's minimum) and of 5 (the minimum of a finder that hashes five bytes).
    for lit, ml in ((4, 4), (3, 5)):
        pool = _rand(rng, 256)
        out = bytearray(pool)
        while len(out) < 65536:
            j = rng.getrandbits(8) % (256 - ml)
            out += _rand(rng, lit) + pool[j:j + ml]
        yield Case("queue", "%d-byte matches every 8 bytes" % ml, bytes(out[:65536]), True)
    # the limits of the queue's 16-bit fields (SMALLQ): the largest match start and the largest match length of a 64 KiB block
    yield Case("queue", "single match at 65535-12, random filler", _last_start(rng, 65535, _rand), False)
    yield Case("queue", "last match at 65535-12, text filler", _last_start(rng, 65535, _text), False)
    yield Case("queue", "last match at 65536-12, text filler", _last_start(rng, 65536, _text), False)
    yield Case("queue", "zeros 65536: one match of 65530", bytes(65536), True)


def _incompressible(rng):
    for n in (13, 64, 4096, 65536, 65537):
        yield Case("incompressible", "random %d" % n, _rand(rng, n), False)


def cases():
    """The list, the same on every call: [Case(family, name, data, must_match)]."""
    out = []
    for k, family in enumerate((_lengths, _ends, _codes, _offsets, _queue, _incompressible)):
        out += list(family(random.Random(SEED + k)))
    return out
