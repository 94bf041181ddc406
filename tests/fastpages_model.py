"""The contract of the fast fixed-size output pages (mi355lz4_compress_pages_fast_device, include/mi355lz4.h) in plain
Python: what a page holds, given the block E that the engine writes for the slice, the slice's length n and the page size T.

    E = s_0 .. s_{m-1} (literals, offset, match) and a last literal run.
    |E| <= T: the page is E and consumes n.
    Otherwise the page is s_0 .. s_j of E, byte for byte, and one literal run of r_j = min(n - inEnd_j, lit(T - outEnd_j)) bytes:
    j is the LAST sequence in parse order with a valid cut behind it -- outEnd_j + 1 <= T, r_j >= 5 and
    matchStart_j + 12 <= inEnd_j + r_j --, or -1 (no sequence, outEnd = inEnd = 0), which is always valid.

The model knows nothing of the kernel: it walks E's bytes and applies the rule.  Any conforming block serves as E (the oracle's, a
hand-built one, the GPU's own batch encoder's).

Test infrastructure only.
"""
from lz4_check import LASTLITERALS, MFLIMIT, MINMATCH


def ext(length):
    """bytes of the length continuation of a literal or match field (ext_len_bytes in encode_wave.hpp)"""
    return 1 + (length - 15) // 255 if length >= 15 else 0


def lit(s):
    """the largest r >= 0 with 1 + ext(r) + r <= s: the longest literal run whose token, length bytes and bytes fit in s bytes;
    -1 when not even a token fits.  By search, from the definition."""
    if s < 1:
        return -1
    r = s - 1
    while 1 + ext(r) + r > s:
        r -= 1
    return r


def lit_closed_form(s):
    """the same in the closed form the kernel computes (page_lit_fit); tests/test_fastpages_host.py holds it to lit()"""
    if s <= 16:
        return min(s - 1, 14)
    w = s - 17
    return 15 + w - (w + 1) // 256


def min_progress(t):
    """7k's progress bound: what the all-literals page of t bytes holds"""
    return (t - 1) - (t + 240) // 256


def iter_sequences(block, n):
    """(matchStart, inEnd, outEnd) of the sequences of `block` that have a match, in parse order.  The block must be a valid one
    that decodes to n bytes (lz4_check.check_block says whether it is)."""
    block = bytes(block)
    i = pos = 0

    def length(i, v):
        if v == 15:
            while True:
                b = block[i]
                i += 1
                v += b
                if b != 255:
                    break
        return i, v

    while True:
        tok = block[i]
        i, ll = length(i + 1, tok >> 4)
        i += ll
        if pos + ll == n:
            assert i == len(block) and not tok & 15
            return
        pos += ll
        i, ml = length(i + 2, tok & 15)
        ml += MINMATCH
        yield pos, pos + ml, i
        pos += ml


def sequences(block, n):
    """[(matchStart, inEnd, outEnd)] of all of them, and the input position where the last literal run starts"""
    seqs = list(iter_sequences(block, n))
    return seqs, (seqs[-1][1] if seqs else 0)


def literal_run(data):
    """a block's last sequence: the token, the length bytes and the bytes of a literal run"""
    r = len(data)
    out = bytearray([min(r, 15) << 4])
    if r >= 15:
        rest = r - 15
        out += b"\xff" * (rest // 255)
        out.append(rest % 255)
    return bytes(out) + bytes(data)


def cut_is_valid(seq, n, t):
    """(valid, r) of the cut behind the sequence (matchStart, inEnd, outEnd)"""
    match_start, in_end, out_end = seq
    r = min(n - in_end, lit(t - out_end))
    return out_end + 1 <= t and r >= LASTLITERALS and match_start + MFLIMIT <= in_end + r, r


def page(block, src, t):
    """The page of size t for the slice `src` (n = len(src) <= 65536 bytes) whose block is `block`.
    Returns (page bytes, consumed, j): j is the index of the last sequence kept, -1 for the all-literals page, None when the page
    is the whole block; (None, 0, None) for t < 1: no page."""
    src = bytes(src)
    n = len(src)
    if t < 1:
        return None, 0, None
    if len(block) <= t:
        return bytes(block), n, None
    best, best_r, in_end, out_end = -1, min(n, lit(t)), 0, 0
    for j, s in enumerate(iter_sequences(block, n)):
        if s[2] + 1 > t:
            break               # outEnd only grows: no sequence from here on leaves room for a token
        ok, r = cut_is_valid(s, n, t)
        if ok:
            best, best_r, in_end, out_end = j, r, s[1], s[2]
    return bytes(block[:out_end]) + literal_run(src[in_end: in_end + best_r]), in_end + best_r, best


def valid_cuts(block, n, t):
    """[bool] per sequence: the kernel relies on these forming a prefix (an invalid cut has none behind it)"""
    return [cut_is_valid(s, n, t)[0] for s in sequences(block, n)[0]]


def chain(src, t, encode, max_pages=None):
    """The chain of pages of size t over src: encode(slice, pos) gives E for the slice of up to 65536 bytes at pos.  Returns
    [(page, consumed, j, pos, n, cut_by_t)] until the input is consumed, max_pages are written or a page takes nothing."""
    src = bytes(src)
    out = []
    pos = 0
    while max_pages is None or len(out) < max_pages:
        if t < 1:
            break
        n = min(len(src) - pos, 65536)
        if n == 0:
            out.append((b"\x00", 0, None, pos, 0, False))
            break
        e = encode(src[pos: pos + n], pos)
        pg, used, j = page(e, src[pos: pos + n], t)
        out.append((pg, used, j, pos, n, len(e) > t))
        pos += used
        if pos >= len(src) or used == 0:
            break
    return out
