"""The contract of the fast fixed-size output pages against a prepared dictionary (mi355lz4_compress_pages_fastdict_device,
include/mi355lz4.h) in plain Python: what a page holds, given the block E that the engine writes for the slice with
the dictionary in front of it, the slice's length n and the page size T.

    E = s_0 .. s_{m-1} (literals, offset, match) and a last literal run.
    |E| <= T: the page is E and consumes n.
    Otherwise the page is s_0 .. s_j of E, byte for byte, and one literal run of r_j = min(n - inEnd_j, lit(T - outEnd_j)) bytes.
    A cut behind s_j is valid when outEnd_j + 1 <= T, r_j >= 5, matchStart_j + 12 <= inEnd_j + r_j and inEnd_j + r_j >= 13.
    j + 1 is the number of LEADING sequences whose cuts are all valid; j = -1 is the all-literals page.

Two points differ from tests/fastpages_model.py (7m), whose helpers are used as they are: the fourth condition -- with a dictionary a
block's first sequence can be a match at position 0, and a block of fewer than 13 bytes must be literals only -- and the leading
run, because with the fourth condition valid cuts no longer form a prefix.  Positions are the slice's own: the dictionary does not
count.

Test infrastructure only.
"""
from fastpages_model import cut_is_valid as cut_is_valid_7m
from fastpages_model import ext, iter_sequences, lit, literal_run, min_progress, sequences  # noqa: F401  (re-exported)
from lz4_check import MIN_LENGTH


def cut_is_valid(seq, n, t):
    """(valid, r) of the cut behind the sequence (matchStart, inEnd, outEnd): 7m's three conditions and the 13 bytes"""
    ok, r = cut_is_valid_7m(seq, n, t)
    return ok and seq[1] + r >= MIN_LENGTH, r


def valid_cuts(block, n, t):
    """[bool] per sequence; NOT a prefix in general (tests/test_dictpages_host.py has the counter-example)"""
    return [cut_is_valid(s, n, t)[0] for s in sequences(block, n)[0]]


def page(block, src, t):
    """The page of size t for the slice `src` (n = len(src) <= 65536 bytes) whose block against the dictionary is `block`.
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
        ok, r = cut_is_valid(s, n, t)
        if not ok:
            break               # the leading run ends at the first sequence without a valid cut
        best, best_r, in_end, out_end = j, r, s[1], s[2]
    return bytes(block[:out_end]) + literal_run(src[in_end: in_end + best_r]), in_end + best_r, best


def page_last_valid(block, src, t):
    """the same with 7m's choice -- the LAST sequence with a valid cut -- under the four conditions: what the rule is not (the
    tests show page sizes at which the two differ)"""
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


def chain(src, t, encode, max_pages=None):
    """The chain of pages of size t over src: encode(slice, pos) gives E for the slice of up to 65536 bytes at pos, with the
    dictionary in front of it.  Returns [(page, consumed, j, pos, n, cut_by_t)] until the input is consumed, max_pages are written
    or a page takes nothing."""
    src = bytes(src)
    out = []
    pos = 0
    while max_pages is None or len(out) < max_pages:
        if t < 1:
            break
        n = min(len(src) - pos, 65536)
        if n == 0 or t == 1:
            out.append((b"\x00", 0, None, pos, n, n > 0))
            break
        e = encode(src[pos: pos + n], pos)
        pg, used, j = page(e, src[pos: pos + n], t)
        out.append((pg, used, j, pos, n, len(e) > t))
        pos += used
        if pos >= len(src) or used == 0:
            break
    return out
