"""The lane-parallel decoder with its window of compressed bytes laid over the top of the output ring, beside the jump table
(decode_par.hpp: PAR_RING 5088, PAR_HIST 1500, PAR_BATCH_OUT 1856; the table is the ring's bytes 4080..5119, the window its bytes
3216..4079, sizeof(ParLds) = 5120 = four LDS granules, so that 28 waves share a CU).

Hand-built blocks; every code and every byte must be the oracle's, and nothing behind a block's bytes may be written (0xA5 guard).
Sequences of 7 compressed bytes (3 literals, a match with one extension byte) come 64 to a batch, the ring slides when its content
(output kept + `dst & 15`) passes 5088 - 1888 = 3200 bytes, and a slide keeps the last 1500..1515 bytes.  Window byte k is ring byte
3216 + k; a batch that starts with 3200 bytes of content and puts out 1856 writes ring bytes 3200..5055: over the window it is
decoded from.

  overwritten   a batch that starts with the content at 3200 - 1, 3200 and 3200 + 1 (which slides first) and puts out 1855 / 1856
                bytes.  Its early sequences carry literal runs of 17, 9, 16, 40 and 270 bytes whose destinations, asserted here,
                lie on the window's ring bytes; the 270-byte run lands on the window bytes that hold the batch's LAST twelve
                sequences (asserted from their window offsets): their tokens, offsets and literals of 1, 8, 9, 16 and 17 bytes
                are read from bytes the same batch writes.  Those twelve are the kinds test_par_overlay_gpu._kinds_batch lists.
  stored        the window of the batch behind one that ends exactly at the no-slide bound (stored without a slide) and one byte
                above it (stored behind the slide): that batch's compressed bytes fill the window as far as a plain sequence can
                reach: a token in every 16-byte slot below byte 496, then a literal run of 33, 49, .. 257 or 269 bytes, whose
                last 16 bytes, offset and extension byte lie in the upper slots 32..48, each in turn
  hand-over     a match with two extension bytes at ring fills around PAR_HIST, the no-slide bound and PAR_RING, then full batches
  history       offsets PAR_HIST - 16 .. PAR_HIST + 48 all through 64 KiB
  occupancy     what the runtime reports: 28 resident waves per CU for the two kernels at seven waves per SIMD
"""
import pytest

from conftest import DECODERS
from test_par_lds_fit_gpu import _B, _run, _place, GAP  # noqa: F401  (_place, GAP: _run's layout)

pytestmark = pytest.mark.gpu

_PAR = [d for d in DECODERS if d in (2, 3)] or [2]
PAR_RING, PAR_HIST, PAR_BATCH_OUT, PAR_WIN = 5088, 1500, 1856, 832
NO_SLIDE = PAR_RING - PAR_BATCH_OUT - 32           # 3200: the most content a batch can start with
JUMP_OFS = (PAR_RING + 32 - 1040) & ~15             # 4080: the table's first byte in the ring
WIN_OFS = JUMP_OFS - (PAR_WIN + 32)                 # 3216: the window's
BASE3 = 1888                                        # ring base behind _prefix's slide

# every layout claim of decode_par.hpp's static_asserts, before anything runs
assert PAR_RING + 32 == 5120 and WIN_OFS % 16 == 0 and JUMP_OFS % 16 == 0
assert WIN_OFS >= (NO_SLIDE + 15) & ~15 and JUMP_OFS + 1040 <= PAR_RING + 32 and 1040 + PAR_WIN + 32 <= PAR_BATCH_OUT + 64
assert PAR_HIST + 30 + PAR_BATCH_OUT + 32 <= PAR_RING


def _batch64(b, total, lo_off=1, hi_off=1400):
    """64 sequences of 7 compressed bytes (3 literals, match of 19 bytes or more: one extension byte) with `total` output bytes"""
    base, rem = divmod(total, 64)
    assert base >= 22 and base + 1 <= 3 + 4 + 15 + 254 and total <= PAR_BATCH_OUT
    for k in range(64):
        n = base + (1 if k < rem else 0)
        off = 2 if b.op == 0 else b.rng.randrange(lo_off, min(b.op + 3, hi_off) + 1)
        b.add(3, off, n - 3)


def _prefix(b, align, delta):
    """Three full batches: 1700 + 1700 bytes (the second ends above 3200: slide, ring base 1888, content 1512 + align), then a
    batch that brings the content to 3200 + delta."""
    _batch64(b, 1700)
    _batch64(b, 1700)
    assert b.op == 3400 and (b.op - PAR_HIST) & ~15 == BASE3
    assert 1700 + align <= NO_SLIDE < 3400 + align
    _batch64(b, NO_SLIDE + delta - (b.op - BASE3) - align)
    assert b.op - BASE3 + align == NO_SLIDE + delta
    assert b.ip == 3 * 64 * 7 and b.ip % 16 == 0


def _own_window_batch(b, total, in_res, ring_of):
    """One batch of `total` output bytes that is decoded from a window it overwrites.  in_res: the data's address mod 16, which is
    the window offset of the batch's first byte (the three batches in front are 1344 = 84 * 16 compressed bytes).  ring_of(op): ring
    index of output position op while this batch is decoded, or None when the batch in front slid (the batch then ends far below
    the window and is only decoded)."""
    start, ip0 = b.op, b.ip
    runs, woff = [], lambda: in_res + (b.ip - ip0)          # window offset of the next sequence's token

    def run(lit, ml):
        d0 = b.op
        b.add(lit, b.rng.randrange(8, 1400), ml)
        runs.append((lit, d0, d0 + lit))

    b.add(0, 700, 23)                    # so that the first run starts above the window's first byte
    run(17, 18)                          # n > 16: first and last 16 bytes from the window
    run(9, 18)
    run(16, 18)                          # 9..16: one 16-byte chunk
    pad = 320 + in_res - (b.op - start) - 40
    assert 19 <= pad <= 273
    run(40, pad)                         # n > 32: the middle from the compressed stream
    assert b.op - start == 320 + in_res
    run(270, 18)                         # the longest plain run; its destination is where the last twelve sequences' window bytes lie
    big = runs[-1]
    special = 6 + 20 + 33 + 49 + 57 + 11 + 4 * 28 + 11 + 18
    rest = total - (b.op - start) - special
    for k in range(4):                   # four matches without literals (4 compressed bytes each) make up the output
        n = rest // 4 + (1 if k < rest % 4 else 0)
        assert 19 <= n <= 273
        b.add(0, b.rng.randrange(300, 1400), n)
    first, kinds = b.op, []

    def kind(lit, off, ml):
        kinds.append((woff(), lit))
        b.add(lit, off, ml)

    def far(lit):
        return b.op + lit - 1000         # source at output position 1000: below every ring base of this block (>= 1888)

    kind(1, 40, 5)                       # 1 literal, 4-byte class (ml < 8, no self-overlap)
    kind(8, 64, 12)                      # 8 literals, 8-byte class
    kind(9, 100, 24)                     # 9 literals, 16-byte class
    kind(16, far(16), 33)                # 16 literals (token 15 + extension byte), far match, 16-byte chunks
    kind(17, 3, 40)                      # 17 literals, self-overlapping match (offset 3)
    kind(2, 9, 9)                        # 8-byte class at its limit (off 9 >= ml 9): copies from the match in front of it
    for _ in range(4):                   # a chain four deep (in-order copy after round two): each match lies in the sequence in front
        kind(3, 30, 25)
    kind(4, far(4), 7)                   # far, 4-byte class
    kind(5, far(5), 13)                  # far, 8-byte class
    assert b.op - first == special and b.op - start == total
    last_token = kinds[-1][0]
    assert last_token <= 511 and woff() <= PAR_WIN - 32          # every token is one of the window's 512 candidates
    assert {1, 8, 9, 16, 17} <= {lit for _, lit in kinds}
    if ring_of is not None:
        for lit, d0, d1 in runs:         # every early literal run is written onto the window's bytes
            assert WIN_OFS <= ring_of(d0) and ring_of(d1) <= WIN_OFS + PAR_WIN, (lit, ring_of(d0), ring_of(d1))
        lo, hi = ring_of(big[1]) - WIN_OFS, ring_of(big[2]) - WIN_OFS       # window bytes the 270-byte run overwrites
        assert lo <= kinds[0][0] and woff() <= hi, (lo, hi, kinds[0][0], woff())   # ... hold the last twelve sequences whole
        assert ring_of(b.op) <= PAR_RING - 32


def _own_window_block(align, delta, total, in_res, seed):
    b = _B(seed)
    _prefix(b, align, delta)
    _own_window_batch(b, total, in_res, (lambda op: op - BASE3 + align) if delta <= 0 else None)
    b.fill(2500)                                         # the block goes on: a slide, further batches
    return b.block()


@pytest.mark.parametrize("decoder", _PAR)
def test_window_overwritten_by_its_own_batch(engine, oracle, decoder):
    items = []
    for align in (0, 1, 15):
        for delta in (-1, 0, 1):
            for total in (PAR_BATCH_OUT - 1, PAR_BATCH_OUT):
                in_res = (align + delta + 1) % 4         # (small: the batch's 514 compressed bytes end below window byte 519)
                blk, n = _own_window_block(align, delta, total, in_res, 8000 + 100 * align + 10 * (delta + 1) + total % 2)
                items.append((blk, n, in_res, align))
    _run(engine, oracle, items, decoder, "window overwritten")


RUNS = tuple(range(33, 258, 16)) + (269,)      # literal runs that end in each of the window's upper 16-byte slots


def _spread_batch(b, run):
    """A batch whose compressed bytes reach far into the window: 60 sequences of 8 bytes (a token in every 16-byte slot below byte
    496 wherever the window starts), then `run` literals and a match with an extension byte.  Of a run above 32 bytes the decoder
    takes the first and the last 16 bytes from the window (the middle comes from the compressed stream in global memory), and the
    offset and the extension byte behind it: with run = 33, 49, .. 257, 269 these lie in window slots 32..48, each in turn (bytes
    480 + 2 + run - 16 .. 480 + 2 + run + 3, plus the window's start of 0..15)."""
    start = b.op
    for _ in range(60):
        b.small(8)
    b.add(run, b.rng.randrange(1, 1400), 19 + b.rng.randrange(0, 100))
    assert b.op - start <= PAR_BATCH_OUT                 # (the run belongs to this batch: its output fits)


def _stored_block(align, delta, run, seed):
    b = _B(seed)
    _prefix(b, align, delta)             # the batch in front ends at or below the no-slide bound (delta <= 0) or slides (delta > 0)
    _spread_batch(b, run)
    _spread_batch(b, RUNS[(RUNS.index(run) + 5) % len(RUNS)])     # ... and once more behind a batch of another size
    b.fill(2500)
    return b.block()


@pytest.mark.parametrize("decoder", _PAR)
def test_window_stored_after_a_slide_and_after_none(engine, oracle, decoder):
    slots = set()
    items = []
    for k, run in enumerate(RUNS):
        for delta in (-1, 0, 1, 2):
            align, in_res = (5 * k + delta) & 15, (3 * k + 7 * delta) & 15
            blk, n = _stored_block(align, delta, run, 8300 + 10 * k + delta)
            items.append((blk, n, in_res, align))
            slots.update(range((in_res + 482 + run - 16) >> 4, ((in_res + 482 + run + 2) >> 4) + 1))   # first spread batch's run end
    assert set(range(32, 48)) <= slots and max(slots) <= 49, sorted(slots)
    _run(engine, oracle, items, decoder, "window stored")


def _handover_block(fill, seed):
    """`fill` bytes of plain sequences, a match of 300 bytes (extension bytes 255, 26: not a plain sequence, so the sequential decoder
    takes it and the ring's history is loaded again, the window fetched again), then two full batches."""
    b = _B(seed)
    b.fill(fill)
    b.add(3, b.rng.randrange(1, min(b.op, 1000) + 1), 300)
    _batch64(b, PAR_BATCH_OUT)
    _batch64(b, PAR_BATCH_OUT - 1)
    b.fill(800)
    return b.block()


@pytest.mark.parametrize("decoder", _PAR)
def test_batch_after_hand_over(engine, oracle, decoder):
    fills = (200, PAR_HIST - 40, PAR_HIST + 20, NO_SLIDE - 310, NO_SLIDE + 40, PAR_RING, 9000)
    items = [(blk, n, (7 * k + a) & 15, a) for k, f in enumerate(fills) for a in (0, 9, 15)
             for blk, n in [_handover_block(f, 8400 + 16 * k + a)]]
    _run(engine, oracle, items, decoder, "hand-over")


def _hist_block(align, seed):
    """64 KiB whose matches all reach back PAR_HIST - 16 .. PAR_HIST + 48 bytes: right after a slide these sources lie just inside the
    ring, across its base, and just below it."""
    b = _B(seed)
    b.fill(PAR_HIST + 100)
    k = 0
    while b.op < 65536 - 64:
        lit = b.rng.randrange(0, 9)
        b.add(lit, PAR_HIST - 16 + (37 * k + 7 * align) % 65, b.rng.choice((4, 5, 7, 8, 12, 15, 16, 17, 24, 31, 32, 33, 40)))
        k += 1
    return b.block()


@pytest.mark.parametrize("decoder", _PAR)
def test_history_kept_by_a_slide(engine, oracle, decoder):
    items = [(blk, n, (11 * a) & 15, a) for a in range(16) for blk, n in [_hist_block(a, 8600 + a)]]
    assert all(n > 3 * PAR_RING for _, n, _, _ in items)
    _run(engine, oracle, items, decoder, "history")


def test_twenty_eight_waves_per_cu(engine):
    """Four 1280-byte granules of LDS and 72 registers: seven waves per SIMD for the two kernels that decode whole independent
    blocks; the other users of ParLds keep five."""
    for k in ("k_decode_par", "k_decode_par_redo"):
        info = engine.kernel_info(k)
        assert info["lds_bytes"] <= 5120 and info["lds_bytes"] == info["par_lds_bytes"], (k, info)
        assert info["resident_per_cu"] >= 28, (k, info)
    for k in ("k_decode_dict", "k_decode_par_partial"):
        info = engine.kernel_info(k)
        assert info["lds_bytes"] <= 5120 and info["resident_per_cu"] >= 20, (k, info)
