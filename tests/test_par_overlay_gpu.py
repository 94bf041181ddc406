"""The lane-parallel decoder with its jump table laid over the top of the output ring (decode_par.hpp: PAR_RING 5504, PAR_HIST 1776,
PAR_BATCH_OUT 2048; the table and the rank records are the ring's bytes 4496..5535, sizeof(ParLds) = 6400 = five LDS granules, so that
24 waves share a CU).

Hand-built blocks; every code and every byte must be the oracle's, and nothing behind a block's bytes may be written (0xA5 guard).
The blocks are built from what the decoder does with them: sequences of 7 compressed bytes (3 literals, a match with one extension
byte) come 64 to a batch, the ring slides when its content (output kept + `dst & 15`) passes 5504 - 2080 = 3424 bytes, and a slide
keeps the last 1776..1791 bytes.

  overwritten   a batch that starts with the ring's content at 3424 - 1, 3424 (the most a batch can start with) and 3424 + 1 (which
                slides first) and puts out 2047 / 2048 bytes (the most a batch can): its output runs over the dead table up to ring
                byte 5472, the highest a batch's output reaches (content + output <= PAR_RING - 32; PAR_RING itself cannot be
                reached, the slide rule keeps 32 bytes clear).  The batch's last 317 bytes -- ring bytes 5155..5472, asserted here to lie
                at or above the table's first byte, 4496 -- are literals of 1, 8, 9, 16, 17 bytes, near matches of the 4-, 8- and
                16-byte classes, far matches of all three chunk sizes, a self-overlapping match and a chain four deep (in-order copy
                after round two).  (From 3424 + 1 the ring slides first and the same batch ends below the table.)
  not yet dead  the same start, content 3424: the table's lowest byte is then as close to live history as it gets.  The batch's
                first matches read the last 32 bytes of that history and depend on each other four deep.
  history       offsets PAR_HIST - 16 .. PAR_HIST + 48 all through 64 KiB
  hand-over     a match with two extension bytes (the sequential decoder takes it, the ring is reloaded) at several ring fills,
                then full batches
  window edge   the first block at byte 0 of the framed buffer (its first window's bytes are checked through the output) and the last
                block ending 0..15 bytes before its end (the slot across the end holds only bytes of the block's last 31, which no batch
                parses: that side is run for the loads it issues, not for its data)
  occupancy     what the runtime reports for the two kernels that run six waves per SIMD, and for the others
"""
import numpy as np
import pytest

import lz4_synth as S
from conftest import DECODERS
from test_par_lds_fit_gpu import _B, _run, _place, GAP

pytestmark = pytest.mark.gpu

_PAR = [d for d in DECODERS if d in (2, 3)] or [2]
PAR_RING, PAR_HIST, PAR_BATCH_OUT = 5504, 1776, 2048
NO_SLIDE = PAR_RING - PAR_BATCH_OUT - 32          # 3424: the most content a batch can start with
JUMP_OFS = (PAR_RING + 32 - 1040) & ~15            # 4496: the table's first byte in the ring


def _batch64(b, total, lo_off=1, hi_off=1500):
    """64 sequences of 7 compressed bytes (3 literals, match of 19 bytes or more: one extension byte) with `total` output bytes"""
    base, rem = divmod(total, 64)
    assert base >= 22 and base + 1 <= 3 + 4 + 15 + 254
    for k in range(64):
        n = base + (1 if k < rem else 0)
        off = 2 if b.op == 0 else b.rng.randrange(lo_off, min(b.op + 3, hi_off) + 1)
        b.add(3, off, n - 3)


def _prefix(b, align, delta):
    """Three full batches: 1800 + 1800 bytes (the second ends above 3424: slide, ring base 1824, content 1776 + align), then a
    batch that brings the content to 3424 + delta."""
    _batch64(b, 1800)
    _batch64(b, 1800)
    assert b.op == 3600 and (b.op - PAR_HIST) & ~15 == 1824
    _batch64(b, NO_SLIDE + delta - (b.op - 1824) - align)
    assert b.op - 1824 + align == NO_SLIDE + delta
    assert b.ip == 3 * 64 * 7


def _kinds_batch(b, total, ring_of=None):
    """One batch of `total` output bytes: 52 plain sequences, then a sequence of every kind the copy phases tell apart, so that
    these are the batch's last 317 bytes.  ring_of(op) is the ring index of output position op while this batch is decoded (None: the
    batch in front slid, and the batch does not reach the table): every special sequence must then lie on the table's bytes."""
    start = b.op
    special = 6 + 20 + 33 + 49 + 57 + 11 + 4 * 28 + 11 + 18
    n = 64 - 12
    base, rem = divmod(total - special, n)
    assert base >= 22
    for k in range(n):
        b.add(3, b.rng.randrange(8, 1500), base + (1 if k < rem else 0) - 3)
    first = b.op

    def far(lit):
        return b.op + lit - 1000                        # source at output position 1000: below every ring base of this block (>= 1824)

    b.add(1, 40, 5)                      # 1 literal, 4-byte class (ml < 8, no self-overlap)
    b.add(8, 64, 12)                     # 8 literals, 8-byte class
    b.add(9, 100, 24)                    # 9 literals, 16-byte class
    b.add(16, far(16), 33)               # 16 literals (token 15 + extension byte), far match, 16-byte chunks
    b.add(17, 3, 40)                     # 17 literals, self-overlapping match (offset 3)
    b.add(2, 9, 9)                       # 8-byte class at its limit (off 9 >= ml 9): copies from the match in front of it
    for _ in range(4):                   # a chain four deep (in-order copy after round two): each match lies in the sequence in front
        b.add(3, 30, 25)
    b.add(4, far(4), 7)                  # far, 4-byte class
    b.add(5, far(5), 13)                 # far, 8-byte class
    assert b.op - first == special and b.op - start == total and len(b.seqs) % 64 == 0
    assert b.ip - 3 * 64 * 7 - 8 + 15 < 512              # all 64 tokens lie among the window's 512 candidates, wherever it starts
    if ring_of is not None:
        assert ring_of(first) >= JUMP_OFS and ring_of(b.op) <= PAR_RING - 32, (ring_of(first), ring_of(b.op))


def _deep_batch(b):
    """The first matches read the last 32 bytes in front of the batch and chain four deep; 2048 bytes in all."""
    start = b.op
    b.add(3, 3 + 32, 29)                 # source: the 32 bytes in front of the batch
    b.add(3, 3 + 20, 20)                 # ... in sequence 0's match
    b.add(3, 3 + 15, 19)                 # ... in sequence 1's
    b.add(3, 3 + 12, 19)                 # ... in sequence 2's
    b.add(3, 3 + 60, 30)                 # across sequences 0..3
    n = 64 - 5
    rest = PAR_BATCH_OUT - (b.op - start)
    base, rem = divmod(rest, n)
    for k in range(n):
        b.add(3, b.rng.randrange(1, 70), base + (1 if k < rem else 0) - 3)
    assert b.op - start == PAR_BATCH_OUT


def _overlay_block(align, delta, total, seed, deep=False):
    b = _B(seed)
    _prefix(b, align, delta)
    if deep:
        _deep_batch(b)
    else:
        # (content 3424 + 1 in front of the batch: the ring slides first, and the batch ends far below the table)
        _kinds_batch(b, total, (lambda op: op - 1824 + align) if delta <= 0 else None)
    b.fill(2500)                                         # the block goes on: a slide, further batches
    return b.block()


@pytest.mark.parametrize("decoder", _PAR)
def test_overlay_overwritten(engine, oracle, decoder):
    items = []
    for align in (0, 1, 15):
        for delta in (-1, 0, 1):
            for total in (PAR_BATCH_OUT - 1, PAR_BATCH_OUT):
                blk, n = _overlay_block(align, delta, total, 7000 + 100 * align + 10 * (delta + 1) + total % 2)
                items.append((blk, n, (3 * align + delta) & 15, align))
    _run(engine, oracle, items, decoder, "overlay overwritten")


@pytest.mark.parametrize("decoder", _PAR)
def test_overlay_not_yet_dead(engine, oracle, decoder):
    items = [(blk, n, (5 * a + 2) & 15, a) for a in range(16) for blk, n in [_overlay_block(a, 0, 0, 7500 + a, deep=True)]]
    _run(engine, oracle, items, decoder, "overlay not yet dead")


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
    items = [(blk, n, (11 * a) & 15, a) for a in range(16) for blk, n in [_hist_block(a, 7600 + a)]]
    assert all(n > 3 * PAR_RING for _, n, _, _ in items)
    _run(engine, oracle, items, decoder, "history")


def _handover_block(fill, align, seed):
    """`fill` bytes of plain sequences, a match of 300 bytes (extension bytes 255, 26: not a plain sequence, so the sequential decoder
    takes it and the ring's history is loaded again), then two full batches parsed into the table."""
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
             for blk, n in [_handover_block(f, a, 7700 + 16 * k + a)]]
    _run(engine, oracle, items, decoder, "hand-over")


def _run_edges(engine, oracle, blocks, shift, tail, decoder):
    """`blocks` as one call whose framed buffer starts `shift` bytes into an allocation, with its first block's header at byte 0
    and exactly `tail` bytes behind its last block."""
    import torch
    whole = torch.zeros(sum(len(b) + 8 + GAP for b, _ in blocks) + 64, dtype=torch.uint8, device="cuda:0")
    inp = whole[shift:]
    out = torch.full((sum(c + GAP for _, c in blocks) + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    boff, ooff, ip, op = [], [], 0, 0
    host = np.zeros(inp.numel(), dtype=np.uint8)
    for i, (blk, cap) in enumerate(blocks):
        host[ip:ip + 8] = np.frombuffer(len(blk).to_bytes(4, "little") + int(cap).to_bytes(4, "little"), np.uint8)
        host[ip + 8:ip + 8 + len(blk)] = np.frombuffer(blk, np.uint8)
        boff.append(ip)
        ip += 8 + len(blk) + (GAP if i + 1 < len(blocks) else 0)
        ooff.append(op)
        op += cap + GAP
    framed_len = ip + tail
    host[ip:] = 0xEE                                     # what lies behind the buffer's end is not the decoder's to read as data
    inp.copy_(torch.from_numpy(host))
    n = len(blocks)
    boff_t = torch.tensor(boff + [framed_len], dtype=torch.int64, device="cuda:0")
    ooff_t = torch.tensor(ooff + [op], dtype=torch.int64, device="cuda:0")
    res = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    engine.set_decoder(decoder)
    try:
        engine.decompress_batch_device(inp, framed_len, boff_t, n, out, ooff_t, res)
        engine.synchronize()
    finally:
        engine.set_decoder(0)
    got, codes = out.cpu().numpy(), res.cpu().tolist()
    for i, (blk, cap) in enumerate(blocks):
        code, dec = oracle.decompress_block(blk, cap)
        assert code > 0 and codes[i] == code, ("edge", shift, tail, i, codes[i], code)
        g, e = got[ooff[i]:ooff[i] + code], np.frombuffer(dec, np.uint8)
        assert np.array_equal(g, e), ("edge", shift, tail, i, "bytes differ at", int(np.argmax(g != e)))
        assert (got[ooff[i] + code:ooff[i] + cap + GAP] == 0xA5).all(), ("edge", shift, tail, i, "bytes behind the block were written")


@pytest.fixture(scope="module")
def edge_blocks():
    out = []
    for seed in (7800, 7801, 7802):
        b = _B(seed)
        b.fill(3000)
        out.append(b.block())
    return out


@pytest.mark.parametrize("decoder", _PAR)
def test_window_crosses_the_buffer_ends(engine, oracle, edge_blocks, decoder):
    """The first block's first window starts in front of the framed buffer (its data lies 8 bytes behind the buffer's start, whose
    address takes all 16 residues): wrong bytes from that slot give wrong output.  The last block's last windows -- 832 bytes from
    16-byte boundaries -- end behind the buffer, which ends 0..15 bytes behind the block; the slot across the end holds bytes of the
    block's last 31 only, which the batch loop never parses, so that side shows faults and stray writes, not wrong data."""
    for shift in range(16):
        _run_edges(engine, oracle, edge_blocks, shift, (5 * shift + 3) & 15, decoder)
    for tail in (0, 15):
        _run_edges(engine, oracle, edge_blocks[:1], 0, tail, decoder)


def test_twenty_four_waves_per_cu(engine):
    """Five 1280-byte granules of LDS and 80 registers: six waves per SIMD for the two kernels that decode whole independent blocks;
    the other users of ParLds keep five."""
    for k in ("k_decode_par", "k_decode_par_redo"):
        info = engine.kernel_info(k)
        assert info["lds_bytes"] <= 6400 and info["lds_bytes"] == info["par_lds_bytes"], (k, info)
        assert info["resident_per_cu"] >= 24, (k, info)
    for k in ("k_decode_dict", "k_decode_par_partial"):
        info = engine.kernel_info(k)
        assert info["lds_bytes"] <= 6400 and info["resident_per_cu"] >= 20, (k, info)
