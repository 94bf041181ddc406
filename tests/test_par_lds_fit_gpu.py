"""The lane-parallel decoder at the limits its LDS footprint sets (decode_par.hpp: PAR_WIN 832, PAR_BATCH_OUT 2048, PAR_RING 5728,
PAR_HIST 2000; sizeof(ParLds) = 7664 <= 7680 = six LDS granules of 1280 bytes, so that 20 waves share a CU).

Hand-built blocks, placed so that the data's address mod 16 (where the window starts) and the output's (`dst & 15`, the ring's
alignment head) are chosen by the test; every code and every byte must be the oracle's.

  window    the latest a plain sequence can end in the 832-byte window: a token at window byte 509, 510, 511 (and 512, which is
            no candidate any more) with 15 + 254 literals and a match-length extension byte -- it ends at byte 785
  batch     full batches of 64 sequences of 33..40 output bytes (41 and 32 too at the two ends) that cross the cap of 2048 output
            bytes at each of lanes 50..63, the sequences behind the cut copying from the cut part
  ring      offsets 1984..2048 -- at and past the history a slide keeps -- all through 64 KiB blocks (a slide every 1.6 to 3.6 KB),
            at all 16 values of dst & 15
  occupancy the runtime's resident workgroups per CU and static LDS of k_decode_par<false>
"""
import random

import numpy as np
import pytest

import lz4_synth as S
from conftest import DECODERS

pytestmark = pytest.mark.gpu

# the lane-parallel decoder: variant 2 (and 3, its list-driven form, in the experiment build's run)
_PAR = [d for d in DECODERS if d in (2, 3)] or [2]
PAR_BATCH_OUT = 2048
GAP = 64


def _place(base, pos, residue):
    """the first position >= pos whose address base + position is `residue` mod 16"""
    return pos + ((residue - (base + pos)) & 15)


def _run(engine, oracle, items, decoder, what):
    """items: [(block, cap, data address mod 16, output address mod 16)] as one decompress_batch_device call with 8-byte
    headers; asserts the oracle's code and bytes for every block and that nothing behind a block's bytes was written"""
    import torch
    n = len(items)
    inp = torch.zeros(sum(len(b) + 8 + 16 + GAP for b, _, _, _ in items) + 64, dtype=torch.uint8, device="cuda:0")
    out = torch.full((sum(c + 16 + GAP for _, c, _, _ in items) + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    host = np.zeros(inp.numel(), dtype=np.uint8)
    boff, ooff, ip, op = [], [], 0, 0
    for blk, cap, ir, orr in items:
        p = _place(inp.data_ptr() + 8, ip, ir)
        host[p:p + 8] = np.frombuffer(len(blk).to_bytes(4, "little") + int(cap).to_bytes(4, "little"), np.uint8)
        host[p + 8:p + 8 + len(blk)] = np.frombuffer(blk, np.uint8)
        boff.append(p)
        ip = p + 8 + len(blk) + GAP
        q = _place(out.data_ptr(), op, orr)
        ooff.append(q)
        op = q + cap + GAP
    inp.copy_(torch.from_numpy(host))
    boff_t = torch.tensor(boff + [ip], dtype=torch.int64, device="cuda:0")
    ooff_t = torch.tensor(ooff + [op], dtype=torch.int64, device="cuda:0")
    res = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    engine.set_decoder(decoder)
    try:
        engine.decompress_batch_device(inp, inp.numel(), boff_t, n, out, ooff_t, res)
        engine.synchronize()
    finally:
        engine.set_decoder(0)
    got, codes = out.cpu().numpy(), res.cpu().tolist()
    for i, (blk, cap, ir, orr) in enumerate(items):
        code, dec = oracle.decompress_block(blk, cap)
        assert codes[i] == code, (what, i, ir, orr, codes[i], code)
        assert code > 0, (what, i, "the block was written to be valid", code)
        g = got[ooff[i]:ooff[i] + code]
        e = np.frombuffer(dec, np.uint8)
        assert np.array_equal(g, e), (what, i, ir, orr, "bytes differ at", int(np.argmax(g != e)))
        assert (got[ooff[i] + code:ooff[i] + cap + GAP] == 0xA5).all(), (what, i, "bytes behind the block were written")


class _B:
    """sequences of one block with the running positions"""

    def __init__(self, seed):
        self.rng, self.seqs, self.ip, self.op = random.Random(seed), [], 0, 0

    def add(self, lit, off, ml):
        lits = bytes(self.rng.randrange(256) for _ in range(lit))
        assert 1 <= off <= self.op + lit
        self.seqs.append((lits, off, ml))
        self.ip += S.seq_size(lit, ml)
        self.op += lit + ml

    def small(self, size, lit=None):
        """a plain sequence of `size` compressed bytes (3 + literals, no extension byte)"""
        lit = size - 3 if lit is None else lit
        assert 0 < lit < 15
        self.add(lit, self.rng.randrange(1, self.op + lit + 1), self.rng.randrange(4, 19))

    def fill(self, nbytes):
        """plain short sequences until `nbytes` more output bytes exist"""
        end = self.op + nbytes
        while self.op < end:
            lit = self.rng.randrange(1, 9)
            self.add(lit, self.rng.randrange(1, min(self.op + lit, 1500) + 1), self.rng.randrange(4, 40))

    def block(self):
        last = bytes(self.rng.randrange(256) for _ in range(12))
        return S.write_block(self.seqs, last), self.op + len(last)


# ---- window -------------------------------------------------------------------------------------------------------------------------

def _window_block(target, in_res, seed):
    """The block's data lies at an address that is in_res mod 16, so its first window starts in_res bytes in front of it and
    the first batch's token k lies at window byte in_res + (compressed bytes in front of it).  Under 64 sequences of 8..17
    bytes bring a token to window byte `target`; that sequence has 15 + 254 literals and a match of 19 + e bytes (one extension
    byte each way): token, extension, 269 literals, offset, extension = 274 bytes, ending at target + 274."""
    b = _B(seed)
    rem = target - in_res
    while rem >= 18:
        b.small(10)
        rem -= 10
    b.small(rem)
    assert b.ip == target - in_res and len(b.seqs) < 60
    b.add(269, b.rng.randrange(1, b.op + 1), 19 + b.rng.randrange(0, 255))
    assert b.ip == target - in_res + 274
    b.fill(1200)                                     # the block goes on: the sequence is far from both of its ends
    return b.block()


@pytest.mark.parametrize("decoder", _PAR)
def test_window_boundary(engine, oracle, decoder):
    """Tokens at window bytes 509, 510, 511 and 512 whose sequences end at bytes 783..786 of the 832-byte window, with the
    window starting 0..15 bytes in front of the block."""
    items = []
    for target in (509, 510, 511, 512):
        for in_res in range(16):
            blk, n = _window_block(target, in_res, 1000 * target + in_res)
            items.append((blk, n, in_res, (in_res * 7 + target) & 15))
    _run(engine, oracle, items, decoder, "window")


# ---- batch cap ----------------------------------------------------------------------------------------------------------------------

def _cut_lens(lane):
    """64 output lengths of 33..40 bytes of which the first `lane` sum to at most PAR_BATCH_OUT and the first lane + 1 to
    more: the batch is cut in front of lane `lane`.  (Lane 50 needs 41 too -- 51 sequences of 40 bytes are 2040 -- and lane 63
    needs 32: 63 sequences of 33 bytes are 2079.)"""
    for s in range(40, 31, -1):
        for a in range(lane + 1):                    # a sequences of s + 1 bytes in front, the others s
            if lane * s + a <= PAR_BATCH_OUT < lane * s + a + s:
                lens = [s + 1] * a + [s] * (64 - a)
                assert sum(lens[:lane]) <= PAR_BATCH_OUT < sum(lens[:lane + 1])
                return lens
    raise AssertionError(lane)


def _batch_block(lane, seed):
    """First batch: 64 sequences of 7 compressed bytes (3 literals, a match with an extension byte), cut by the output cap in
    front of lane `lane`.  Every sequence from the cut on copies from the sequence in front of it or the one before that: the
    sources of the second batch's first matches lie in the part the first batch left behind, and chain."""
    b = _B(seed)
    for k, n in enumerate(_cut_lens(lane)):
        if k == 0:
            b.add(3, 2, n - 3)
        elif k < lane:
            b.add(3, b.rng.randrange(1, b.op + 3 + 1), n - 3)
        else:
            b.add(3, b.rng.randrange(20, 75), n - 3)
    assert b.ip == 64 * 7                            # all 64 tokens lie below window byte 512 - 49
    for _ in range(40):                              # ... and the chain goes on through the next batch
        b.add(3, b.rng.randrange(20, 75), b.rng.randrange(30, 38))
    b.fill(600)
    return b.block()


def _steady_block(seed):
    """64 KiB of sequences of 33..40 output bytes and 7 compressed bytes: every batch is full and is cut by the output cap,
    wherever the batch in front of it was cut"""
    b = _B(seed)
    b.add(3, 2, 33)
    while b.op < 65536 - 64:
        b.add(3, b.rng.randrange(1, min(b.op, 4000) + 1), b.rng.randrange(30, 38))
    return b.block()


@pytest.mark.parametrize("decoder", _PAR)
def test_batch_cap(engine, oracle, decoder):
    items = [(blk, n, lane & 15, (5 * lane) & 15) for lane in range(50, 64) for blk, n in [_batch_block(lane, lane)]]
    items += [(blk, n, 3 * k, 5 * k + 1) for k in range(4) for blk, n in [_steady_block(70 + k)]]
    _run(engine, oracle, items, decoder, "batch cap")


# ---- ring base and history ----------------------------------------------------------------------------------------------------------

def _ring_block(align, seed):
    """64 KiB whose matches all reach back 1984..2048 bytes: a slide keeps the last 2000..2015 bytes in the ring, so right
    after one these sources lie just inside the ring, across its base, and just below it (in global memory, flushed or not).
    Sequence k takes offset 1984 + (37 k + 7 align) mod 65: every offset turns up behind the slides of the 16 blocks."""
    b = _B(seed)
    b.fill(2100)
    k = 0
    while b.op < 65536 - 64:
        lit = b.rng.randrange(0, 9)
        b.add(lit, 1984 + (37 * k + 7 * align) % 65, b.rng.choice((4, 5, 7, 8, 12, 15, 16, 17, 24, 31, 32, 33, 40)))
        k += 1
    return b.block()


@pytest.mark.parametrize("decoder", _PAR)
def test_ring_base_and_history(engine, oracle, decoder):
    items = [(blk, n, (11 * a) & 15, a) for a in range(16) for blk, n in [_ring_block(a, 300 + a)]]
    assert all(n > 3 * 5728 for _, n, _, _ in items)         # (many slides: the ring holds 5728 bytes)
    _run(engine, oracle, items, decoder, "ring")


# ---- occupancy ----------------------------------------------------------------------------------------------------------------------

def test_twenty_waves_per_cu(engine):
    """The point of the footprint: at most six 1280-byte granules of LDS per wave, so that the registers (5 waves per SIMD),
    not the LDS, bound the waves of a CU."""
    for k in ("k_decode_par", "k_decode_par_redo", "k_decode_dict", "k_decode_par_partial"):
        info = engine.kernel_info(k)
        assert info["lds_bytes"] <= 7680 and info["lds_bytes"] == info["par_lds_bytes"], (k, info)
        assert info["resident_per_cu"] >= 20, (k, info)
