"""k_decode_par and k_decode_par_redo at EIGHT waves per SIMD: 32 waves per CU, all a CU holds, each with 5120 bytes of LDS -- all of the
CU's 160 KiB -- and 64 registers (decode_par.hpp: PAR_WAVES_MAIN 8; every phase of a batch takes the lane id afresh, `lnow`).

  occupancy   what the runtime reports for the two kernels (32 resident waves, 5120 bytes) and for two that keep five waves per SIMD
  no LDS to spare   a call of 2 x 32 x (CU count) blocks, every slot taken twice: up to 28 waves the byte behind a wave's ring was
              nobody's, now it is another wave's.  Block k is 8 KiB + k % 97 bytes of the engine's generator, half lzsynth and half
              text, decoded to `dst & 15` = k & 15 with guard bytes between the outputs; decoder 2, then decoder 4 forced
  phases      hand-built blocks whose batches are laid out by a model of the decoder (_M: 64 sequences to a batch, the slide rule,
              the reload behind a hand-over), compared with the oracle byte for byte and code for code at all sixteen `dst & 15`:
              far matches of every length class whose sources end 1 and 17 bytes in front of the ring's base and 40 000 bytes back,
              each class alone in a batch and all of them mixed; literal runs of every length class as the first, a middle and the
              last sequence of a full batch; a hand-over right behind a batch with far matches and a long literal run.
              The tested part of a block is 12-20 KiB of output (more than three ring lengths: the ring slides); the blocks of the
              40 000-byte class carry a 40 KiB match in front of it, which the sequential decoder takes.
              A run of 270 literals needs two extension bytes, so it is a sequence the batch loop hands over where it stands; 269,
              the longest run the loop takes itself, is tested beside it.
"""
import functools

import pytest

from conftest import DECODERS
from test_par_lds_fit_gpu import _B, _run, _place, GAP  # noqa: F401  (_place, GAP: _run's layout)

pytestmark = pytest.mark.gpu

_PAR = [d for d in DECODERS if d in (2, 3)] or [2]
PAR_RING, PAR_HIST, PAR_BATCH_OUT = 5088, 1500, 1856
FAR_ML = (4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 270)
LITS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48, 269, 270)
PAD_OUT = 4 + 18                                   # the most a padding sequence puts out


# ---- occupancy ----------------------------------------------------------------------------------------------------------------------

def test_thirty_two_waves_per_cu(engine):
    for k in ("k_decode_par", "k_decode_par_redo"):
        info = engine.kernel_info(k)
        assert info["resident_per_cu"] >= 32, (k, info)
        assert info["lds_bytes"] == info["par_lds_bytes"] == 5120, (k, info)
    for k in ("k_decode_dict", "k_decode_par_partial"):
        info = engine.kernel_info(k)
        assert info["resident_per_cu"] >= 20, (k, info)


# ---- a CU with no LDS to spare --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def full_call(engine, slz4):
    """the blocks, compressed once: (n, row length, source rows, lengths, dense stream, its offsets and size)"""
    import torch
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, W = 2 * 32 * cus, 8192 + 96
    half = n // 2
    src = torch.empty(n * W, dtype=torch.uint8, device=dev)
    engine.generate("lzsynth", src[:half * W], W, half)
    engine.generate("text", src[half * W:], W, n - half, first_block=half)
    lens = (8192 + torch.arange(n, device=dev) % 97).to(torch.int32)
    stride = slz4.slot_stride(W, 8)
    slots = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    flen = torch.empty(n, dtype=torch.int32, device=dev)
    dense = torch.empty(n * stride, dtype=torch.uint8, device=dev)
    doff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    engine.compress_batch_device(src, n, W, slots, stride, flen, src_off=torch.arange(n, dtype=torch.int64, device=dev) * W,
                                 src_len=lens, block_stride=0)
    engine.compact_device(slots, stride, flen, n, dense, n * stride, doff)
    engine.synchronize()
    rows = src.view(n, W)
    # every block is different: a 64-bit hash of each row's first 8192 bytes (every block has those)
    mult = torch.randint(1, 2 ** 62, (1024,), dtype=torch.int64, device=dev, generator=torch.Generator(device=dev).manual_seed(7)) | 1
    h = (rows[:, :8192].contiguous().view(torch.int64).view(n, 1024) * mult).sum(1)
    assert torch.unique(h).numel() == n, "the generator repeated a block"
    del slots
    return n, W, rows, lens, dense, doff, int(doff[-1].item())


@pytest.mark.parametrize("decoder", (2, 4))
def test_every_wave_slot_taken_twice(engine, full_call, decoder):
    import torch
    n, W, rows, lens, dense, doff, cbytes = full_call
    dev = rows.device
    P = (W + 64 + 15 + 15) & ~15                                  # pitch of the outputs: the longest block, its guard, its shift
    out = torch.full((n * P + 64,), 0xA5, dtype=torch.uint8, device=dev)
    k = torch.arange(n, dtype=torch.int64, device=dev)
    shift = (k - out.data_ptr()) & 15                             # dst & 15 == k & 15
    ooff = torch.cat([k * P + shift, torch.tensor([n * P], dtype=torch.int64, device=dev)])
    assert int(((out.data_ptr() + ooff[:n]) & 15).ne(k & 15).sum().item()) == 0
    assert int((ooff[1:n] - ooff[:n - 1] - lens[:n - 1]).min().item()) >= 64
    res = torch.zeros(n, dtype=torch.int32, device=dev)
    engine.set_decoder(decoder)
    try:
        engine.decompress_batch_device(dense, cbytes, doff, n, out, ooff, res)
        engine.synchronize()
    finally:
        engine.set_decoder(0)
    assert torch.equal(res, lens), ("results", (res != lens).nonzero()[:8].flatten().tolist())
    got = out[:n * P].view(n, P)
    for lo in range(0, n, 4096):                                  # expected rows: the guard value, the block at its shift
        hi = min(lo + 4096, n)
        idx = torch.arange(P, dtype=torch.int64, device=dev)[None, :] - shift[lo:hi, None]
        inside = (idx >= 0) & (idx < lens[lo:hi, None])
        exp = torch.where(inside, rows[lo:hi].gather(1, idx.clamp(0, W - 1)), torch.full_like(idx, 0xA5, dtype=torch.uint8))
        bad = (got[lo:hi] != exp)
        if bool(bad.any().item()):
            r, c = [int(v) for v in bad.nonzero()[0]]
            where = "block's bytes" if bool(inside[r, c].item()) else "guard bytes"
            raise AssertionError("decoder %d, block %d (dst & 15 = %d): %s differ at output byte %d"
                                 % (decoder, lo + r, (lo + r) & 15, where, c - int(shift[lo + r].item())))
    assert int((out[n * P:] != 0xA5).sum().item()) == 0


# ---- the decoder's batches and ring, modelled ---------------------------------------------------------------------------------------

class _M(_B):
    """_B that lays its sequences out in the decoder's batches and follows the ring's base.  Every batch is 64 sequences (or fewer,
    closed by a sequence the loop hands over) whose tokens lie among the window's candidates wherever the window starts
    (0..15 bytes in front of the batch), whose output fits PAR_BATCH_OUT, and whose compressed size keeps the next batch at eight
    candidates per lane (more than 6.5 bytes per sequence, decode_par.hpp PAR_ADAPT6).  If the decoder cut its batches elsewhere,
    the comparison with the oracle would hold all the same; only the edges the blocks aim at would be missed."""

    def __init__(self, seed, align):
        super().__init__(seed)
        self.A, self.rb, self.n, self.b_ip, self.b_op = align, 0, 0, 0, 0

    def _new_batch(self):
        self.n, self.b_ip, self.b_op = 0, self.ip, self.op

    def seq(self, lit, off, ml):
        assert lit <= 269 and 4 <= ml <= 273, "a plain sequence: one extension byte at most each way"
        assert self.ip - self.b_ip + 15 < 512, "the token is one of the window's candidates"
        spos = self.op + lit - off
        assert spos >= self.rb or spos + ml <= max(self.b_op - 128, 0), "the source is in the ring, or flushed"
        self.add(lit, off, ml)
        self.n += 1
        assert self.op - self.b_op <= PAR_BATCH_OUT and self.ip - self.b_ip + 15 <= 785
        if self.n == 64:
            assert self.ip - self.b_ip > 416, "eight candidates per lane stay chosen"
            if self.op - self.rb + self.A + PAR_BATCH_OUT + 32 > PAR_RING:          # the slide at a batch's end
                self.rb = (self.op - PAR_HIST) & ~15
            self._new_batch()

    def hand(self, lit, off, ml):
        """a sequence the batch loop does not take: it ends the batch, and the ring is loaded again behind it"""
        assert lit >= 270 or ml >= 274
        assert self.n < 16 or (self.ip - self.b_ip) * 64 > 416 * self.n
        self.add(lit, off, ml)
        self.rb = (self.op - PAR_HIST) & ~15 if self.op > PAR_HIST else 0
        self._new_batch()

    def close(self):
        if self.n:
            self.hand(3, self.rng.randrange(1, 1401), 300)

    def pad(self, size=7):
        """a near sequence of `size` compressed bytes, 3..7 (no extension byte)"""
        lit = size - 3
        self.seq(lit, self.rng.randrange(1, min(self.op + lit, 1400) + 1), self.rng.randrange(4, 19))

    def fat(self, total=1700):
        """a full batch of 64 sequences of 7 compressed bytes (3 literals, a match with an extension byte) and `total` output bytes"""
        assert self.n == 0
        base, rem = divmod(total, 64)
        for k in range(64):
            n = base + (1 if k < rem else 0)
            self.seq(3, 2 if self.op == 0 else self.rng.randrange(1, min(self.op + 3, 1400) + 1), n - 3)

    def finish(self, start, lo=12288, hi=20480):
        self.close()
        while self.op - start < lo:
            self.fat(1700)
        self.fill(800)
        assert lo <= self.op - start <= hi, (self.op - start)
        return self.block()


def _lead(m, deep):
    """deep: a match of 40 100 bytes first (extension bytes: the sequential decoder's), so that an offset of 40 000 has a source;
    then two full batches, the second of which slides the ring"""
    if deep:
        m.hand(16, 16, 40100)
    start = m.op
    m.fat(1700)
    m.fat(1720)
    assert m.rb == (m.op - PAR_HIST) & ~15 and m.rb >= 1888
    return start


def _far_seq(m, ml, dist, j):
    lit = 3 if ml >= 19 else 4                       # 7 compressed bytes either way
    dpos = m.op + lit
    if dist == 40000:
        off = 40000
    else:
        end = m.rb - (dist - 1) - 3 * j             # one byte behind the source: j = 0 ends `dist` bytes in front of the ring's base
        off = dpos - (end - ml)
    assert off <= 65535 and dpos - off + ml <= m.rb
    m.seq(lit, off, ml)


def _far_batch(m, specs):
    """64 sequences, len(specs) of them far matches (ml, dist) spread over the lanes, the others near"""
    assert m.n == 0 and sum(ml + 4 for ml, _ in specs) + (64 - len(specs)) * PAD_OUT <= PAR_BATCH_OUT
    at = {1 + (j * 62) // len(specs): j for j in range(len(specs))}
    for k in range(64):
        if k in at:
            _far_seq(m, specs[at[k]][0], specs[at[k]][1], at[k])
        else:
            m.pad()


def _alone(ml, dist):
    k = max(1, min(12, (PAR_BATCH_OUT - 64 * PAD_OUT) // (ml + 4)))
    return [(ml, dist)] * k


@functools.lru_cache(maxsize=None)
def _far_items():
    items = []
    near_base = [_alone(ml, d) for ml in FAR_ML for d in (1, 17)] + [[(ml, (1, 17)[i & 1]) for i, ml in enumerate(FAR_ML)]]
    deep = [_alone(ml, 40000) for ml in FAR_ML] + [[(ml, (40000, 1, 17)[i % 3]) for i, ml in enumerate(FAR_ML)]]
    for align in range(16):
        for is_deep, batches in ((False, near_base), (True, deep)):
            for c in range(0, len(batches), 8):
                m = _M(9000 + 64 * align + 2 * c + is_deep, align)
                start = _lead(m, is_deep)
                for specs in batches[c:c + 8]:
                    _far_batch(m, specs)
                blk, n = m.finish(start)
                items.append((blk, n, (7 * c + 3 * align + is_deep) & 15, align))
    return items


@pytest.mark.parametrize("decoder", _PAR)
def test_far_matches_of_every_class(engine, oracle, decoder):
    _run(engine, oracle, _far_items(), decoder, "far matches")


def _lit_batch(m, n, pos, ml):
    """a literal run of n bytes as sequence `pos` of a batch of 64; the sequences around it as large as the window's candidates allow"""
    assert m.n == 0
    if n >= 270:                                     # two extension bytes: handed over where it stands, then the batch's other sequences
        for _ in range(pos):
            m.pad()
        m.hand(n, m.rng.randrange(1, 1401), ml)
        for _ in range(63 - pos):
            m.pad()
        m.close()
        return
    size = 3 + n + (1 if n >= 15 else 0)
    c = 7
    while pos < 63 and 62 * c + size > 496:          # the last sequence's token stays a candidate
        c -= 1
    assert c >= 3 and 63 * c + size > 416
    for k in range(64):
        if k == pos:
            m.seq(n, m.rng.randrange(1, 1401), ml)
        else:
            m.pad(c)


@functools.lru_cache(maxsize=None)
def _lit_items():
    items = []
    cases = [(n, pos) for n in LITS for pos in (0, 31, 63)]
    for align in range(16):
        for c in range(0, len(cases), 7):
            m = _M(9500 + 64 * align + c, align)
            start = _lead(m, False)
            for i, (n, pos) in enumerate(cases[c:c + 7]):
                _lit_batch(m, n, pos, 4 if (align + c + i) & 1 else 13)      # (4: a short run's stores fall short of 8 / 16 bytes)
            blk, size = m.finish(start)
            items.append((blk, size, (5 * c + 11 * align) & 15, align))
    return items


@pytest.mark.parametrize("decoder", _PAR)
def test_literal_runs_of_every_class(engine, oracle, decoder):
    _run(engine, oracle, _lit_items(), decoder, "literal runs")


@functools.lru_cache(maxsize=None)
def _hand_items():
    """A batch of 20 sequences -- far matches of the 4-, 8- and 16-byte classes and one above 32 bytes, a run of 40 literals -- ended
    by a match with two extension bytes; then full batches, whose sources reach back across the sequence that was handed over: the
    lane id and the window are made again behind the call, the ring is loaded again."""
    items = []
    for align in range(16):
        for fats in (0, 1, 2):
            m = _M(9800 + 4 * align + fats, align)
            start = _lead(m, False)
            for _ in range(fats):
                m.fat(1500 + 100 * fats)
            far = {2: (5, 1), 5: (12, 17), 9: (33, 1), 14: (65, 17), 17: (16, 1)}
            for k in range(20):
                if k in far:
                    _far_seq(m, far[k][0], far[k][1], k)
                elif k == 11:
                    m.seq(40, m.rng.randrange(1, 1401), 9)
                else:
                    m.pad()
            m.hand(3, m.rng.randrange(1, 1401), 300)
            m.fat(PAR_BATCH_OUT)
            m.fat(1700)
            blk, n = m.finish(start)
            items.append((blk, n, (3 * align + 5 * fats) & 15, align))
    return items


@pytest.mark.parametrize("decoder", _PAR)
def test_hand_over_behind_far_matches_and_a_long_run(engine, oracle, decoder):
    _run(engine, oracle, _hand_items(), decoder, "hand-over")
