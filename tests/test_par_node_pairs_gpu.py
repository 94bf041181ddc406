"""The speculative parse of k_decode_par and k_decode_par_redo with the nodes interleaved in pairs (decode_par.hpp, parse_square): lane
l speculates the window bytes 128p + 2l and 128p + 2l + 1 for p < NL / 2, and reads the bytes n, n + 1, n + 2 of its pair from the
window's rows of 128 bytes.  What can go wrong is which lane sees which token, so the blocks put tokens on every node and on every
seam between two rows; every result and every byte must be the oracle's, at decoder 2 and at decoder 4 forced (its redo pass is
k_decode_par_redo), and no byte around an output may be written.

  constant   blocks of 2 to 4 KiB of output whose sequences all have the same compressed size s, s = 3 .. 20 (the first sequence of
             the s = 3 block has 4: a block starts with a literal), at all sixteen `src & 15`: 288 blocks in one call.  s <= 6 runs
             the six-node form after the first batch, s >= 8 the eight-node form
  seams      blocks whose sizes come from a seeded generator, and blocks built to put a token on window bytes 126 .. 129, 254 .. 257,
             382 .. 385, 510 and 511 -- with the literal nibble 15 on 127, 255, 383 and 511: its extension byte is the first byte of
             the next row, which no lane of the row reads for itself.  _walk follows the blocks batch by batch the way the decoder
             cuts them and the test asserts that each position was a token of a batch, in both forms
  hops       literal runs of 15 .. 269 bytes (one extension byte): the successor lies one, two or three rows on; 270 is handed over
  clamp      blocks of 64 .. 600 compressed bytes (step 7): inLim lies below the node count of each form, and clamping every successor
             to the absorbing node is what ends the batch
  LDS        k_decode_par and k_decode_par_redo hold nothing in LDS but their ParLds (5120 bytes): their table stores take the table's
             address as the 16-bit base of ds_write_addtid_b32 (par_table_store, TID), which reaches the first 64 KiB only

_run here is test_par_lds_fit_gpu's with the guard in FRONT of the call's first output checked too (behind every output it is checked
there: that is the front of the next one).
"""
import functools
import random

import pytest

import lz4_synth as S
from conftest import DECODERS
from test_par_lds_fit_gpu import _B, _place, GAP

pytestmark = pytest.mark.gpu

_DEC = [d for d in DECODERS if d in (2, 3, 4)] or [2]
FRONT = 64


def _run(engine, oracle, items, decoder, what):
    """items: [(block, cap, data address mod 16, output address mod 16)] as one decompress_batch_device call with 8-byte headers;
    asserts the oracle's code and bytes for every block and that no byte in front of, between or behind the outputs was written"""
    import numpy as np
    import torch
    n = len(items)
    inp = torch.zeros(sum(len(b) + 8 + 16 + GAP for b, _, _, _ in items) + 64, dtype=torch.uint8, device="cuda:0")
    out = torch.full((FRONT + sum(c + 16 + GAP for _, c, _, _ in items) + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    host = np.zeros(inp.numel(), dtype=np.uint8)
    boff, ooff, ip, op = [], [], 0, FRONT
    for blk, cap, ir, orr in items:
        p = _place(inp.data_ptr() + 8, ip, ir)
        host[p:p + 8] = np.frombuffer(len(blk).to_bytes(4, "little") + int(cap).to_bytes(4, "little"), np.uint8)
        host[p + 8:p + 8 + len(blk)] = np.frombuffer(blk, np.uint8)
        boff.append(p)
        ip = p + 8 + len(blk) + GAP
        q = _place(out.data_ptr(), op, orr)
        ooff.append(q)
        op = q + cap + GAP
    assert op <= out.numel()
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
    assert (got[:ooff[0]] == 0xA5).all(), (what, "bytes in front of the first block were written")
    for i, (blk, cap, ir, orr) in enumerate(items):
        code, dec = oracle.decompress_block(blk, cap)
        assert codes[i] == code, (what, i, ir, orr, codes[i], code)
        assert code > 0, (what, i, "the block was written to be valid", code)
        g = got[ooff[i]:ooff[i] + code]
        e = np.frombuffer(dec, np.uint8)
        assert np.array_equal(g, e), (what, i, ir, orr, "bytes differ at", int(np.argmax(g != e)))
        end = ooff[i + 1] if i + 1 < n else len(got)
        assert (got[ooff[i] + code:end] == 0xA5).all(), (what, i, "bytes behind the block were written")


def test_par_lds_is_all_of_the_kernels_lds(engine):
    for k in ("k_decode_par", "k_decode_par_redo"):
        info = engine.kernel_info(k)
        assert info["lds_bytes"] == info["par_lds_bytes"] <= 65536, (k, info)


PAR_WIN, PAR_BATCH_OUT, PAR_ADAPT6 = 832, 1856, 416
SEAMS = (126, 127, 128, 129, 254, 255, 256, 257, 382, 383, 384, 385, 510, 511)
NIBBLE15_AT = (127, 255, 383, 511)


def _sized(b, s, k=0):
    """a plain sequence of exactly s compressed bytes, 3 <= s <= 20, in the k-th of the ways to write it"""
    room = b.op > 0
    if s <= 17 and (k % 3 != 2 or s < 4 or not room):
        lit, ml = s - 3, b.rng.randrange(4, 19)                     # no extension byte
    elif s <= 18:
        lit, ml = s - 4, 19 + b.rng.randrange(0, 12)                # the match's extension byte
    elif k % 2 or s == 19:
        lit, ml = s - 4, b.rng.randrange(4, 19)                     # the literals' extension byte (lit >= 15)
    else:
        lit, ml = s - 5, 19 + b.rng.randrange(0, 12)                # both
    if not room and lit == 0:
        lit = 1                                                     # (a block's first sequence has a literal)
    b.add(lit, b.rng.randrange(1, min(b.op + lit, 1400) + 1), ml)


def _pad_to(b, n, lo, hi):
    """plain sequences of lo .. hi compressed bytes (hi <= 17) until exactly n more compressed bytes are written"""
    end = b.ip + n
    while b.ip < end:
        rem = end - b.ip
        if rem <= hi:
            s = rem
        elif rem < lo + hi:
            s = rem - lo if rem - lo >= lo else rem // 2
        else:
            s = b.rng.randrange(lo, hi + 1)
        assert 3 <= s <= 17 and (rem == s or rem - s >= 3), (rem, s)
        _sized(b, s)
    assert b.ip == end


def _finish(b, lo=2048):
    while b.op < lo:
        _sized(b, b.rng.randrange(7, 13))
    return b.block()


# ---- the decoder's batches, walked ---------------------------------------------------------------------------------------------------

def _walk(blk, cap, in_res):
    """[(nodes per lane, window byte of the token, literal nibble)] of every sequence a batch of the lane-parallel decoder takes, by a
    model of its batch loop: the window starts at the 16-byte boundary in front of the batch, a batch takes up to 64 plain sequences
    whose tokens are among its NL * 64 nodes, which end inside the window and 32 bytes in front of the block's end, and whose output
    stays within PAR_BATCH_OUT; NL follows the batch before (PAR_ADAPT6).  If the decoder cut its batches elsewhere the comparison
    with the oracle would hold all the same; only the positions the blocks aim at would be missed."""
    seqs = [q for q in S.parse(blk) if q[3] is not None]
    ends = [q[0] for q in seqs[1:]] + [S.parse(blk)[-1][0]]
    res, i, nl, op = [], 0, 8, 0
    while i < len(seqs) and len(blk) - seqs[i][0] >= 64 and cap - op >= 128:
        ip = seqs[i][0]
        wofs = (in_res + ip) & 15
        lim = min(len(blk) - (ip - wofs) - 32, PAR_WIN)
        n, out = 0, 0
        while i + n < len(seqs) and n < 64:
            tp, _, lit, off, ml, _ = seqs[i + n]
            w = tp - ip + wofs
            plain = lit <= 269 and ml <= 273 and off != 0
            if w >= nl * 64 or w > lim or not plain or ends[i + n] - ip + wofs > lim or out + lit + ml > PAR_BATCH_OUT or \
                    op + out + lit + ml + 64 >= cap:
                break
            res.append((nl, w, blk[tp] >> 4))
            out += lit + ml
            n += 1
        if n == 0:                                     # handed over: one sequence by the sequential decoder
            op += seqs[i][2] + seqs[i][4]
            i += 1
            continue
        used = ends[i + n - 1] - ip
        more = i + n < len(seqs) and seqs[i + n][0] - ip + wofs < nl * 64
        if n >= 16:
            nl = 6 if used * 64 <= PAR_ADAPT6 * n else 8
        elif nl == 6 and not more:
            nl = 8
        op += out
        i += n
    return res


# ---- constant-size blocks ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _constant_items():
    items = []
    for s in range(3, 21):
        for in_res in range(16):
            b = _B(20000 + 16 * s + in_res)
            k = 0
            while b.op < 2048:
                _sized(b, s, k)
                k += 1
            blk, n = b.block()
            assert 2048 <= n <= 4096
            sizes = {y[0] - x[0] for x, y in zip(S.parse(blk), S.parse(blk)[1:])}
            assert sizes <= ({s, 4} if s == 3 else {s}), (s, sizes)
            items.append((blk, n, in_res, (5 * in_res + s) & 15))
    return items


def test_constant_blocks_run_both_forms():
    for s in range(3, 21):
        for blk, n, in_res, _ in _constant_items()[16 * (s - 3):16 * (s - 2)]:
            forms = {nl for nl, _, _ in _walk(blk, n, in_res)}
            assert (forms == {6, 8} if s <= 6 else forms == {8} if s >= 8 else forms), (s, in_res, forms)


@pytest.mark.parametrize("decoder", _DEC)
def test_constant_size_sequences(engine, oracle, decoder):
    items = _constant_items()
    assert len(items) == 288
    _run(engine, oracle, items, decoder, "constant size")


# ---- seams ---------------------------------------------------------------------------------------------------------------------------

def _eight_block(target, in_res, lit15, seed):
    """the block's first batch (eight nodes per lane) has a token at window byte `target`"""
    b = _B(seed)
    _pad_to(b, target - in_res, 8, 17)
    assert len(b.seqs) < 64
    _probe(b, lit15)
    return _finish(b)


def _six_block(target, in_res, lit15, seed):
    """a first batch of 64 sequences of 6 bytes -- 384 compressed bytes, so the next window starts where the first did and has six
    nodes per lane --, then a token at window byte `target` of the second batch behind at most 63 sequences of 5 .. 7 bytes"""
    b = _B(seed)
    for _ in range(64):
        _sized(b, 6)
    n0 = len(b.seqs)
    _pad_to(b, target - in_res, 5 if target - in_res < 370 else 6, 7)
    assert len(b.seqs) - n0 < 64
    _probe(b, lit15)
    return _finish(b)


def _probe(b, lit15):
    if lit15:
        b.add(15 + b.rng.randrange(0, 40), b.rng.randrange(1, b.op + 1), b.rng.randrange(4, 30))
    else:
        _sized(b, b.rng.randrange(5, 12))


def _random_block(in_res, lo, hi, seed):
    b = _B(seed)
    while b.op < 3000:
        _sized(b, b.rng.randrange(lo, hi + 1), b.rng.randrange(6))
    return b.block()


@functools.lru_cache(maxsize=None)
def _seam_items():
    items = []
    for j, t in enumerate(SEAMS):
        for c, in_res in enumerate(((3 * j) & 15, (3 * j + 7) & 15)):
            lit15 = t in NIBBLE15_AT and c == 0
            items.append(_eight_block(t, in_res, lit15, 31000 + 16 * t + in_res) + (in_res, (t + in_res) & 15))
            if t < 384:
                items.append(_six_block(t, in_res, lit15, 32000 + 16 * t + in_res) + (in_res, (t + 5 * in_res) & 15))
    for in_res in range(16):
        items.append(_random_block(in_res, 8, 17, 33000 + in_res) + (in_res, (7 * in_res) & 15))
        items.append(_random_block(in_res, 5, 7, 33100 + in_res) + (in_res, (9 * in_res) & 15))
    return items


def test_seam_positions_occur():
    """from the test's own walk of the blocks: every seam position is a token of a batch, and the tokens on a row's last byte have
    the literal nibble 15 in a block of each form"""
    seen, seen15 = set(), set()
    for blk, n, in_res, _ in _seam_items():
        for nl, w, nib in _walk(blk, n, in_res):
            seen.add((nl, w))
            if nib == 15:
                seen15.add((nl, w))
    assert not [(8, t) for t in SEAMS if (8, t) not in seen], sorted(seen)
    assert not [(6, t) for t in SEAMS if t < 384 and (6, t) not in seen], sorted(seen)
    assert not [(nl, w) for nl, w in seen if w >= nl * 64]
    assert all((8, t) in seen15 for t in NIBBLE15_AT) and all((6, t) in seen15 for t in NIBBLE15_AT if t < 384), sorted(seen15)


@pytest.mark.parametrize("decoder", _DEC)
def test_tokens_on_every_seam(engine, oracle, decoder):
    _run(engine, oracle, _seam_items(), decoder, "seams")


# ---- long hops -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _hop_items():
    items = []
    for in_res in range(16):
        b = _B(34000 + in_res)
        _pad_to(b, 40 + in_res, 8, 17)
        for lit in range(15 + in_res, 270, 16):               # every run length 15 .. 269 over the sixteen blocks
            b.add(lit, b.rng.randrange(1, min(b.op + lit, 1400) + 1), b.rng.randrange(4, 30))
            for _ in range(b.rng.randrange(0, 4)):
                _sized(b, b.rng.randrange(4, 14))
        items.append(_finish(b) + (in_res, (11 * in_res) & 15))
    for in_res in (0, 5, 15):                                 # 270 literals: two extension bytes, handed over where it stands
        b = _B(34100 + in_res)
        _pad_to(b, 100 + in_res, 8, 17)
        b.add(270, b.rng.randrange(1, b.op + 1), 9)
        _pad_to(b, 120, 8, 17)
        b.add(269, b.rng.randrange(1, b.op + 1), 9)
        items.append(_finish(b) + (in_res, in_res ^ 9))
    return items


def test_hops_cover_every_run_length():
    lits = {q[2] for blk, _, _, _ in _hop_items() for q in S.parse(blk) if q[3] is not None}
    assert set(range(15, 271)) <= lits


@pytest.mark.parametrize("decoder", _DEC)
def test_long_hops(engine, oracle, decoder):
    _run(engine, oracle, _hop_items(), decoder, "long hops")


# ---- clamp ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _clamp_items():
    items = []
    for j, src_len in enumerate(range(64, 601, 7)):
        for lo, hi in ((8, 12), (4, 6)):                      # eight nodes per lane throughout; six behind the first batch
            b = _B(35000 + 2 * src_len + (lo == 4))
            _pad_to(b, src_len - 13, lo, hi)
            blk, n = b.block()
            assert len(blk) == src_len
            items.append((blk, max(n, 128), (j + lo) & 15, (3 * j + lo) & 15))
    return items


def test_clamp_blocks_end_below_the_nodes():
    forms = set()
    for blk, n, in_res, _ in _clamp_items():
        assert 64 <= len(blk) <= 600
        forms |= {nl for nl, _, _ in _walk(blk, n, in_res)}
    assert forms == {6, 8}


@pytest.mark.parametrize("decoder", _DEC)
def test_clamp_to_the_absorbing_node(engine, oracle, decoder):
    _run(engine, oracle, _clamp_items(), decoder, "clamp")
