"""The copy phases of the lane-parallel decoder's batch loop (decode_par.hpp, steps 5 to 7), whose registers are no longer zeroed and
whose steps run on a masked length: the literals' r0 / r1, the far classes' f0 f1 fa fb fw0 fw1 and the far loop's pair, the near
step's v0 / v1 (a 16-byte match reads its second chunk from the ring like a longer one), and the heads of the near and the far
32-byte loops (`stepMl`, `farMl`: 0 in the lanes that do not copy).  Every store of those registers must stand under the condition
of its load, in lanes that disagree within one batch and in the lanes beyond `nseq`; a wrong condition shows in a neighbouring
sequence's bytes or in the guard bytes.  So every block is hand-built, every case runs at decoder 2 and at decoder 4 forced (its
redo pass is k_decode_par_redo), every byte and every result is the oracle's, and 64 guard bytes in front of, between and behind
the outputs stay as they were (test_par_node_pairs_gpu's _run).  The dictionary form runs through a linked device call (dense
outputs: the guard is behind the call's last output, tests/guarded.py).

  classes    match lengths 4, 5, 7, 8, 9, 11, 12, 15, 16, 17, 31, 32, 33, 64, 65 at offsets 1, 3, 7, 8, 15, 16, 31, 32, ml - 1, ml
             and ml + 1: all three chunk classes (16, 8 and 4 bytes), the 8-byte funnel's ml - 8 = 0..7, the 4-byte funnel's
             ml - 4 = 0..3, the self-overlapping copies, one 32-byte step and more.  Every probe is followed by a long match, so
             that no batch fills its 64 lanes, and sources lie one sequence back, so that lanes of one batch copy in different rounds
  literals   runs of 0, 1, 7, 8, 9, 15, 16, 17, 32 and 33 literals in front of those matches, n + ml on both sides of 8 and of 16
  far        the same lengths with the source behind the ring's history (only a block's output beyond 3200 bytes makes the ring
             slide, so these probes are the last 200 bytes in front of a 4 KiB block's tail), beside near matches in the same batch
  dictionary the same lengths with the source in the block before, in a linked stream

_walk follows the blocks batch by batch the way the decoder cuts them (test_par_node_pairs_gpu's model, with the ring's base added)
and the tests assert from it that every listed value occurred where it was aimed.  The field decode, the rank queries and the
window-edge path have no case here: that code is the parent's, instruction for instruction.
"""
import functools

import pytest

import lz4_synth as S
from conftest import DECODERS
from test_par_lds_fit_gpu import _B
from test_par_node_pairs_gpu import _run, PAR_WIN, PAR_BATCH_OUT, PAR_ADAPT6

pytestmark = pytest.mark.gpu

_DEC = [d for d in DECODERS if d in (2, 3, 4)] or [2]
PAR_RING, PAR_HIST = 5088, 1500
MLS = (4, 5, 7, 8, 9, 11, 12, 15, 16, 17, 31, 32, 33, 64, 65)
OFFS = (1, 3, 7, 8, 15, 16, 31, 32)
LITS = (0, 1, 7, 8, 9, 15, 16, 17, 32, 33)


def _offsets(ml):
    return sorted(set(OFFS) | {ml - 1, ml, ml + 1})


class _D(_B):
    """_B with `base` bytes of dictionary in front of the block: an offset may reach into them"""

    def __init__(self, seed, base=0):
        super().__init__(seed)
        self.base = base

    def add(self, lit, off, ml):
        lits = bytes(self.rng.randrange(256) for _ in range(lit))
        assert 1 <= off <= self.base + self.op + lit
        self.seqs.append((lits, off, ml))
        self.ip += S.seq_size(lit, ml)
        self.op += lit + ml


def _spacer(b):
    """a long match whose source lies well back: two sequences per 60 output bytes, so 64 of them never fit a batch"""
    lit = b.rng.randrange(0, 4) if b.op else 8
    b.add(lit, b.rng.randrange(40, min(b.op + lit, 1400) + 1) if b.op + lit >= 40 else b.op + lit, 56 + b.rng.randrange(0, 8))


def _tail(b):
    """behind the probes: over 64 output bytes and over 32 compressed bytes, which a batch leaves to the sequential decoder"""
    _spacer(b)
    for _ in range(8):
        b.add(2, b.rng.randrange(40, 200), 6)
    return b.block()


# ---- the decoder's batches, walked ---------------------------------------------------------------------------------------------------

def _walk(blk, cap, in_res, out_res, dict_len=0):
    """[[(lit, off, ml, kind, waits)] per batch]: test_par_node_pairs_gpu's model of the batch loop with the ring added.  kind is
    'near' (the source starts in the ring), 'far' (it ends below the ring's base: global memory) or 'dict' (it ends at or below
    the block's first byte); waits says that the source reaches into this batch's own output, so the lane copies in a later round
    than the lanes whose sources are complete.  The ring slides behind a batch that leaves less than PAR_BATCH_OUT + 32 bytes."""
    seqs = [q for q in S.parse(blk) if q[3] is not None]
    ends = [q[0] for q in seqs[1:]] + [S.parse(blk)[-1][0]]
    res, i, nl, op, base = [], 0, 8, 0, 0
    while i < len(seqs) and len(blk) - seqs[i][0] >= 64 and cap - op >= 128:
        ip = seqs[i][0]
        wofs = (in_res + ip) & 15
        lim = min(len(blk) - (ip - wofs) - 32, PAR_WIN)
        n, out, batch = 0, 0, []
        while i + n < len(seqs) and n < 64:
            tp, _, lit, off, ml, _ = seqs[i + n]
            w = tp - ip + wofs
            dpos = op + out + lit
            spos = dpos - off
            if spos >= base:
                kind = "near"
            elif spos >= 0 and spos + ml <= base:
                kind = "far"
            elif dict_len and spos >= -dict_len and spos + ml <= 0:
                kind = "dict"
            else:
                break                                  # (straddles: the sequential decoder's)
            plain = lit <= 269 and ml <= 273 and off != 0
            if w >= nl * 64 or w > lim or not plain or ends[i + n] - ip + wofs > lim or out + lit + ml > PAR_BATCH_OUT or \
                    op + out + lit + ml + 64 >= cap:
                break
            batch.append((lit, off, ml, kind, kind == "near" and min(spos + ml, dpos - lit) > max(spos, op)))
            out += lit + ml
            n += 1
        if n == 0:                                     # handed over: one sequence by the sequential decoder, the ring reloaded
            op += seqs[i][2] + seqs[i][4]
            base = (op - PAR_HIST) & ~15 if op > PAR_HIST else 0
            i += 1
            continue
        res.append(batch)
        used = ends[i + n - 1] - ip
        more = i + n < len(seqs) and seqs[i + n][0] - ip + wofs < nl * 64
        if n >= 16:
            nl = 6 if used * 64 <= PAR_ADAPT6 * n else 8
        elif nl == 6 and not more:
            nl = 8
        op += out
        i += n
        if op - base + out_res + PAR_BATCH_OUT + 32 > PAR_RING:
            base = (op - PAR_HIST) & ~15
    return res


def _assert_batches_never_fill(walks):
    assert walks and all(0 < len(batch) < 64 for w in walks for batch in w), sorted({len(batch) for w in walks for batch in w})


# ---- near matches and literal runs ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _near_items():
    probes = [(ml, off) for ml in MLS for off in _offsets(ml) if off >= 1]
    items, k = [], 0
    for rep in range(2):                               # every probe twice, with another literal run and at another alignment
        j = 0
        while j < len(probes):
            b = _B(41000 + 1000 * rep + j)
            _spacer(b)
            _spacer(b)
            while j < len(probes) and b.op < 3600:
                ml, off = probes[j]
                b.add(LITS[(j + 3 * rep) % len(LITS)], off, ml)
                _spacer(b)
                j += 1
            while b.op < 2048:
                _spacer(b)
            blk, n = _tail(b)
            assert 2048 <= n <= 4096, n
            items.append((blk, n, k & 15, (5 * k + 3) & 15))
            k += 1
    for n_lit in LITS:                                 # every literal run in front of every class, n + ml around 8 and 16
        b = _B(43000 + n_lit)
        _spacer(b)
        for ml in MLS:
            b.add(n_lit, max(ml, 8) + b.rng.randrange(0, 30), ml)
            if ml < 12:
                b.add(n_lit, 1 + b.rng.randrange(0, 3), ml)
            _spacer(b)
        while b.op < 2048:
            _spacer(b)
        blk, n = _tail(b)
        assert 2048 <= n <= 4096, n
        items.append((blk, n, (n_lit + 7) & 15, n_lit & 15))
    return items


def test_near_probes_occur():
    """from the walk: every length at every offset and every literal run in front of every length is a near match of a batch; the
    chunk classes, both funnels and the self-overlap are all there; a batch has lanes that wait beside lanes that do not; and no
    batch fills, so lanes beyond nseq are present in every one"""
    walks = [_walk(blk, n, ir, orr) for blk, n, ir, orr in _near_items()]
    _assert_batches_never_fill(walks)
    near = [q for w in walks for batch in w for q in batch if q[3] == "near"]
    seen = {(ml, off) for _, off, ml, _, _ in near}
    assert not [(ml, off) for ml in MLS for off in _offsets(ml) if off >= 1 and (ml, off) not in seen]
    assert not [(n, ml) for n in LITS for ml in MLS if not any(q[0] == n and q[2] == ml for q in near)]
    g16 = {ml for _, off, ml, _, _ in near if ml >= 16 and off >= 8 and (off >= 32 or off >= ml)}
    g8 = {ml - 8 for _, off, ml, _, _ in near if 8 <= ml < 16 and off >= 8 and (off >= 32 or off >= ml)}
    g4 = {ml - 4 for _, off, ml, _, _ in near if ml < 8 and off >= ml}
    slow = {(ml, off) for _, off, ml, _, _ in near if not ((ml >= 8 and off >= 8 and (off >= 32 or off >= ml)) or (ml < 8 and off >= ml))}
    assert g16 >= {16, 17, 31, 32, 33, 64, 65} and g8 >= {0, 1, 3, 4, 7} and g4 >= {0, 1, 2, 3}, (g16, g8, g4)
    assert {(16, 15), (33, 31), (9, 8), (4, 3), (65, 1)} <= slow
    sums = {(n > 8, n + ml < 8, n + ml < 16) for n, _, ml, _, _ in near if n > 0}
    assert {(False, True, True), (False, False, True), (False, False, False), (True, False, True), (True, False, False)} <= sums, sums
    assert any(any(q[4] for q in batch if q[3] == "near") and any(not q[4] for q in batch if q[3] == "near") for w in walks for batch in w)


@pytest.mark.parametrize("decoder", _DEC)
def test_near_classes_and_literal_runs(engine, oracle, decoder):
    items = _near_items()
    _run(engine, oracle, items * (200 // len(items) + 1), decoder, "near classes")


# ---- far matches ---------------------------------------------------------------------------------------------------------------------

FAR_GROUPS = ((4, 5, 7, 8, 9, 11, 12), (15, 16, 17, 31), (32, 33, 64), (65, 16, 8, 4))


@functools.lru_cache(maxsize=None)
def _far_items():
    items = []
    for g, mls in enumerate(FAR_GROUPS):
        for c in range(16):
            b = _B(45000 + 16 * g + c)
            _spacer(b)
            while b.op < 3712:                         # two batches of output: the ring has slid when the probes come
                _spacer(b)
            for j, ml in enumerate(mls):
                lit = (0, 1, 7, 8)[(j + c) & 3] if sum(mls) < 120 else (0, 1)[(j + c) & 1]
                b.add(lit, b.op + lit - b.rng.randrange(40, 900), ml)          # source at output 40 .. 900 + ml
                if j & 1:
                    b.add(1, 20 + b.rng.randrange(0, 12), 4 + (j & 3))         # a near match between them
            blk, n = _tail(b)
            assert n <= 4096 + 64, n
            items.append((blk, n, (c + g) & 15, (3 * c + g) & 15))
    return items


def test_far_probes_occur():
    walks = [_walk(blk, n, ir, orr) for blk, n, ir, orr in _far_items()]
    _assert_batches_never_fill(walks)
    far = {q[2] for w in walks for batch in w for q in batch if q[3] == "far"}
    assert far >= set(MLS), sorted(far)
    assert any(q[3] == "far" and q[2] > 32 for w in walks for batch in w for q in batch)                # the far loop beyond 32 bytes
    assert any({"far", "near"} <= {q[3] for q in batch} for w in walks for batch in w)                  # both kinds in one batch


@pytest.mark.parametrize("decoder", _DEC)
def test_far_classes(engine, oracle, decoder):
    items = _far_items()
    _run(engine, oracle, items * (200 // len(items) + 1), decoder, "far classes")


# ---- far matches into the dictionary, in a linked stream -----------------------------------------------------------------------------

DICT_LEN = 4000


@functools.lru_cache(maxsize=None)
def _dict_stream():
    """[(name, block, cap, True)]: a block of plain output, then a block whose probes copy from it, eight times over"""
    st = []
    for c in range(8):
        d = _B(47000 + c)
        _spacer(d)
        while d.op < DICT_LEN - 140:
            _spacer(d)
        blk, n = d.block()
        st.append(("dictionary %d" % c, blk, n, True))
        b = _D(47100 + c, base=n)
        _spacer(b)
        for j, ml in enumerate(MLS):
            lit = LITS[(j + c) % len(LITS)]
            b.add(lit, b.op + lit + b.rng.randrange(ml, 3000), ml)             # ends at or below the block's first byte
            _spacer(b)
            if (j + c) & 1:
                b.add(LITS[(j + 2 * c) % len(LITS)], _offsets(ml)[(j + c) % len(_offsets(ml))] or 1, ml)
        blk2, n2 = _tail(b)
        st.append(("probes %d" % c, blk2, n2, True))
    return st


def test_dictionary_probes_occur():
    st = _dict_stream()
    walks = [_walk(blk, n, 0, 0, dict_len=st[i - 1][2]) for i, (_, blk, n, _) in enumerate(st) if i & 1]
    _assert_batches_never_fill(walks)
    seen = {q[2] for w in walks for batch in w for q in batch if q[3] == "dict"}
    assert seen >= set(MLS), sorted(seen)
    assert any({"dict", "near"} <= {q[3] for q in batch} for w in walks for batch in w)


@pytest.mark.parametrize("decoder", _DEC)
def test_dictionary_classes_linked(engine, oracle, decoder):
    """the stream 14 times over in one linked device call (224 blocks), then as the call's own dictionary through the host call"""
    from test_parity_gpu import _decode_streams
    st = _dict_stream() * 14
    expect = S.linked_expect(oracle, st)
    assert all(code == cap for (code, _), (_, _, cap, _) in zip(expect, st))
    engine.set_decoder(decoder)
    try:
        out, res, ulen, _ = _decode_streams(engine, [S.framed([(b, c) for _, b, c, _ in st])], "one")
        assert res == [code for code, _ in expect]
        assert out == b"".join(dec for _, dec in expect)
        for k in range(1, 16, 2):
            o, blen = engine.decompress_batch(S.framed([st[k][1:3]]), linked=True, dict_bytes=expect[k - 1][1], raise_on_block_error=False)
            assert blen == [expect[k][0]] and o == expect[k][1], k
    finally:
        engine.set_decoder(0)
