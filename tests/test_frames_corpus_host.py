"""The inputs of tests/frames_corpus.py, the part that needs no GPU: the builders are held to what each family is for -- the
model accepts and refuses what the corpus says it should, the checksum and size fields the builders wrote are right wherever the
model gets that far, frames are wider than a wavefront, pairs of errors lie in different 64-block chunks and show both halves of
the "which error wins" contract, the stored sweep meets every residue, the mutations meet every code -- and, where the system
liblz4 loads, the model is held to LZ4F_decompress on every input it accepts."""
import collections
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import frames_corpus as K  # noqa: E402
import frames_model as M  # noqa: E402
import lz4_synth as Z  # noqa: E402
import lz4f  # noqa: E402
from test_frames_gpu import expect  # noqa: E402  (the model's answers, kept once a process)

L = lz4f.load()
LOAD_CODES = set(M.NAMES)
ALL = sorted(K.FAMILIES)


def answers(oracle, name, flags=0):
    """[(case, (sizes entry, result entry, bytes))]"""
    return [(c, expect(oracle, c[0], c[1], flags)) for c in K.family(name, oracle)]


def tally(ans):
    """(accepted, refused at load, refused at decode)"""
    return (sum(1 for _, (s, r, _b) in ans if r >= 0), sum(1 for _, (s, r, _b) in ans if s < 0),
            sum(1 for _, (s, r, _b) in ans if s >= 0 and r < 0))


def n_blocks(data):
    return [len(f.blocks) for f in M.walk(data)[0]]


def test_seam_dictionaries_are_not_one_byte():
    for dl in Z.SEAM_DICT_LENS:
        d = Z.seam_dictionary(dl)
        assert len(d) == dl and (dl < 16 or len(set(d)) > min(dl, 256) // 4)


def test_builders_decoder_is_the_models(oracle):
    """frames_corpus.decode, which the checksum and size fields are made with, against the oracle on every corpus block"""
    n = 0
    for c in Z.independent_cases():
        got = K.decode(c.block)
        if got is not None:
            r, want = oracle.decompress_block(c.block, len(got))
            if r >= 0:                              # (the oracle also applies the end rules, which is not this decoder's business)
                assert (r, want) == (len(got), got), c
                n += 1
    assert n >= 251


def test_corpus_in_frames(oracle):
    """A: 264 blocks, 236 of them a second time with code 4; for the plain independent form the model accepts 251, refuses 10 at
    load and 3 at decode; a refusal is always FRM_E_BLOCK -- never a checksum or a content size the builder got wrong"""
    cases = Z.independent_cases()
    assert len(cases) == 264 and max(c.cap for c in cases) < (1 << 18)
    ind, lnk = answers(oracle, "A-independent"), answers(oracle, "A-linked")
    assert len(ind) == len(lnk) == 264 + 236
    plain = [a for a in ind if a[0][0].startswith("A/indep-b5/")]
    assert len(plain) == 264 and tally(plain) == (251, 10, 3)
    for ans in (ind, lnk):
        assert all(r >= 0 or r == M.E_BLOCK for _, (s, r, _b) in ans)
    # behind two blocks nothing is lost: what the model accepts alone it accepts there, with the same bytes at the end
    for (ci, (si, ri, bi)), (cl, (sl, rl, bl)) in zip(ind, lnk):
        if ri >= 0:
            assert rl == ri + 333 + 1500 and bl.endswith(bi), cl[0]
    assert all(n_blocks(c[1]) == [3] for c, _ in lnk)


def test_seam_corpus_in_frames(oracle):
    """B: every cut and every probe block, one linked frame each; the dictionary lies in pieces of both kinds"""
    cuts, fam = answers(oracle, "B-cuts"), answers(oracle, "B-family")
    assert len(cuts) == len(Z.seam_cuts()) == 1212 and len(fam) == len(Z.seam_family()) == 3022
    assert tally(cuts) == (1157, 46, 9) and tally(fam) == (2989, 0, 33)
    for ans in (cuts, fam):
        assert all(r >= 0 or r == M.E_BLOCK for _, (s, r, _b) in ans)
    # a valid case's content is its dictionary and what the block decodes to behind it
    for (c, (s, r, b)), (_, dl, blk, cap, valid) in zip(fam, Z.seam_family()):
        if valid:
            d = Z.seam_dictionary(dl)
            assert r == dl + cap and b == d + oracle.decompress_block(blk, cap, d)[1], c[0]
    kinds = collections.Counter()
    widest = 0
    for c, _ in cuts + fam:
        f = M.walk(c[1])[0][0]
        assert not f.flg & 0x20
        for (_p, stored, payload, _ck) in f.blocks[:-1]:
            kinds[stored] += 1
        widest = max(widest, len(f.blocks))
    assert kinds[True] > 3000 and kinds[False] > 3000 and widest > 30
    behind = answers(oracle, "B-behind")
    assert len(behind) == sum(1 for n, dl, *_ in Z.seam_family() if dl == 100 and "one in front" in n) >= 4
    for c, (s, r, _b) in behind:
        assert s > 0 and r == M.E_BLOCK and n_blocks(c[1])[0] == 2


def test_wide_frames(oracle):
    """C: the block counts on both sides of one and two wavefronts, all 16 flag combinations, stored, empty and one-byte blocks"""
    wide = answers(oracle, "C-wide")
    seen = set()
    for c, (s, r, _b) in wide:
        assert r == s > 0, c[0]
        f = M.walk(c[1])[0][0]
        seen.add((len(f.blocks), f.flg & 0x3C))
        if len(f.blocks) >= 63 and "truly" not in c[0]:
            assert any(st and not p for _, st, p, _ in f.blocks) and any(not st and p == b"\x00" for _, st, p, _ in f.blocks)
    assert {n for n, _ in seen} >= set(K.WIDE_COUNTS)
    for n in K.WIDE_COUNTS:
        assert len({flg for m, flg in seen if m == n}) == 16
    # the truly linked frames need their window: decoded block by block on their own they do not come out
    for c, (s, r, b) in wide:
        if "truly" in c[0]:
            f = M.walk(c[1])[0][0]
            assert sum(1 for _, st, p, _ in f.blocks if oracle.decompress_block(p, 400)[0] < 0) > len(f.blocks) // 2


def test_placed_errors(oracle):
    """C: one error at block 0, 63, 64, 65, 128 and the last of 300; then two, in different chunks of 64 blocks"""
    one = answers(oracle, "C-one")
    want = {"bsum": (M.E_BLOCK_CHECKSUM, M.E_BLOCK_CHECKSUM), "load": (M.E_BLOCK, M.E_BLOCK), "decode": (None, M.E_BLOCK)}
    assert len(one) == 2 * 3 * len(K.DAMAGE_AT)
    for c, (s, r, _b) in one:
        kind = c[0].split()[1]
        assert r == want[kind][1] and (s == want[kind][0] if want[kind][0] else s > 0), c[0]
        assert n_blocks(c[1]) == [300]
    pairs = answers(oracle, "C-pairs")
    code = {"bsum": M.E_BLOCK_CHECKSUM, "load": M.E_BLOCK, "decode": M.E_BLOCK, "csize": M.E_CONTENT_SIZE, "csum": M.E_CONTENT_CHECKSUM}
    at_load = ("bsum", "load", "csize")
    seen = set()
    load_beats_earlier_decode = later_chunk_loses = 0
    for c, (s, r, _b) in pairs:
        x, y = c[2]
        seen.add((x, y))
        # the contract, spelled out: a load-time error beats every decode-time one; among equals the first position wins
        if x in at_load or y not in at_load:
            assert r == code[x], c[0]
        else:
            assert r == code[y], c[0]
        assert (s < 0) == (x in at_load or y in at_load), c[0]
        if x not in at_load and y in at_load:
            load_beats_earlier_decode += 1
        if x in at_load and y in at_load and code[x] != code[y] and x != "csize":
            later_chunk_loses += 1
            assert max(n_blocks(c[1])) == 200
    assert seen == {(x, y) for x in K.KINDS for y in K.KINDS if not (x == y and x in ("csize", "csum"))}
    assert load_beats_earlier_decode >= 6 and later_chunk_loses >= 4


def test_inputs_of_many_frames(oracle):
    many = dict((c[0], (c[1], a)) for c, a in answers(oracle, "C-many"))
    for name, n in (("C/many/70 frames", 70), ("C/many/200 frames", 200)):
        data, (s, r, b) = many[name]
        nb = n_blocks(data)
        assert len(nb) == n and r == s > 0 and 65 in nb and 1 in nb and data.count(b"\x2a\x4d\x18") > n // 8
        flgs = {f.flg & 0x20 for f in M.walk(data)[0]}
        assert flgs == {0, 0x20}
    data, (s, r, _b) = many["C/many/200 frames, 3 and 150 fail"]
    assert s > 0 and r == M.E_BLOCK and len(n_blocks(data)) == 200
    for name, want in (("C/many/cut in frame 100", M.E_TRUNCATED), ("C/many/bad magic at frame 100", M.E_MAGIC)):
        data, (s, r, _b) = many[name]
        frames, err = M.walk(data)
        assert s == r == want and err[1] == want and len([f for f in frames if f.end is not None]) == 100


def test_stored_sweep(oracle):
    """D: every N with every P in both kinds of frame; in the order of the GPU test's call the second block's destination and
    source meet all 16 residues with every N around the 512-byte threshold"""
    cases = K.family("D", oracle)
    assert {(c[2][0], c[2][1], c[2][2]) for c in cases} == {(N, P, lk) for N in K.STORED_N for P in range(16) for lk in (True, False)}
    for c, (s, r, b) in answers(oracle, "D"):
        N, P, linked, at = c[2]
        assert r == s == N + P and c[1][at:at + N] == b[P:] and bool(M.walk(c[1])[0][0].checksum is not None) == (N <= 1040)
    dst, src = K.stored_residues(K.shuffled(cases, K.STORED_SEED))
    want = {(N, res) for N in K.STORED_EDGE for res in range(16)}
    assert want <= dst and want <= src
    assert {res for _, res in dst} == {res for _, res in src} == set(range(16))


def test_block_maxima(oracle):
    ans = dict((c[0], a) for c, a in answers(oracle, "E"))
    for bid in (4, 5, 6, 7):
        bmax = 1 << (8 + 2 * bid)
        for tag in ("L", "I"):
            assert ans["E/b%d %s compressed max" % (bid, tag)][:2] == (bmax, bmax)
            assert ans["E/b%d %s compressed max + 1" % (bid, tag)][:2] == (M.E_BLOCK, M.E_BLOCK)
        assert ans["E/b%d stored max" % bid][:2] == (bmax, bmax)
        assert ans["E/b%d block word max + 1" % bid][1] == ans["E/b%d compressed block word max + 1" % bid][1] == M.E_BLOCK_SIZE
    for bid in (4, 5):
        s, r, b = ans["E/b%d three maximal blocks linked" % bid]
        bmax = 1 << (8 + 2 * bid)
        assert r == s == 3 * bmax
        assert b[bmax + 8:bmax + 28] == b[bmax + 8 - 65535:bmax + 28 - 65535] and b[:bmax] != b[bmax:2 * bmax]


def test_mutations(oracle):
    """F: 32 bases, 24 mutations each in six modes; the model meets every code and "valid" at least 10 times and refuses at
    least 30 at decode"""
    cases = K.family("F", oracle)
    assert len(cases) == 768 and collections.Counter(c[2] for c in cases) == {m: 128 for m in K.MODES}
    bases = K.mutation_bases(oracle)
    assert len(bases) == 32 and sorted(set(tuple(n_blocks(b.data)) for _, b in bases)) == [(5,), (70,)]
    for flags in (0, 3):
        ans = answers(oracle, "F", flags)
        count = collections.Counter(M.NAMES.get(r, "valid") for _, (s, r, _b) in ans)
        if flags == 0:
            assert set(count) == set(M.NAMES.values()) | {"valid"} and min(count.values()) >= 10, count
            assert tally(ans)[2] >= 30
        else:
            assert not count["BLOCK_CHECKSUM"] and not count["CONTENT_CHECKSUM"] and count["valid"] > 100


def test_checksums_where_the_content_is_small(oracle):
    """every frame of A, B and E whose content is at most 64 KiB has both checksums; of the larger ones some have"""
    big = collections.Counter()
    for fam in ("A-independent", "A-linked", "B-cuts", "B-family", "E"):
        for c, (s, r, _b) in answers(oracle, fam):
            if r < 0:
                continue
            f = M.walk(c[1])[0][0]
            both = bool(f.flg & 0x10) and bool(f.flg & 4)
            assert both or r > K.SMALL, c[0]
            if r > K.SMALL:
                big[both] += 1
    assert big[True] >= big[False] // 8 > 0


@pytest.mark.skipif(L is None, reason="system liblz4 with LZ4F_* not found")
@pytest.mark.parametrize("name", ALL)
def test_liblz4_reads_what_the_model_accepts(oracle, name):
    """LZ4F_decompress on every input the model accepts, byte for byte.  (What the model refuses liblz4 may accept: the size
    rule is the header's, not the format's.)"""
    n = 0
    for c, (s, r, b) in answers(oracle, name):
        if r >= 0:
            assert lz4f.decompress(L, c[1], r + 16) == b, c[0]
            n += 1
    assert n or name in ("B-behind", "C-one", "C-pairs")
