"""The hand-built LZ4 blocks of tests/lz4_synth.py, on the host: the writer writes what the format says (plain_decode, the
oracle and the reference agree on every block, code and bytes), and every family still reaches the edges it names -- recomputed
from the written blocks, so that an edit of the generator cannot quietly lose coverage."""
import numpy as np
import pytest

import lz4_synth as S


@pytest.fixture(scope="module")
def cases():
    return S.independent_cases()


@pytest.fixture(scope="module")
def dict_streams():
    return S.dictionary_streams()


def test_every_block_decodes_as_written(oracle, cases):
    assert len(cases) > 200
    for c in cases:
        code, dec = oracle.decompress_block(c.block, c.cap)
        assert (code >= 0) == c.valid, (c, code)
        pcode, pdec = S.plain_decode(c.block, c.cap)
        assert (pcode >= 0) == (code >= 0), (c, code, pcode)
        if code >= 0:
            assert pcode == code and pdec == dec, c
            n = sum(s[2] + (s[4] or 0) for s in S.parse(c.block))
            assert code == n, (c, code, n)


def test_every_block_decodes_as_the_reference_does(oracle, reference, cases):
    for c in cases:
        assert reference.decompress_block(c.block, c.cap) == oracle.decompress_block(c.block, c.cap), c


def _seqs(cases):
    """(case, token_pos, lit_len, offset, match_len, lit_end, match_end) of every sequence of every case"""
    for c in cases:
        for tp, ls, lit, off, ml, op in S.parse(c.block):
            yield c, tp, lit, off, ml, op + lit, op + lit + (ml or 0)


def test_families_reach_their_edges(cases):
    seqs = list(_seqs(cases))
    missing = []

    def need(what, ok):
        if not ok:
            missing.append(what)

    lits = {q[2] for q in seqs}
    mls = {q[4] for q in seqs if q[4]}
    for L in S.LIT_LENS:
        need("literal run of %d" % L, L in lits)
    for M in S.ML_LENS:
        need("match of %d" % M, M in mls)
    need("literal run of a few thousand", any(L >= 2000 for L in lits))
    need("match of tens of thousands", any(M >= 10000 for M in mls))
    for L, M in ((269, 273), (270, 274), (524, 528), (525, 529)):
        need("lit %d + match %d in one sequence" % (L, M), any(q[2] == L and q[4] == M for q in seqs))
    for off in S.SMALL_OFFSETS:
        need("offset %d overlapping its match" % off, any(q[3] == off and q[4] > off for q in seqs))
        for w in (4, 8, 16):
            need("offset %d with a match over %d bytes" % (off, w), any(q[3] == off and q[4] > max(off, w) for q in seqs))
    for off in S.RING_OFFSETS + S.SEGMENT_OFFSETS:
        need("offset %d" % off, any(q[3] == off and q[5] >= off for q in seqs))
    need("offset to the output's first byte", any(q[0].valid and q[3] and q[3] == q[5] and q[5] > 100 for q in seqs))
    need("offset one past the output's first byte", any(not q[0].valid and q[3] and q[3] == q[5] + 1 for q in seqs))
    for s in S.SHIFTS:
        for name, bs in S.OUT_EDGES.items():
            for B in bs:
                need("match end at %s %d %+d" % (name, B, s), any(q[4] and q[6] == B + s for q in seqs))
        need("literal end at 32 KiB %+d" % s, any(q[4] and q[2] and q[5] == S.CU_OUTMAX + s for q in seqs))
        for name, bs in S.IN_EDGES.items():
            for B in bs:
                need("token at %s %d %+d" % (name, B, s), any(q[1] == B + s for q in seqs))
        need("token at block end - 512 %+d" % s, any(q[1] == len(q[0].block) - S.CU_TAIL + s for q in seqs))
    # parse-adversarial: k disjoint speculative chains for k = 3..8, six tokens in a 16-byte chunk, more sequences in 32 KiB of
    # output than a segment has records
    for k in range(3, 9):
        need("self-similar period %d" % k, any(
            sum(1 for q in seqs if q[0] is c and q[3] == c.block[q[1]] * 257 and (q[4] - 4, q[2]) == (c.block[q[1]] & 15, k - 3)
                and c.block[q[1]:q[1] + k] == bytes([c.block[q[1]]]) * k) >= 2000 for c in cases))
    six = False
    for c in cases:
        toks = [q[1] // S.CU_CHUNK for q in seqs if q[0] is c]
        six = six or any(toks.count(t) >= 6 for t in set(toks[:3000]))
    need("six tokens in a 16-byte chunk", six)
    need("over 4096 sequences in 32 KiB of output", any(sum(1 for q in seqs if q[0] is c and q[5] < S.CU_OUTMAX) > 4096 for c in cases))
    # dependence: offset-1 runs across the segment and batch boundaries, chains of matches that copy the match in front of them
    need("offset-1 run across 32 KiB", any(q[3] == 1 and q[5] < S.CU_OUTMAX < q[6] for q in seqs))
    need("offset-1 run across a PAR_BATCH_OUT multiple",
         any(q[3] == 1 and q[5] // S.PAR_BATCH_OUT != (q[6] - 1) // S.PAR_BATCH_OUT for q in seqs))
    depth = 0
    for c in cases:
        run = 0
        for q in seqs:
            if q[0] is c:
                run = run + 1 if (q[2] == 0 and q[3] and q[3] == q[4]) else 0
                depth = max(depth, run)
    need("a chain of 2500 matches, each copying the one in front of it", depth >= 2500)
    # end rules and capacities
    caps = [c for c in cases if c.family == "caps"]
    for slack in S.CAP_SLACK:
        need("capacity n + %d" % slack, any(c.cap - sum(q[2] + (q[4] or 0) for q in S.parse(c.block)) == slack for c in caps))
    for n in (0, 64, 128, 256):
        need("a block shorter than %d" % (n + 1), any(sum(q[2] + (q[4] or 0) for q in S.parse(c.block)) < n + 1 for c in caps))
    ends = [c for c in cases if c.family == "ends"]
    for before in (11, 12, 13):
        need("last match %d before the end" % before, any(
            c.cap - (S.parse(c.block)[-2][5] + S.parse(c.block)[-2][2]) == before for c in ends if c.block[-1:] and _final(c)))
    for last in range(7):
        need("%d last literals" % last, any(_final(c) and S.parse(c.block)[-1][2] == last for c in ends))
    need("a block that ends with a match", any(not _final(c) for c in ends))
    need("offset 0", any(q[3] == 0 for q in seqs))
    assert not missing, missing


def _final(c):
    try:
        return S.parse(c.block)[-1][3] is None
    except ValueError:
        return False


def test_dictionary_family(oracle, dict_streams):
    """Linked: plain_decode with the same dictionary as the oracle's block-by-block decode (the last block that decoded); and the
    family reaches the dictionary's first byte, one byte before it, straddles its end by 1..16 bytes, and offsets near 65535
    with dictionaries shorter and longer than 64 KiB."""
    hit = set()
    for st in dict_streams:
        expect = S.linked_expect(oracle, st)
        d = b""
        for (name, blk, cap, valid), (code, dec) in zip(st, expect):
            assert (code >= 0) == valid, (name, code)
            pcode, pdec = S.plain_decode(blk, cap, d)
            assert pcode == code if code >= 0 else pcode < 0, (name, code, pcode)
            if code >= 0:
                assert pdec == dec, name
            dl = min(len(d), 65536)
            for tp, ls, lit, off, ml, op in S.parse(blk):
                if off is None:
                    continue
                src = op + lit - off
                if d and src == -dl:
                    hit.add("dictLen")
                if d and src == -dl - 1 and code < 0:
                    hit.add("dictLen + 1")
                if d and -16 <= src < 0 and src + ml > 0:
                    hit.add("straddle %d" % -src)
                if d and off >= 65000 and src < 0:
                    hit.add("near 65535, dictionary %s 64 KiB" % ("shorter than" if len(d) < 65536 else "of"))
            if code > 0:
                d = dec
    want = {"dictLen", "dictLen + 1", "near 65535, dictionary shorter than 64 KiB", "near 65535, dictionary of 64 KiB"}
    want |= {"straddle %d" % s for s in range(1, 17)}
    assert want <= hit, sorted(want - hit)


def test_dictionary_family_as_the_reference_decodes_it(oracle, reference, dict_streams):
    for st in dict_streams:
        d = None
        for name, blk, cap, valid in st:
            got = reference.decompress_block(blk, cap, d)
            assert got == oracle.decompress_block(blk, cap, d), name
            if got[0] > 0:
                d = got[1]


@pytest.mark.parametrize("stop_after", [None, 2 * S.SPARSE_STEP])
def test_sparse_dependence_stream(oracle, stop_after):
    """The path-6 stream: every block 1 MiB, compressible far below 15/16; the quad at every multiple of 65535 (up to stop_after)
    is the stream's first 4 bytes, non-zero, so that a block decoded against zeros differs there and nowhere else."""
    blocks = S.sparse_dependence_stream(stop_after=stop_after)
    quad = bytes([0x11, 0x22, 0x33, 0x44])
    d = None
    for i, blk in enumerate(blocks):
        assert 3072 <= len(blk) < S.BIG * 15 // 16
        code, dec = oracle.decompress_block(blk, S.BIG, d)
        assert code == S.BIG, (i, code)
        deps = [k * S.SPARSE_STEP for k in range(S.BIG // S.SPARSE_STEP + 1) if stop_after is None or k * S.SPARSE_STEP <= stop_after]
        if i == 0:
            assert all(dec[p:p + 4] == quad for p in deps)
        else:
            z_code, z = oracle.decompress_block(blk, S.BIG, bytes(65536))
            assert z_code == S.BIG
            diff = np.nonzero(np.frombuffer(z, np.uint8) != np.frombuffer(dec, np.uint8))[0].tolist()
            assert diff == [p + j for p in deps for j in range(4)], (i, diff[:8], deps[:8])
            if stop_after is None:
                assert all(dec[p:p + 4] == quad for p in deps)
        d = dec
