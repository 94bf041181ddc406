"""The hand-built LZ4 blocks of tests/lz4_synth.py, on the host: the writer writes what the format says (plain_decode, the
oracle and the reference agree on every block, code and bytes), and every family still reaches the edges it names -- recomputed
from the written blocks, so that an edit of the generator cannot quietly lose coverage.  The same for the two sets aimed at the
decoders' dictionary form: the blocks cut at a sequence boundary (seam_cuts) and the probes on the dictionary's edges
(seam_family).

What the two sets held when they were written: 1212 cuts from the 225 cases with a match (1167 valid; 45 of the 11 invalid
cases stay invalid behind the cut), with 1297 matches that straddle the seam and 711 inside the dictionary that end less than
16 bytes before its end; 3022 probe blocks of at most 2063 compressed bytes.  plain_decode, the oracle and the reference agreed
on every one of them, code and bytes."""
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


# ---- the dictionary form: blocks cut at a sequence boundary, probes on the dictionary's edges ------------------------------------

@pytest.fixture(scope="module")
def cuts():
    return S.seam_cuts()


@pytest.fixture(scope="module")
def seam():
    return S.seam_family()


def _dict_matches(block, dict_len):
    """(sequence index, offset, match_len, spos, out_pos, match_end) of every match of a block that starts in front of its first
    output byte; spos = its source relative to that byte, out_pos = where its sequence starts in the output"""
    for i, (tp, ls, lit, off, ml, op) in enumerate(S.parse(block)):
        if off is not None and off > op + lit:
            yield i, off, ml, op + lit - off, op, op + lit + ml


def test_seam_cuts_decode_as_written(oracle, cases, cuts):
    """Every cut: plain_decode and the oracle agree on code and bytes, validity is as written, and the suffix of a valid case
    behind the boundary at k, with the case's first k bytes as its dictionary, decodes to the rest of the case."""
    whole = {"%s/%s" % (c.family, c.name): (c, oracle.decompress_block(c.block, c.cap)) for c in cases}
    assert len(whole) == len(cases)                          # (the names tell the cases apart)
    for name, d, blk, cap, valid in cuts:
        code, dec = oracle.decompress_block(blk, cap, d)
        assert (code >= 0) == valid, (name, code)
        pcode, pdec = S.plain_decode(blk, cap, d)
        assert pcode == code if code >= 0 else pcode < 0, (name, code, pcode)
        base, k = name.rsplit(" @", 1)
        k = int(k)
        c, (wcode, wdec) = whole[base]
        assert len(d) == k and cap == c.cap - k, name
        if code >= 0:
            assert pdec == dec, name
        if wcode >= 0:
            assert valid and d == wdec[:k] and (code, dec) == (wcode - k, wdec[k:]), (name, code, wcode)


def test_seam_cuts_decode_as_the_reference_does(oracle, reference, cuts):
    for name, d, blk, cap, valid in cuts:
        assert reference.decompress_block(blk, cap, d) == oracle.decompress_block(blk, cap, d), name


def test_seam_cuts_cover_the_cases(cases, cuts):
    """Every valid case with a match is cut at three places at least; only the cases without a match yield nothing; and the set
    holds what it is for: matches that straddle the seam and matches inside the dictionary's last 16 bytes, in numbers."""
    per = {}
    for name, d, blk, cap, valid in cuts:
        per.setdefault(name.rsplit(" @", 1)[0], set()).add(len(d))
    none = 0
    for c in cases:
        n = len(per.get("%s/%s" % (c.family, c.name), ()))
        has_match = any(q[3] is not None for q in S.parse(c.block))
        none += n == 0
        assert n > 0 or not has_match, c
        assert n >= 3 or not (c.valid and has_match), (c, n)
    assert none <= 39, none
    straddle = near_end = first = plain = 0
    for name, d, blk, cap, valid in cuts:
        if not valid:
            continue
        for i, off, ml, spos, op, end in _dict_matches(blk, len(d)):
            straddle += spos + ml > 0
            near_end += spos + ml <= 0 and -(spos + ml) < 16
            first += spos == -len(d)
            plain += spos + ml <= 0
    assert straddle >= 1000 and near_end >= 150 and first >= 20 and plain >= 20000, (straddle, near_end, first, plain)


def test_seam_family_decodes_as_written(oracle, seam):
    assert 2500 < len(seam) < 4100
    assert max(len(blk) for _, _, blk, _, _ in seam) <= 16384
    assert {dl for _, dl, _, _, _ in seam} == set(S.SEAM_DICT_LENS)
    for name, dl, blk, cap, valid in seam:
        d = S.seam_dictionary(dl)
        code, dec = oracle.decompress_block(blk, cap, d)
        assert (code >= 0) == valid, (name, code)
        pcode, pdec = S.plain_decode(blk, cap, d)
        assert pcode == code if code >= 0 else pcode < 0, (name, code, pcode)
        if code >= 0:
            assert code == cap and pdec == dec, name


def test_seam_family_decodes_as_the_reference_does(oracle, reference, seam):
    for name, dl, blk, cap, valid in seam:
        d = S.seam_dictionary(dl)
        assert reference.decompress_block(blk, cap, d) == oracle.decompress_block(blk, cap, d), name


def test_seam_family_reaches_its_edges(seam):
    """Recomputed from the written blocks: every end gap e with every copy width, every straddle, the dictionary's first byte
    and the byte in front of it, and every place -- each shown by the one match of a block that starts in the dictionary."""
    hit = set()
    for name, dl, blk, cap, valid in seam:
        probes = list(_dict_matches(blk, dl))
        assert len(probes) == 1, name                        # (everything else in the block is self-contained)
        i, off, ml, spos, op, end = probes[0]
        reach = min(dl, 65535)
        n_matches = sum(1 for q in S.parse(blk) if q[3] is not None)
        if spos == -dl - 1 and not valid:
            hit.add("one in front")
            hit.add("one in front at %s" % ("index 0" if i == 0 else "depth %d" % op))
            continue
        assert valid and spos >= -reach, name
        if spos + ml <= 0:
            e = -(spos + ml)
            cls = "4..7" if ml < 8 else "8..15" if ml < 16 else "16" if ml == 16 else "17..32" if ml <= 32 else "above 32"
            hit.add("e %d, ml %s" % (e, cls))
            what = "inside e %d" % e
        else:
            hit.add("straddle %d" % -spos)
            if off < ml:
                hit.add("straddle with offset < ml")
            what = "straddle %d" % -spos
        if spos == -reach:
            hit.add("first byte, dictionary %s 65535" % ("shorter than" if dl < 65535 else "of" if dl == 65535 else "longer than"))
        hit.add("index %d" % i)
        hit.add("depth %d" % op)
        hit.add("end %d" % (cap - end))
        if n_matches == 1:
            hit.add("cap %d" % cap)
            if len(blk) < 64:
                hit.add("short input")
        for place in ["index %d" % i, "depth %d" % op, "end %d" % (cap - end)] + \
                     (["cap %d" % cap] if n_matches == 1 else []):
            hit.add("%s at %s" % (what, place))
    want = {"e %d, ml %s" % (e, cls) for e in S.SEAM_GAPS for cls in ("4..7", "8..15", "16", "17..32", "above 32")}
    want |= {"straddle %d" % s for s in S.SEAM_STRADDLES} | {"straddle with offset < ml", "one in front", "short input"}
    want |= {"first byte, dictionary %s 65535" % w for w in ("shorter than", "of", "longer than")}
    want |= {"index %d" % i for i in S.SEAM_INDICES} | {"depth %d" % p for p in S.SEAM_DEPTHS}
    want |= {"end %d" % p for p in S.SEAM_END_DISTANCES} | {"cap %d" % c for c in S.SEAM_TINY_CAPS}
    # index 0 and the depths see every end gap and every straddle; every other place the three copy widths' worth of
    # e in {0, 15, 16} and s in {1, 15, 16}
    for place in ["index 0"] + ["depth %d" % p for p in S.SEAM_DEPTHS]:
        want |= {"inside e %d at %s" % (e, place) for e in S.SEAM_GAPS} | {"straddle %d at %s" % (s, place) for s in S.SEAM_STRADDLES}
        want.add("one in front at %s" % place)
    for place in ["index %d" % i for i in S.SEAM_INDICES[1:]] + ["end %d" % p for p in S.SEAM_END_DISTANCES] + \
                 ["cap %d" % c for c in S.SEAM_TINY_CAPS[2:]]:
        want |= {"inside e %d at %s" % (e, place) for e in (0, 15, 16)} | {"straddle %d at %s" % (s, place) for s in (1, 15, 16)}
    # (a straddle of 15 bytes is a match of 16 at least: with the 5 last literals it does not fit 13 or 20 bytes; nor does the
    # 8-byte match with its 1 literal fit 13)
    want |= {"inside e 0 at cap 13", "inside e 16 at cap 13", "straddle 1 at cap 13"}
    want |= {"inside e 0 at cap 20", "inside e 15 at cap 20", "inside e 16 at cap 20", "straddle 1 at cap 20"}
    assert want <= hit, sorted(want - hit)
