"""The strict block validator (tests/lz4_check.py) and the encoders' edge inputs (tests/encode_cases.py), pinned on the CPU:
the oracle's and the reference's own blocks pass every rule on every case, the flagged cases do give the oracle a match, and
the validator rejects hand-built violations by the right rule -- its negative control."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encode_cases as EC  # noqa: E402
import lz4_check as LC  # noqa: E402
import lz4_synth as LS  # noqa: E402

ACCELS = (1, 9, 65537)


@pytest.fixture(scope="module")
def cases():
    return EC.cases()


def test_case_list(cases):
    again = EC.cases()
    assert [tuple(c) for c in cases] == [tuple(c) for c in again], "the list differs between two calls"
    assert all(type(c.data) is bytes for c in cases)
    assert sum(len(c.data) for c in cases) <= EC.MAX_TOTAL
    assert {c.family for c in cases} == set(EC.FAMILIES)
    names = [(c.family, c.name) for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        if c.must_match:
            assert len(c.data) >= 64 and not c.name.startswith("distance"), c.name
    # what the families promise
    by = {f: [c for c in cases if c.family == f] for f in EC.FAMILIES}
    assert sorted({len(c.data) for c in by["lengths"]}) == sorted(EC.LENGTHS) and len(by["lengths"]) == 3 * len(EC.LENGTHS)
    assert len(by["ends"]) == 15 + 9 + 2 and len(by["codes"]) == len(EC.MATCH_CODES) + len(EC.LITERAL_CODES)
    assert [len(c.data) for c in by["incompressible"]] == [13, 64, 4096, 65536, 65537]
    assert sum(len(c.data) > 65536 for c in by["offsets"]) == 5      # only these need a block above 64 KiB
    for c in by["offsets"]:
        if c.name.startswith("distance"):
            d = int(c.name.split()[1])
            assert c.data[100:164] == c.data[100 + d:164 + d]
    for c in by["queue"]:
        if "match at" in c.name:
            n = len(c.data)
            assert c.data[n - 12:n - 5] == c.data[n - 3012:n - 3005] and c.data[n - 13] != c.data[n - 3013]


@pytest.mark.parametrize("accel", ACCELS)
def test_oracle_blocks_pass(oracle, cases, accel):
    for c in cases:
        try:
            LC.check_block(oracle.compress_block(c.data, accel), len(c.data))
        except AssertionError as e:
            raise AssertionError("%s/%s at acceleration %d: %s" % (c.family, c.name, accel, e))


@pytest.mark.parametrize("accel", ACCELS)
def test_reference_blocks_pass(reference, cases, accel):
    for c in cases:
        try:
            LC.check_block(reference.compress_block(c.data, accel), len(c.data))
        except AssertionError as e:
            raise AssertionError("%s/%s at acceleration %d: %s" % (c.family, c.name, accel, e))


def test_must_match_cases_match(oracle, cases):
    flagged = [c for c in cases if c.must_match]
    assert len(flagged) >= 100
    for c in flagged:
        assert LC.check_block(oracle.compress_block(c.data, 1), len(c.data))[0] >= 1, (c.family, c.name)


def test_codes_force_their_lengths(oracle, cases):
    """the oracle's parse of a `codes` case holds the length the case is named after: the brackets do force it"""
    for c in cases:
        if c.family != "codes":
            continue
        want = int(c.name.split()[-1])
        seqs = LS.parse(oracle.compress_block(c.data, 1))
        if c.name == "match of 4":             # five bytes are hashed: the reference has no matches of exactly 4 (why it has no flag)
            assert seqs[0][3] is None and not c.must_match
        elif c.name.startswith("match"):
            assert want in [s[4] for s in seqs], (c.name, [s[4] for s in seqs])
        else:
            assert want in [s[2] for s in seqs[1:-1]], (c.name, [s[2] for s in seqs])


def test_counts_and_dictionary():
    # 8 literals, a match of 8 at offset 12 (4 bytes into the dictionary), 2 literals, a match of 4 at offset 3, 12 literals
    blk = LS.write_block([(b"abcdefgh", 12, 8), (b"ij", 3, 4)], b"klmnopqrstuv")
    assert LC.check_block(blk, 34, dict_len=4) == (2, 12, 18, 1)
    assert LC.check_block(blk, 34, dict_len=70000) == (2, 12, 18, 1)
    with pytest.raises(LC.BlockRuleError) as e:
        LC.check_block(blk, 34, dict_len=3)
    assert e.value.rule == LC.OFFSET
    assert LC.check_block(b"\x00", 0) == (0, 0, -1, 0)
    assert LC.check_block(b"\x30abc", 3) == (0, 0, -1, 0)


VALID = LS.write_block([(b"abcdefgh", 4, 8)], b"ijklmnopqrst")        # 28 bytes; the last token is 13 bytes from the end


def _hand_built():
    lit8 = b"abcdefgh"
    low = bytearray(VALID)
    low[-13] |= 3
    return [
        ("offset 0", LS.write_block([(lit8, 0, 8)], b"x" * 12), 28, LC.OFFSET),
        ("offset one past the output start", LS.write_block([(lit8, 9, 8)], b"x" * 12), 28, LC.OFFSET),
        ("match start at n-11", LS.write_block([(lit8, 4, 4)], b"x" * 7), 19, LC.MATCH_START),
        ("4 last literals", LS.write_block([(lit8, 4, 8)], b"x" * 4), 20, LC.LAST_LITERALS),
        ("non-zero last low nibble", bytes(low), 28, LC.LAST_SEQUENCE),
        ("truncated by a byte", VALID[:-1], 28, LC.BOUNDS),
        ("a trailing byte", VALID + b"\x00", 28, LC.END),
        ("a match in 12 bytes", LS.write_block([(b"a", 1, 4)], b"x" * 7), 12, LC.SHORT),
        ("one byte over the bound", LS.write_block([], b"x" * 30)[:1] + b"\xff" * 20 + b"x" * 30, 30, LC.BOUND),
        ("the output one byte short", VALID, 29, LC.END),
        ("the output one byte long", VALID, 27, LC.END),
    ]


@pytest.mark.parametrize("name,block,n,rule", _hand_built(), ids=[h[0] for h in _hand_built()])
def test_rejects_hand_built(name, block, n, rule):
    LC.check_block(VALID, 28)
    with pytest.raises(LC.BlockRuleError) as e:
        LC.check_block(block, n)
    assert e.value.rule == rule, str(e.value)
    assert rule in str(e.value)


def test_rejects_invalid_synth_ends(oracle):
    """every invalid block of lz4_synth's family `ends`, by the rule it was written to break; the valid ones pass (offset 0
    decodes in the reference, which writes zeros for it, and is no block a compressor may write)"""
    ends = [c for c in LS.independent_cases() if c.family == "ends"]
    invalid = [c for c in ends if not c.valid]
    assert len(invalid) == 2 + 5 + 1
    for c in ends:
        if c.valid and not c.name.startswith("offset 0"):
            LC.check_block(c.block, c.cap)
            continue
        if c.name.startswith("offset 0"):
            rule = LC.OFFSET
        elif c.name.startswith("last match 11"):
            rule = LC.MATCH_START
        else:                                    # 0..4 last literals; a block that ends with a match has none either
            rule = LC.LAST_LITERALS
        with pytest.raises(LC.BlockRuleError) as e:
            LC.check_block(c.block, c.cap)
        assert e.value.rule == rule, (c.name, str(e.value))
