"""tests/golden/legacy_sessions.json -- the reference's LZ4_decompress_safe_continue / LZ4_compress_fast_continue call by call on
the sessions of tests/legacy_cases.py -- held against (1) the reference itself, where it is built, and (2) the oracle under the
session rule that the linked GPU kernels restate: the dictionary is the output of the last block that decoded to at least one
byte, a result <= 0 changes nothing.  No GPU."""
import pytest

import legacy_cases as LC

GROUPS = ("D1", "D2", "D3", "D4", "D5", "D6")


@pytest.fixture(scope="module")
def gold():
    return LC.load_golden()


@pytest.fixture(scope="module")
def sessions():
    return LC.decode_sessions()


def _compare(group, sessions, recs, run):
    assert [name for name, _ in sessions] == [r["session"] for r in recs], group
    for (name, steps), rec in zip(sessions, recs):
        got = LC.record(run(steps))
        for k, (step, _, cap) in enumerate(steps):
            assert (got["codes"][k], got["sha256"][k]) == (rec["codes"][k], rec["sha256"][k]), \
                "%s, step %d (%s, capacity %d): code %d, recorded %d" % (name, k, step, cap, got["codes"][k], rec["codes"][k])
        assert len(rec["codes"]) == len(steps), name


def test_fixture_covers_the_cases(gold, sessions):
    d = gold["decode"]
    assert gold["lz4_version"] == 10903 and sorted(d) == list(GROUPS)
    assert len(sessions["D1"]) == 264 and all(len(r["codes"]) == 1 for r in d["D1"])
    assert max(cap for _, steps in sessions["D1"] for _, _, cap in steps) == 93537
    assert [len(r["codes"]) for r in d["D2"]] == [266, 266] and [r["codes"][:2] for r in d["D2"]] == [[70000, 3000], [100, 3000]]
    # blocks that reach in front of their own start decode behind a dictionary, and do not without one
    alone = [r["codes"][0] for r in d["D1"]]
    assert any(a < 0 < b for a, b in zip(alone, d["D2"][0]["codes"][2:]))
    assert d["D5"][0]["codes"] == list(LC.SWING_SIZES)
    c4 = d["D4"][0]["codes"]
    assert [c > 0 for c in c4] == [True, False, True, False, True, False, False, True] and c4[3] == 0
    by_name = {r["session"]: r["codes"] for r in d["D6"]}
    assert by_name["D6 no dictionary, [0x00] capacity 0"] == [0] and by_name["D6 no dictionary, capacity 0"] == [-1]
    assert by_name["D6 no dictionary, srcSize 0 capacity 100"] == [-1] and by_name["D6 no dictionary, srcSize 0 capacity 0"] == [-1]
    assert by_name["D6 dictionary in force"][-7:] == [-2, -1, 0, 0, -1, -1, 3000]


@pytest.mark.parametrize("group", GROUPS)
def test_fixture_matches_the_reference(reference, gold, sessions, group):
    _compare(group, sessions[group], gold["decode"][group], lambda steps: reference.decode_session([(b, c) for _, b, c in steps]))


@pytest.mark.parametrize("group", GROUPS)
def test_oracle_session_model_matches_the_fixture(oracle, gold, sessions, group):
    _compare(group, sessions[group], gold["decode"][group], lambda steps: LC.model_session(oracle, steps))


def test_compress_fixture_matches_the_reference(reference, oracle, gold):
    cases = LC.c1_sessions(oracle)
    assert [name for name, _, _ in cases] == [r["session"] for r in gold["compress"]["C1"]]
    for (name, steps, forced), rec in zip(cases, gold["compress"]["C1"]):
        got = LC.record(reference.compress_session([(data, n, cap, accel) for _, data, n, cap, accel in steps]))
        if forced:
            assert (got["codes"], got["sha256"]) == (rec["codes"], rec["sha256"]), name
        else:
            assert [c > 0 for c in got["codes"]] == rec["positive"] and all(rec["positive"]), name


def test_forced_compress_outcomes(oracle, gold):
    """what C1 is about, read from the record: an empty input is one zero byte, or 0 without room for it; incompressible input in a
    buffer of its own size, a negative size and one past LZ4_MAX_INPUT_SIZE return 0"""
    recs = {r["session"]: r for r in gold["compress"]["C1"]}
    assert recs["C1 srcSize 0, capacity 1"]["codes"] == [1] and recs["C1 srcSize 0, capacity 1"]["sha256"] == [LC.sha(b"\x00")]
    for name in ("C1 srcSize 0, capacity 0", "C1 4096 random bytes, capacity = srcSize", "C1 70000 random bytes, capacity = srcSize",
                 "C1 srcSize -1", "C1 srcSize LZ4_MAX_INPUT_SIZE + 1"):
        assert recs[name]["codes"] == [0], name
