"""Writes tests/golden/legacy_sessions.json: what the REAL reference functions (oracle/_ref, oracle/ref_harness.c's session
runners) return, call by call, on the sessions of tests/legacy_cases.py.  Run where the reference is built:

    python tests/golden/make_legacy_golden.py

Data only: per session the return code of every step and the sha256 of the bytes of every step that returned more than 0.  No
block and no input is stored: legacy_cases.py rebuilds them.  Running it again leaves the file byte-identical.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import legacy_cases as LC  # noqa: E402
from oracle.oracle import Oracle, Reference  # noqa: E402


def build(O, R):
    gold = {"lz4_version": R.version(), "decode": {}, "compress": {}}
    for group, sessions in LC.decode_sessions().items():
        recs = []
        for name, steps in sessions:
            rec = LC.record(R.decode_session([(blk, cap) for _, blk, cap in steps]))
            rec["session"] = name
            recs.append(rec)
        gold["decode"][group] = recs
    # what the sessions are for, checked where they are recorded
    d = gold["decode"]
    assert sum(len(r["codes"]) for r in d["D1"]) == 264
    assert [r["codes"] for r in d["D5"]] == [list(LC.SWING_SIZES)], d["D5"]
    c4 = d["D4"][0]["codes"]
    assert [c4[0], c4[2], c4[3], c4[4], c4[7]] == [5000, 4000, 0, 3000, 3500] and max(c4[1], c4[5], c4[6]) < 0, c4
    recs = []
    for name, steps, forced in LC.c1_sessions(O):
        rec = LC.record(R.compress_session([(data, n, cap, accel) for _, data, n, cap, accel in steps]))
        rec["session"], rec["forced"] = name, forced
        if not forced:                                   # the reference's sizes and bytes are its own: only that it succeeded
            assert all(c > 0 for c in rec["codes"]), (name, rec["codes"])
            rec = {"session": name, "forced": False, "positive": [c > 0 for c in rec["codes"]]}
        recs.append(rec)
    gold["compress"]["C1"] = recs
    return gold


def main():
    O, R = Oracle(), Reference()
    assert R.version() == 10903, R.version()
    gold = build(O, R)
    with open(LC.GOLDEN, "w") as f:
        f.write(json.dumps(gold, separators=(",", ":")).replace('{"codes"', '\n{"codes"').replace('{"session"', '\n{"session"') + "\n")   # a session a line
    steps = sum(len(r["codes"]) for g in gold["decode"].values() for r in g)
    print("wrote %s: %d decode sessions, %d steps, %d compress sessions"
          % (os.path.relpath(LC.GOLDEN, ROOT), sum(len(g) for g in gold["decode"].values()), steps, len(gold["compress"]["C1"])))


if __name__ == "__main__":
    main()
