#!/usr/bin/env python3
"""Development aid: the rows of profiles/cframes_kernel_resources.txt, and the check that goes with them.  Compiles device
translation units for gfx950 with hipcc's resource-usage remarks, as scripts/hstreams_resources.py does.  No GPU is needed.

    scripts/cframes_resources.py [TREE]             one row per kernel of TREE's kernels_cframes.hip
    scripts/cframes_resources.py --compare A B      every kernel of kernels.hip and kernels_hstreams.hip in the trees A and B:
                                                    says whether all their remarks are the same, and lists the ones that differ

(TREE, A, B: checkouts of this repository; TREE defaults to this one.)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hstreams_resources import FIELDS, remarks  # noqa: E402


def row(name, r):
    return "%-72s %s" % (name, " ".join("%s %*s" % (tag, w, r.get(key, "?")) for tag, key, w in FIELDS))


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":
        a, b = os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3])
        bad = 0
        for unit in ("kernels.hip", "kernels_hstreams.hip"):
            ra, rb = remarks(a, unit), remarks(b, unit)
            diff = sorted(k for k in set(ra) | set(rb) if ra.get(k) != rb.get(k))
            print("%s: %d kernels in A, %d in B, %d differ" % (unit, len(ra), len(rb), len(diff)))
            for k in diff:
                print("  A " + row(k, ra.get(k, {})))
                print("  B " + row(k, rb.get(k, {})))
            bad += len(diff)
        sys.exit(1 if bad else 0)
    tree = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else here
    for name, r in sorted(remarks(tree, "kernels_cframes.hip").items()):
        print(row(name, r))


if __name__ == "__main__":
    main()
