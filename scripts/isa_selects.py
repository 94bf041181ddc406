#!/usr/bin/env python3
"""Development aid: the v_cndmask_b32 of one kernel's batch loop, basic block by basic block.
usage: isa_selects.py kernels.s <mangled-kernel-name>
(kernels.s from: hipcc -O3 -std=c++17 --offload-arch=gfx950 -gline-tables-only -S --cuda-device-only)

The batch loop is the largest backward-branch span of the function that holds no call, as in
profiles/par_pairs_kernel_resources.txt.  For every basic block inside it with a select: the selects by form (e32 on vcc,
e64 on an SGPR pair), what stands in front of each (the v_cmp that writes its condition, another select, anything else), the
longest run of selects, and the source lines they come from.  Then the loop's totals, its scratch instructions and its
spill-lane traffic.  scripts/micro/valu_rate.hip prices the placements (profiles/par_sel_valu_rate.txt): only a run of more
than four e32 selects on vcc is expensive."""
import collections
import re
import sys

path, fn = sys.argv[1], sys.argv[2]
ins = []            # (op, text, source line, label or None)
inside = False
loc = 0
pending = None
for line in open(path, errors="replace"):
    if line.startswith(fn + ":"):
        inside = True
        continue
    if not inside:
        continue
    if line.startswith(".Lfunc_end"):
        break
    s = line.strip()
    m = re.match(r"\.loc\s+\d+\s+(\d+)", s)
    if m:
        loc = int(m.group(1))
        continue
    m = re.match(r"^(\.LBB\d+_\d+):", s)
    if m:
        pending = m.group(1)
        continue
    if not s or s.startswith((".", ";")) or s.endswith(":"):
        continue
    ins.append((s.split()[0], s, loc, pending))
    pending = None

label_at = {lab: i for i, (_, _, _, lab) in enumerate(ins) if lab}
calls = [i for i, (op, _, _, _) in enumerate(ins) if op.startswith("s_swappc")]
best = None
for i, (op, s, _, _) in enumerate(ins):
    if op.startswith("s_cbranch") or op == "s_branch":
        t = label_at.get(s.split()[-1])
        if t is not None and t < i and not any(t <= c <= i for c in calls):
            if best is None or i - t > best[1] - best[0]:
                best = (t, i)
lo, hi = best
print("%s\nbatch loop %s: instructions %d..%d of %d (%d in the loop)" % (fn, ins[lo][3], lo, hi, len(ins), hi - lo + 1))

def form(op):
    return "e32" if op.endswith("_e32") else "e64"

tot = collections.Counter()
front = collections.Counter()
runs = collections.Counter()
block = None
rows = []
for i in range(lo, hi + 1):
    op, s, ln, lab = ins[i]
    if lab or block is None or ins[i - 1][0].startswith(("s_cbranch", "s_branch")):
        block = {"name": lab or ("(%d)" % i), "n": 0, "sel": collections.Counter(), "front": collections.Counter(), "run": 0, "lines": collections.Counter()}
        rows.append(block)
        run = 0
    block["n"] += 1
    if op.startswith("v_cndmask"):
        run += 1
        block["run"] = max(block["run"], run)
        f = form(op)
        block["sel"][f] += 1
        tot[f] += 1
        block["lines"][ln] += 1
        j = i - 1
        while j > lo and ins[j][0] in ("s_nop", "s_waitcnt"):
            j -= 1
        p = ins[j][0]
        k = "select" if p.startswith("v_cndmask") else "its v_cmp" if p.startswith("v_cmp") else "other"
        block["front"][k] += 1
        front[k] += 1
    else:
        if run:
            runs[run] += 1
        run = 0
print("%-12s %5s  %4s %4s  %-34s %3s  %s" % ("block", "insts", "e32", "e64", "in front: v_cmp / select / other", "run", "source lines (count)"))
for b in rows:
    if not b["sel"]:
        continue
    print("%-12s %5d  %4d %4d  %10d / %6d / %5d %12d  %s" % (b["name"], b["n"], b["sel"]["e32"], b["sel"]["e64"], b["front"]["its v_cmp"],
          b["front"]["select"], b["front"]["other"], b["run"], " ".join("%d(%d)" % kv for kv in sorted(b["lines"].items()))))
kinds = collections.Counter()
for i in range(lo, hi + 1):
    op = ins[i][0]
    kinds["valu" if op.startswith("v_") else "salu" if op.startswith("s_") else "lds" if op.startswith("ds_")
          else "vmem" if op.startswith(("global_", "flat_", "buffer_", "scratch_")) else "other"] += 1
print("loop mix: %s" % dict(kinds))
print("selects in the loop: %d e32 on vcc, %d e64; in front of them: %s" % (tot["e32"], tot["e64"], dict(front)))
print("runs of selects by length: %s" % dict(sorted(runs.items())))
print("scratch instructions in the loop: %d" % sum(1 for i in range(lo, hi + 1) if ins[i][0].startswith("scratch_")))
print("spill lanes in the loop: %d v_writelane_b32, %d v_readlane_b32" % (
    sum(1 for i in range(lo, hi + 1) if ins[i][0] == "v_writelane_b32"), sum(1 for i in range(lo, hi + 1) if ins[i][0] == "v_readlane_b32")))
