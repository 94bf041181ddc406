#!/usr/bin/env python3
"""Host-side model of decode_par.hpp's batch loop: what a choice of PAR_HIST / PAR_RING / PAR_BATCH_OUT does to the batches, the
slides and the far matches of a block, without a GPU.  Oracle only: blocks of the `lzsynth` generator compressed by the oracle.

The model has decode_block_par's acceptance rules (a token among the window's candidates, one extension byte each way, the sequence
inside the window, the batch's output cap, the source in the ring or already flushed), its slide rule, its far test, the adaptive
nodes per lane and the hand-over of one sequence to the sequential decoder.  It does not model time.

    python scripts/par_ring_model.py [--blocks 64] [--kind lzsynth] [HIST/RING/BATCH_OUT ...]
"""
import argparse
import bisect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle import Oracle  # noqa: E402

WAVE, WIN = 64, 832


def parse(blk):
    """[(position, literals, offset, match length, compressed bytes, plain)]; the last, literal-only sequence is left out"""
    seqs, p, n = [], 0, len(blk)
    while p < n:
        s, t = p, blk[p]
        p += 1
        lit, ext = t >> 4, 0
        if lit == 15:
            while True:
                b = blk[p]; p += 1; lit += b; ext += 1
                if b != 255: break
        lext = ext
        p += lit
        if p >= n: break
        off = blk[p] | (blk[p + 1] << 8)
        p += 2
        ml, ext = (t & 15), 0
        if ml == 15:
            while True:
                b = blk[p]; p += 1; ml += b; ext += 1
                if b != 255: break
        plain = lext <= 1 and ext <= 1 and off != 0 and not (lext == 1 and lit == 15 + 255) and not (ext == 1 and ml == 15 + 255)
        seqs.append((s, lit, off, ml + 4, p - s, plain))
    return seqs


def model(blk, cap, hist, ring, batch_out, align=0, data_align=8):
    seqs = parse(blk)
    at = {s[0]: i for i, s in enumerate(seqs)}
    iend = len(blk)
    ip = op = ring_base = flushed = 0
    nl = 8
    st = dict(batches=0, seqs=0, slides=0, far=0, handovers=0, waiting=0)
    while iend - ip >= 64 and cap - op >= 128:
        wofs = (data_align + ip) & 15
        in_lim = min(iend - (ip - wofs) - 32, WIN)
        node_lim = min(in_lim, nl * WAVE - 1)
        i = at.get(ip)
        taken, out, o, depth_of, far = [], 0, op, [], 0
        while i is not None and i < len(seqs) and len(taken) < WAVE:
            s, lit, off, ml, size, plain = seqs[i]
            c = wofs + (s - ip)
            spos = o + lit - off
            if not (plain and c <= node_lim and c + size <= in_lim and out + lit + ml <= batch_out and o + lit + ml + 64 < cap
                    and spos >= 0 and (spos >= ring_base or spos + ml <= flushed)):
                break
            taken.append((o, lit, ml, spos))
            out += lit + ml
            o += lit + ml
            i += 1
        if not taken:
            # one sequence through the sequential decoder, then the ring's history is loaded again
            st["handovers"] += 1
            i = at.get(ip)
            if i is None or i >= len(seqs): break
            s, lit, off, ml, size, plain = seqs[i]
            ip, op = s + size, op + lit + ml
            ring_base = ((op - hist) & ~15) if op > hist else 0
            flushed = op
            continue
        # dependency depth of the near matches (a match is ready when every sequence of the batch its source overlaps is complete)
        starts = [t[0] for t in taken]
        for k, (o0, lit, ml, spos) in enumerate(taken):
            if spos < ring_base:
                far += 1; depth_of.append(0); continue
            hi = min(spos + ml, o0)
            d = 0
            if hi > op and hi > spos:
                jlo = bisect.bisect_right(starts, max(spos, op)) - 1
                jhi = bisect.bisect_right(starts, hi - 1) - 1
                for j in range(max(jlo, 0), min(jhi, k - 1) + 1):
                    d = max(d, depth_of[j])
            depth_of.append(d + 1)
        st["batches"] += 1
        st["seqs"] += len(taken)
        st["far"] += far
        st["waiting"] += sum(1 for d in depth_of if d > 2)
        nxt = seqs[i - 1][0] + seqs[i - 1][4]
        if len(taken) >= 16:
            nl = 6 if (nxt - ip) * WAVE <= 416 * len(taken) else 8
        elif nl == 6:
            nl = 8
        ip, op = nxt, o
        flushed = max(flushed, op - ((align + op) & 63))
        if op - ring_base + align + batch_out + 32 > ring:
            st["slides"] += 1
            ring_base = (op - hist) & ~15
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--kind", default="lzsynth")
    ap.add_argument("settings", nargs="*", default=["2000/5728/2048", "2000/5504/2048", "1888/5504/2048", "1776/5504/2048", "1776/5504/1792"])
    a = ap.parse_args()
    O = Oracle()
    bl = 65536
    raw = O.gen(a.kind, a.blocks, bl).tobytes()
    blocks = [O.compress_block(raw[i * bl:(i + 1) * bl]) for i in range(a.blocks)]
    print("| HIST / RING / BATCH_OUT | batches per block | sequences per batch | slides per block | far lanes per batch | waiting after two rounds | hand-overs per block |")
    print("|---|---|---|---|---|---|---|")
    for s in a.settings:
        hist, ring, bout = (int(x) for x in s.split("/"))
        if hist + 30 + bout + 32 > ring:
            print("| %s | a batch does not fit the ring after a slide | | | | | |" % s.replace("/", " / "))
            continue
        tot = dict(batches=0, seqs=0, slides=0, far=0, handovers=0, waiting=0)
        for b in blocks:
            for k, v in model(bytes(b), bl, hist, ring, bout).items():
                tot[k] += v
        n, nb = float(a.blocks), float(max(tot["batches"], 1))
        print("| %s | %.1f | %.1f | %.1f | %.2f | %.2f | %.2f |" % (s.replace("/", " / "), tot["batches"] / n, tot["seqs"] / nb, tot["slides"] / n,
                                                                   tot["far"] / nb, tot["waiting"] / nb, tot["handovers"] / n))


if __name__ == "__main__":
    main()
