#!/usr/bin/env python3
"""Host-side model of the LDS bank conflicts of decode_par.hpp's squaring rounds (parse_square): what the assignment of the window's
nodes to lanes does to the gathers from the successor table.  Oracle only: blocks of the generators compressed by the oracle, cut
into batches by par_ring_model.py's rules; needs no GPU.

Per batch the successor table is built from the window's bytes the way the speculative parse builds it, and the three squaring
rounds are followed with the table's real contents: gather j of a round reads, in lane l, the 16-bit entry at byte 2 * J of jump[],
J being the current successor of the j-th node lane l owns.  Banking as MI355X's ds_read_b32 (scripts/micro/lds_u16_banks.hip:
ds_read_u16 is banked the same): lanes 0-31 and 32-63 are served one after the other, bank = (byte address / 4) % 32, the same
dword is read once for all its lanes, and a group takes one cycle per distinct dword on its busiest bank.  Two cycles per gather
are the floor.  jump[] starts on a 16-byte boundary (PAR_JUMP_OFS), so its bank offset is 0 or a multiple of four banks, which does
not change a count.

Ownerships:  rows   lane l owns nodes NL * l .. NL * l + NL - 1 (up to docs/MEASUREMENT_LOG.md 20)
             pairs  lane l owns nodes 128p + 2l, 128p + 2l + 1 for p < NL / 2 (shipped)
             single lane l owns nodes 64j + l (conflict-free at best, but its table stores are 16-bit)

    python scripts/par_bank_model.py [--blocks 3] [--kinds lzsynth,text]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from oracle.oracle import Oracle  # noqa: E402
from par_ring_model import parse, WAVE, WIN  # noqa: E402

HIST, RING, BATCH_OUT, ROUNDS = 1500, 5088, 1856, 3
OWNERS = {
    "rows": lambda nl, l, j: nl * l + j,
    "pairs": lambda nl, l, j: 128 * (j >> 1) + 2 * l + (j & 1),
    "single": lambda nl, l, j: 64 * j + l,
}


def batches(blk, cap, data_align=8):
    """(ip, wofs, nodes per lane, inLim) of every batch of the block: par_ring_model.model's loop, which see"""
    seqs = parse(blk)
    at = {s[0]: i for i, s in enumerate(seqs)}
    iend = len(blk)
    ip = op = ring_base = flushed = 0
    nl = 8
    while iend - ip >= 64 and cap - op >= 128:
        wofs = (data_align + ip) & 15
        in_lim = min(iend - (ip - wofs) - 32, WIN)
        node_lim = min(in_lim, nl * WAVE - 1)
        i = at.get(ip)
        n, out, o = 0, 0, op
        while i is not None and i < len(seqs) and n < WAVE:
            s, lit, off, ml, size, plain = seqs[i]
            c = wofs + (s - ip)
            spos = o + lit - off
            if not (plain and c <= node_lim and c + size <= in_lim and out + lit + ml <= BATCH_OUT and o + lit + ml + 64 < cap
                    and spos >= 0 and (spos >= ring_base or spos + ml <= flushed)):
                break
            out += lit + ml
            o += lit + ml
            n += 1
            i += 1
        yield ip, wofs, nl, in_lim
        if n == 0:
            i = at.get(ip)
            if i is None or i >= len(seqs):
                break
            s, lit, off, ml, size, plain = seqs[i]
            ip, op = s + size, op + lit + ml
            ring_base = ((op - HIST) & ~15) if op > HIST else 0
            flushed = op
            continue
        nxt = seqs[i - 1][0] + seqs[i - 1][4]
        if n >= 16:
            nl = 6 if (nxt - ip) * WAVE <= 416 * n else 8
        elif nl == 6:
            nl = 8
        ip, op = nxt, o
        flushed = max(flushed, op - (op & 63))
        if op - ring_base + BATCH_OUT + 32 > RING:
            ring_base = (op - HIST) & ~15


def successor_table(blk, ip, wofs, nl, in_lim, header):
    """jump[] of the batch in nodes (the kernel stores 2 x node): nl * 64 entries and the absorbing one behind them"""
    base = ip - wofs

    def byte(c):
        p = base + c
        if p < 0:
            return header[p] if p >= -len(header) else 0
        return blk[p] if p < len(blk) else 0
    nodes = nl * WAVE
    absorb = min(max(in_lim, 0), nodes - 1) + 1
    jump = []
    for n in range(nodes):
        t = byte(n)
        lit0 = t >> 4
        term = 16 + byte(n + 1) if lit0 == 15 else lit0
        jump.append(min(n + 3 + term + ((t & 15) == 15), absorb))
    jump.append(nodes)
    return jump


def gather_cycles(addrs):
    """LDS cycles of one gather: addrs = the 64 lanes' byte addresses"""
    cyc = 0
    for half in (addrs[:32], addrs[32:]):
        per_bank = {}
        for a in half:
            per_bank.setdefault((a >> 2) & 31, set()).add(a >> 2)
        cyc += max(len(v) for v in per_bank.values())
    return cyc


def batch_cycles(jump, nl, owner):
    """(cycles, gathers) of the batch's squaring rounds with the given ownership"""
    cyc = 0
    cur = list(jump)
    for _ in range(ROUNDS):
        for j in range(nl):
            cyc += gather_cycles([2 * cur[owner(nl, l, j)] for l in range(WAVE)])
        cur = [cur[cur[n]] for n in range(len(cur))]
    return cyc, ROUNDS * nl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--kinds", default="lzsynth,text")
    a = ap.parse_args()
    O = Oracle()
    bl = 65536
    print("# blocks 0 .. %d of each generator, every batch's window, the three squaring rounds' gathers; LDS cycles" % (a.blocks - 1))
    print("| stream | nodes per lane | ownership | batches | cycles per gather | gathers per batch | cycles per batch | floor per batch |")
    print("|---|---|---|---|---|---|---|---|")
    for kind in a.kinds.split(","):
        raw = O.gen(kind, a.blocks, bl).tobytes()
        tabs = []
        for i in range(a.blocks):
            blk = bytes(O.compress_block(raw[i * bl:(i + 1) * bl]))
            header = len(blk).to_bytes(4, "little") + bl.to_bytes(4, "little")
            for ip, wofs, nl, in_lim in batches(blk, bl):
                tabs.append((successor_table(blk, ip, wofs, nl, in_lim, header), nl))
        for form in (None, 6, 8):
            sel = [t for t in tabs if form is None or t[1] == form]
            if not sel:
                continue
            for name, owner in OWNERS.items():
                cyc = gat = 0
                for jump, nl in sel:
                    c, g = batch_cycles(jump, nl, owner)
                    cyc += c
                    gat += g
                nb = float(len(sel))
                print("| %s | %s | %s | %d | %.2f | %.1f | %.1f | %.1f |" % (kind, "all" if form is None else form, name, len(sel), cyc / float(gat), gat / nb,
                                                                       cyc / nb, 2 * gat / nb))


if __name__ == "__main__":
    main()
