"""Placement: the regions of a device call laid out in any order and at any distance, beyond 4 GiB too.

include/mi355lz4.h asks for no order among blockOff[], outOff[], srcOff[] and the slots, and all of them are 64-bit.  place()
gives a call's regions four layouts ("dense", "permuted", "far", "far_permuted") inside one FAR BUFFER: an allocation of
2^31 + 2^32 + 2^27 bytes of which the call is handed the view that starts 2^31 bytes in.  The front pad is there so that an
offset truncated to 32 bits -- zero- or sign-extended -- still lands inside the allocation: aliases(x) says where.  A bug then
shows as a failed assertion, not as a GPU fault.

  * Windows guards the outputs without touching 6 GiB: guarded.pattern lies in a window of at least guarded.END_GUARD bytes on
    both sides of every output region and in an equal window at every alias of the region; after the call every byte of
    those windows outside the regions must still hold it.
  * put_inputs stores the inputs, and at every alias of an input OTHER VALID INPUT of another length (a decoy): a truncated
    read gives wrong bytes or a wrong size, never the right answer by luck.

All offsets are relative to the view (so the front pad is [-half, 0)).  Space(bits) scales the marks: bits = 32 is the far
buffer, tests/test_placement.py runs the same arithmetic on numpy buffers with bits = 24.

Test infrastructure only (imported by tests, like guarded.py).  Nothing GPU-related is loaded at import."""
import numpy as np

import guarded as G

MODES = ("dense", "permuted", "far", "far_permuted")
MIN_FREE = 40 << 30            # a GPU test that uses far buffers skips below this much free device memory


class Space:
    """The far buffer's geometry: `half` bytes of front pad, then the view of full + tail bytes.  bits = 32: the marks are
    2^31 and 2^32 and the tail is 2^27 bytes."""

    def __init__(self, bits=32, front=None):
        self.bits = int(bits)
        self.half, self.full, self.tail = 1 << (bits - 1), 1 << bits, 1 << (bits - 5)
        self.total = self.half + self.full + self.tail
        # The view starts here in the allocation.  A smaller front pad (a longer view) is for the calls whose fixed strides
        # need more than 2^32 + 2^27 bytes behind the pointer: sign-extended aliases below -front then go unwatched.
        self.front = self.half if front is None else int(front)
        self.view_len = self.total - self.front
        self.lo, self.hi = -self.front, self.view_len  # the allocation in view coordinates

    def aliases(self, x):
        """where a 32-bit truncation of offset x lands: x mod 2^bits and, when that is >= 2^(bits-1), that minus 2^bits (the
        sign extension); each one that lies inside the allocation and is not x itself"""
        x = int(x)
        u = x % self.full
        cand = [u] + ([u - self.full] if u >= self.half else [])
        return [a for a in cand if a != x and self.lo <= a < self.hi]

    def shifts(self, start, size):
        """the distances at which a region has aliases: those of its first and of its last byte (a region that straddles a
        mark has aliases its start has not)"""
        out = []
        for x in (int(start), int(start) + max(int(size), 1) - 1):
            for a in self.aliases(x):
                if a - x not in out:
                    out.append(a - x)
        return out


FAR = Space(32)


def aliases(x, space=FAR):
    return space.aliases(x)


# ---- layouts ---------------------------------------------------------------------------------------------------------------------

def memory_order(n):
    """the order in which a permuted layout's blocks lie in memory: the odd blocks descending, block 0, the even ones
    ascending.  From 2 blocks on, block 1 lies below block 0 (below its predecessor and below the call's first block); the
    last odd block lies lowest and the last even one highest, and one of them is the other's predecessor."""
    return [i for i in range(n - 1, 0, -1) if i % 2] + [i for i in range(0, n, 2)]


def _zones(n):
    """far layouts: the zone of every memory position, ascending.  0 near offset 0, 1 straddling 2^31, 2 above it, 3 straddling
    2^32, 4 above it; the straddling zones hold one region each."""
    if n < 5:
        return {0: [], 1: [3], 2: [0, 4], 3: [0, 3, 4], 4: [0, 1, 3, 4]}[n]
    base, rem = divmod(n - 2, 3)
    a, b, c = base + (rem > 0), base + (rem > 1), base
    return [0] * a + [1] + [2] * b + [3] + [4] * c


def _bump(pos, residue):
    return pos + (residue - pos) % 16


_SPREAD = 2 * G.END_GUARD + G.GAP      # regions of a far zone are a window apart: no two windows of a far layout overlap


def place(sizes, mode, space=FAR, first_residue=0, zones=None):
    """region starts (view coordinates) of regions of `sizes` bytes, in the call's block order.

    "dense": ascending, guarded.GAP between regions (the control).  "permuted": the same positions, held by the blocks in
    memory_order.  "far": ascending through _zones: near 0, straddling and above 2^31, straddling and above 2^32.
    "far_permuted": the far positions in memory_order -- some block then lies more than 2^32 bytes from its predecessor.
    The region at memory position k starts at residue (first_residue + k) mod 16.  zones (far layouts; ascending, one per
    memory position) replaces _zones: a call with one or two regions says where it wants them.  Raises ValueError when regions,
    windows of different zones or alias windows would overlap, or do not fit the space."""
    sizes = [int(s) for s in sizes]
    n = len(sizes)
    if mode not in MODES:
        raise ValueError(mode)
    order = memory_order(n) if mode in ("permuted", "far_permuted") else list(range(n))
    msizes = [sizes[i] for i in order]                 # sizes by memory position
    mstarts = [0] * n
    if mode in ("dense", "permuted"):
        if zones is not None:
            raise ValueError("zones are for the far layouts")
        pos = G.END_GUARD
        for k, s in enumerate(msizes):
            pos = _bump(pos, (first_residue + k) % 16)
            mstarts[k] = pos
            pos += s + G.GAP
    else:
        zones = _zones(n) if zones is None else list(zones)
        if len(zones) != n or sorted(zones) != zones or any(zones.count(z) > 1 for z in (1, 3)):
            raise ValueError("zones: one per region, ascending, one region per straddling zone")
        by_zone = {z: [k for k in range(n) if zones[k] == z] for z in range(5)}
        step = _SPREAD

        def run(base, ks):                             # consecutive regions from `base` on; the end of the last one's window
            pos = base
            for k in ks:
                pos = _bump(pos, (first_residue + k) % 16)
                mstarts[k] = pos
                pos += msizes[k] + step
            return pos
        # the straddling regions first: the one at 2^32 has its alias around offset 0, where zone 0 must stay clear of it
        for z, mark in ((1, space.half), (3, space.full)):
            for k in by_zone[z]:
                want = (first_residue + k) % 16
                s = mark - msizes[k] // 2
                mstarts[k] = s - (s - want) % 16
        clear0 = max([G.END_GUARD] + [msizes[k] - msizes[k] // 2 + 2 * G.END_GUARD + G.GAP for k in by_zone[3]])
        end0 = run(clear0, by_zone[0])
        run(space.half + max([0] + [msizes[k] for k in by_zone[1]]) + step, by_zone[2])
        # zone 4 aliases to offsets behind zone 0
        run(space.full + end0 + step, by_zone[4])
    starts = [0] * n
    for k, i in enumerate(order):
        starts[i] = mstarts[k]
    check_layout(starts, sizes, space, windows=mode in ("far", "far_permuted"))
    return starts


def _overlap(a, b):
    return a[0] < b[1] and b[0] < a[1]


def check_layout(starts, sizes, space=FAR, windows=True):
    """ValueError unless every region lies inside the view, no two regions touch or overlap, no region overlaps another
    region's alias window and -- with `windows` -- no window overlaps another region's window or alias window"""
    regs = [(s, s + n) for s, n in zip(starts, sizes)]
    for r in regs:
        if r[0] < 0 or r[1] > space.view_len:
            raise ValueError("region %r outside the view" % (r,))
    wins = [(s - G.END_GUARD, e + G.END_GUARD) for s, e in regs]
    al = [[(w[0] + d, w[1] + d) for d in space.shifts(r[0], r[1] - r[0])] for r, w in zip(regs, wins)]
    for i in range(len(regs)):
        for j in range(len(regs)):
            if i == j:
                continue
            if i < j and regs[i][0] <= regs[j][1] and regs[j][0] <= regs[i][1]:
                raise ValueError("regions %d and %d touch or overlap" % (i, j))
            if windows and i < j and _overlap(wins[i], wins[j]):
                raise ValueError("windows %d and %d overlap" % (i, j))
            for a in al[j]:
                if _overlap(regs[i], a) or (windows and _overlap(wins[i], a)):
                    raise ValueError("region %d overlaps an alias window of region %d" % (i, j))


def units(starts, unit_sizes):
    """a linked compress stream lies back to back as one unit: the starts of the blocks of unit u, placed at starts[u]"""
    out = []
    for s, lens in zip(starts, unit_sizes):
        pos = s
        for n in lens:
            out.append(pos)
            pos += n
    return out


def describe(starts, sizes, space=FAR):
    """what a layout has, for the tests that pin it"""
    regs = [(s, s + n) for s, n in zip(starts, sizes)]
    dist = [abs(starts[i] - starts[i - 1]) for i in range(1, len(starts))]
    return {
        "straddles_half": any(s < space.half < e for s, e in regs), "above_half": any(space.half <= s and e <= space.full for s, e in regs),
        "straddles_full": any(s < space.full < e for s, e in regs), "above_full": any(space.full <= s for s, e in regs),
        "near_zero": any(e < space.half // 2 for s, e in regs),
        "below_predecessor": any(starts[i] < starts[i - 1] for i in range(1, len(starts))),
        "below_first": any(s < starts[0] for s in starts[1:]),
        "max_predecessor_distance": max(dist) if dist else 0,
        "residues": {s % 16 for s in starts},
    }


# ---- window guards -----------------------------------------------------------------------------------------------------------------

class Windows:
    """The guard windows of one call's output regions in a far buffer.  fill(buf) before the call, check(buf) after it; buf
    is the whole allocation (a numpy array or a torch tensor of space.total bytes)."""

    def __init__(self, starts, sizes, space=FAR, seed=0, reach=G.END_GUARD):
        if reach < G.END_GUARD:
            raise ValueError("windows narrower than a workgroup segment")
        self.space, self.seed = space, seed
        self.regions = [(int(s), int(s) + int(n)) for s, n in zip(starts, sizes)]
        spans = []
        for s, e in self.regions:
            w = (s - reach, e + reach)
            spans.append(w)
            spans += [(w[0] + d, w[1] + d) for d in space.shifts(s, e - s)]
        # in allocation coordinates, clipped to the allocation, overlapping windows merged
        self.spans = [tuple(m) for m in G._merge([(a + space.front, b + space.front) for a, b in spans], space.total)]
        self.allowed = [tuple(m) for m in G._merge([(a + space.front, b + space.front) for a, b in self.regions], space.total)]
        self._regions_abs = [(a + space.front, b + space.front) for a, b in self.regions]

    def _seed(self, k):
        return self.seed + 1 + k                      # a window's pattern is its own: positions 2^32 apart do not share bytes

    def fill(self, buf):
        for k, (a, b) in enumerate(self.spans):
            buf[a:b] = G.pattern(a, b - a, self._seed(k), like=buf)

    def violations(self, buf):
        torch_ = G._is_torch(buf)
        count, found = 0, []
        for k, (a, b) in enumerate(self.spans):
            bad = buf[a:b] != G.pattern(a, b - a, self._seed(k), like=buf)
            for s, e in self.allowed:
                if s < b and a < e:
                    bad[max(s, a) - a:min(e, b) - a] = False
            n = int(bad.sum().item()) if torch_ else int(bad.sum())
            if n and len(found) < G._MAX_REPORT:
                where = (bad.nonzero().flatten().cpu().numpy() if torch_ else np.flatnonzero(bad))[: G._MAX_REPORT - len(found)]
                vals = buf[a:b][where.tolist()]
                vals = vals.cpu().tolist() if torch_ else vals.tolist()
                found += [(int(w) + a, v) for w, v in zip(where.tolist(), vals)]
            count += n
        front = self.space.front
        rep = []
        for off, v in found:                           # reported as guarded.assert_confined does, in view coordinates
            _, k, d, _ = G._describe(off, v, self._regions_abs)
            rep.append((off - front, k, d, v))
        return count, rep

    def check(self, buf, what=""):
        count, found = self.violations(buf)
        assert count == 0, ("%s: %d bytes written outside the allowed ranges; (offset, nearest region, distance from its start "
                            "(<0) or end (>0), value): %r" % (what, count, found))


# ---- inputs and their decoys --------------------------------------------------------------------------------------------------------

def _store(buf, at, data):
    d = np.frombuffer(bytes(data), dtype=np.uint8)
    if not d.size:
        return
    if G._is_torch(buf):
        import torch
        buf[at:at + d.size] = torch.from_numpy(d.copy()).to(buf.device)
    else:
        buf[at:at + d.size] = d


def put_inputs(buf, starts, datas, decoys, space=FAR):
    """datas[i] at starts[i] of the view and, at every alias of starts[i], decoys[i] (or decoys[i % len]): other valid input of
    another length.  ValueError when a decoy would overlap an input or leave the allocation."""
    regs = [(s, s + len(d)) for s, d in zip(starts, datas)]
    for i, (s, d) in enumerate(zip(starts, datas)):
        dec = decoys[i % len(decoys)] if decoys else b""
        if dec and len(dec) == len(d) and bytes(dec) == bytes(d):
            raise ValueError("decoy %d equals its input" % i)
        for a in space.aliases(s):
            if a + len(dec) > space.hi:
                raise ValueError("decoy %d leaves the allocation" % i)
            if any(_overlap((a, a + len(dec)), r) for r in regs):
                raise ValueError("decoy %d overlaps an input" % i)
            _store(buf, a + space.front, dec)
    for s, d in zip(starts, datas):                   # (inputs last: they win where a decoy's tail was checked clear anyway)
        _store(buf, s + space.front, d)


def read(buf, start, n, space=FAR):
    """bytes [start, start + n) of the view"""
    part = buf[start + space.front:start + space.front + n]
    return (part.cpu().numpy() if G._is_torch(buf) else part).tobytes()


def new_far(device="cuda:0", space=FAR):
    """one far buffer: torch.empty, never filled"""
    import torch
    return torch.empty(space.total, dtype=torch.uint8, device=device)


def view(buf, space=FAR):
    return buf[space.front:]
