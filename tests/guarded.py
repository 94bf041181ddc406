"""Guarded buffers: what a kernel must NOT touch, made observable.

A call is handed regions of one allocation (a block's output, a compress slot, a result array).  layout() places the regions in
one buffer with guards between them and larger guards at both ends; fill() writes a byte pattern that depends on the position;
violations() recomputes the pattern after the call and reports every byte outside the allowed ranges that no longer holds it.

  * Region starts cycle through all 16 residues mod 16; with equal or ragged sizes the ends do too (Layout.start_residues /
    end_residues say which occur, tests/test_guarded.py pins them for the layouts the GPU tests use).
  * A guard between two regions is at least GAP bytes: one wavefront-wide 16-byte store (64 lanes x 16 = 1 KiB) plus an odd
    remainder, so that a whole stray vector store lands in bytes that are checked and no region start inherits its
    predecessor's alignment.
  * The end guards are at least END_GUARD bytes: one 32 KiB workgroup segment.  A stray write inside the allocation is seen; one
    outside it is not, so the guards must be wider than the widest single store a kernel issues.
  * The pattern is a hash of the byte's index (and a seed), never a constant: a stray COPY of neighbouring guard bytes, or of
    another guarded buffer, does not restore the expected value.

Works on numpy arrays (host-buffer calls, tests without a GPU) and on torch tensors (the check runs on the device in chunks and
brings back only the violations, so layouts of several GiB stay cheap).  torch is imported only when a tensor is handed in.

Test infrastructure only (imported by tests, like lz4_synth.py).
"""
import numpy as np

WAVE_STORE = 64 * 16          # one wavefront, 16 bytes a lane
GAP = WAVE_STORE + 13         # guard between regions (an odd remainder on top of a wave-wide store)
END_GUARD = 32768 + 5         # guard at both ends of the allocation (a workgroup's LDS segment, and then some)
_CHUNK = 1 << 24              # bytes checked per step (the index array is 8 bytes a byte)
_MAX_REPORT = 32              # violations brought back in full; the count is always exact


class Layout:
    """starts[i], sizes[i]: region i is [starts[i], starts[i] + sizes[i]) of a buffer of `total` bytes."""

    def __init__(self, starts, sizes, total):
        self.starts, self.sizes, self.total = list(starts), list(sizes), int(total)

    def __len__(self):
        return len(self.starts)

    def ranges(self):
        return [(s, s + n) for s, n in zip(self.starts, self.sizes)]

    def start_residues(self):
        return {s % 16 for s in self.starts}

    def end_residues(self):
        return {(s + n) % 16 for s, n in zip(self.starts, self.sizes)}

    def gaps(self):
        """the guards, in order: head, between consecutive regions, tail"""
        edges = [0] + [x for r in self.ranges() for x in r] + [self.total]
        return [(edges[i], edges[i + 1]) for i in range(0, len(edges), 2)]


def layout(sizes, stride=None, first_residue=0, gap=GAP, end_guard=END_GUARD, align=1):
    """Places regions of `sizes` bytes in one buffer.

    stride = None: every region gets its own start; region k starts at a position = (first_residue + k) * align mod 16, at least
    `gap` bytes behind the end of region k - 1.  (align = 4 / 8 for arrays of int32 / int64 items: then only the residues that
    are multiples of it occur.)
    stride = n: the regions are the slots of a compress call, region k at base + k * stride with base = first_residue mod 16;
    what lies between a region's end and the next slot is the caller's guard (stride - size), the end guards are the builder's.
    """
    sizes = [int(s) for s in sizes]
    if gap < GAP or end_guard < END_GUARD:
        raise ValueError("guards narrower than a wave-wide store / a workgroup segment")
    starts = []
    if stride is not None:
        if any(s > stride for s in sizes):
            raise ValueError("a region is larger than the stride")
        base = end_guard + (first_residue - end_guard) % 16
        starts = [base + k * stride for k in range(len(sizes))]
        end = base + len(sizes) * stride if sizes else base
    else:
        pos = end_guard
        for k, n in enumerate(sizes):
            want = ((first_residue + k) * align) % 16
            pos += (want - pos) % 16
            starts.append(pos)
            pos += n + gap
        end = pos - gap if sizes else pos
    return Layout(starts, sizes, end + end_guard)


# ---- the pattern ---------------------------------------------------------------------------------------------------------------

def _mix(idx, seed):
    """byte value at index idx (an int64 array, numpy or torch): a 32-bit integer hash of the index, its low byte.  Every
    intermediate stays below 2^62."""
    x = (idx + (seed & 0xFFFF) * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF
    x = ((x ^ (x >> 15)) * 0x2C1B3C6D) & 0xFFFFFFFF
    x = ((x ^ (x >> 12)) * 0x297A2D39) & 0xFFFFFFFF
    return (x ^ (x >> 15)) & 0xFF


def _is_torch(buf):
    return type(buf).__module__.split(".")[0] == "torch"


def pattern(start, n, seed=0, like=None):
    """the pattern's bytes [start, start + n): a numpy uint8 array, or a torch tensor on `like`'s device"""
    if like is not None and _is_torch(like):
        import torch
        idx = torch.arange(start, start + n, dtype=torch.int64, device=like.device)
        return _mix(idx, seed).to(torch.uint8)
    return _mix(np.arange(start, start + n, dtype=np.int64), seed).astype(np.uint8)


def fill(buf, seed=0):
    """writes the pattern over all of buf (1-D uint8, numpy or torch), in place; returns buf"""
    n = int(buf.shape[0])
    for a in range(0, n, _CHUNK):
        b = min(n, a + _CHUNK)
        buf[a:b] = pattern(a, b - a, seed, like=buf)
    return buf


def new_numpy(total, seed=0):
    return fill(np.empty(int(total), dtype=np.uint8), seed)


def new_torch(total, seed=0, device="cuda:0"):
    import torch
    return fill(torch.empty(int(total), dtype=torch.uint8, device=device), seed)


# ---- the checker ---------------------------------------------------------------------------------------------------------------

def _merge(ranges, total):
    out = []
    for s, e in sorted((max(0, int(s)), min(int(total), int(e))) for s, e in ranges):
        if e <= s:
            continue
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def _describe(off, value, ranges):
    """(offset, nearest region, distance, value): distance < 0 = that many bytes in front of the region's start, > 0 = the
    byte's position behind the region's end (1 = the first byte past it)"""
    if not ranges:
        return (off, None, None, value)
    best = None
    for k, (s, e) in enumerate(ranges):
        d = off - s if off < s else off - e + 1
        if best is None or abs(d) < abs(best[1]):
            best = (k, d)
    return (off, best[0], best[1], value)


def violations(buf, allowed, seed=0):
    """(count, [(offset, nearest region, distance, value)]): the bytes of buf outside the allowed ranges [(start, end)] that no
    longer hold the pattern.  Regions are numbered as given in `allowed`.  At most _MAX_REPORT of them are described (the first
    ones), all are counted."""
    total = int(buf.shape[0])
    allowed = [(int(s), int(e)) for s, e in allowed]
    merged = _merge(allowed, total)
    torch_ = _is_torch(buf)
    if torch_:
        import torch
        st = torch.tensor([m[0] for m in merged] or [total], dtype=torch.int64, device=buf.device)
        en = torch.tensor([m[1] for m in merged] or [total], dtype=torch.int64, device=buf.device)
    else:
        st = np.array([m[0] for m in merged] or [total], dtype=np.int64)
        en = np.array([m[1] for m in merged] or [total], dtype=np.int64)
    count, found = 0, []
    for a in range(0, total, _CHUNK):
        b = min(total, a + _CHUNK)
        if torch_:
            idx = torch.arange(a, b, dtype=torch.int64, device=buf.device)
            k = torch.searchsorted(st, idx, right=True) - 1
            inside = (k >= 0) & (idx < en[k.clamp(min=0)])
            bad = (buf[a:b] != _mix(idx, seed).to(torch.uint8)) & ~inside
            n = int(bad.sum().item())
            if n and len(found) < _MAX_REPORT:
                where = idx[bad][: _MAX_REPORT - len(found)]
                vals = buf[where].cpu().tolist()
                found += list(zip(where.cpu().tolist(), vals))
        else:
            idx = np.arange(a, b, dtype=np.int64)
            k = np.searchsorted(st, idx, side="right") - 1
            inside = (k >= 0) & (idx < en[np.maximum(k, 0)])
            bad = (buf[a:b] != _mix(idx, seed).astype(np.uint8)) & ~inside
            n = int(bad.sum())
            if n and len(found) < _MAX_REPORT:
                where = idx[bad][: _MAX_REPORT - len(found)]
                found += list(zip(where.tolist(), buf[where].tolist()))
        count += n
    return count, [_describe(off, v, allowed) for off, v in found]


def assert_confined(buf, allowed, seed=0, what=""):
    count, found = violations(buf, allowed, seed)
    assert count == 0, ("%s: %d bytes written outside the allowed ranges; (offset, nearest region, distance from its start (<0) "
                        "or end (>0), value): %r" % (what, count, found))


# ---- typed auxiliary arrays (result[], framedLen[], denseOff[], ...) -------------------------------------------------------------

class GuardedArray:
    """n items of `dtype` inside a guarded byte buffer: .view is the array handed to the call, .check() asserts that nothing but
    items [lo, hi) of it was written (default: all n)."""

    def __init__(self, n, dtype, seed, device=None, lead=0):
        self.n, self.seed, self.lead = int(n), seed, int(lead)
        if device is None:
            self.item = np.dtype(dtype).itemsize
            self.lay = layout([(self.n + self.lead) * self.item], first_residue=0)
            self.buf = new_numpy(self.lay.total, seed)
        else:
            import torch
            self.item = torch.empty(0, dtype=dtype).element_size()
            self.lay = layout([(self.n + self.lead) * self.item], first_residue=0)
            self.buf = new_torch(self.lay.total, seed, device)
        s = self.lay.starts[0]
        self.all = self.buf[s:s + (self.n + self.lead) * self.item].view(dtype)   # with the `lead` items in front (result[-1])
        self.view = self.all[self.lead:]

    def check(self, lo=0, hi=None, what=""):
        hi = self.n if hi is None else hi
        s = self.lay.starts[0] + self.lead * self.item
        assert_confined(self.buf, [(s + lo * self.item, s + hi * self.item)], self.seed, what)


# ---- the input side: the same regions, different bytes in every gap ------------------------------------------------------------------

def pair(lay, datas, seeds=(101, 202)):
    """Two numpy buffers of lay.total bytes with datas[i] at region i and different bytes in EVERY guard byte: a call whose
    results differ between the two has read outside the regions it was given."""
    a, b = new_numpy(lay.total, seeds[0]), new_numpy(lay.total, seeds[1])
    # where the two patterns happen to agree (one byte in 256), make them differ
    same = a == b
    b[same] ^= 0x5A
    for s, d in zip(lay.starts, datas):
        d = np.frombuffer(bytes(d), dtype=np.uint8)
        a[s:s + d.size] = d
        b[s:s + d.size] = d
    return a, b
