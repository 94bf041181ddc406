"""The frame batches' contract in plain Python: what mi355lz4_frames_load and mi355lz4_frames_decode must answer for one input.

model(data, oracle, flags) walks the input by the format rules stated in include/mi355lz4.h ("batches of standard LZ4 frames"),
checks header, block and content checksums with an xxh32 written from its published definition, sizes every compressed block
by the decoded-size rule without the last clause of its rule 4 (size_model.model_size keeps that clause), decodes it through
the committed oracle with the frame's window as dictionary, and returns the size or the code of the error with the smallest
byte position.  It shares no code with the library.

Test infrastructure only (imported by tests, like lz4_synth.py).
"""
import lz4_synth as Z

E_MAGIC, E_HEADER, E_HEADER_CHECKSUM, E_TRUNCATED, E_BLOCK_SIZE, E_BLOCK_CHECKSUM, E_BLOCK, E_CONTENT_SIZE, \
    E_CONTENT_CHECKSUM = [-0x7F000100 - k for k in range(1, 10)]
NAMES = {E_MAGIC: "MAGIC", E_HEADER: "HEADER", E_HEADER_CHECKSUM: "HEADER_CHECKSUM", E_TRUNCATED: "TRUNCATED",
         E_BLOCK_SIZE: "BLOCK_SIZE", E_BLOCK_CHECKSUM: "BLOCK_CHECKSUM", E_BLOCK: "BLOCK", E_CONTENT_SIZE: "CONTENT_SIZE",
         E_CONTENT_CHECKSUM: "CONTENT_CHECKSUM"}
SKIP_CONTENT_CHECKSUM, SKIP_BLOCK_CHECKSUM = 1, 2
MAGIC = 0x184D2204

_M = 0xFFFFFFFF
_P1, _P2, _P3, _P4, _P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & _M


def xxh32(data, seed=0):
    data = bytes(data)
    n, p = len(data), 0
    if n >= 16:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed & _M, (seed - _P1) & _M]
        while p + 16 <= n:
            for j in range(4):
                w = int.from_bytes(data[p + 4 * j: p + 4 * j + 4], "little")
                v[j] = (_rotl((v[j] + w * _P2) & _M, 13) * _P1) & _M
            p += 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while p + 4 <= n:
        h = (_rotl((h + int.from_bytes(data[p: p + 4], "little") * _P3) & _M, 17) * _P4) & _M
        p += 4
    while p < n:
        h = (_rotl((h + data[p] * _P5) & _M, 11) * _P1) & _M
        p += 1
    h ^= h >> 15
    h = (h * _P2) & _M
    h ^= h >> 13
    h = (h * _P3) & _M
    h ^= h >> 16
    return h


def block_size(block, max_uncomp):
    """size_model.model_size for a frame's block: everything but the last clause of rule 4.  None: no size to vouch for."""
    block = bytes(block)
    try:
        seqs = Z.parse(block)
    except ValueError:
        return None
    if not seqs or seqs[-1][3] is not None:
        return None
    last = seqs[-1]
    s = last[5] + last[2]
    if s > max_uncomp:
        return None
    for _tp, _, lit, off, ml, op in seqs[:-1]:
        pos = op + lit
        if s < Z.MFLIMIT + 1 or pos > s - Z.MFLIMIT or pos + ml > s - Z.LASTLITERALS:
            return None
        if off == 0:
            return None
    if s == 0 and block != b"\x00":
        return None
    return s


class Frame:
    def __init__(self):
        self.flg = 0
        self.bmax = 0
        self.declared = None
        self.blocks = []          # (position of the size word, stored, payload bytes, checksum word or None)
        self.end = None           # position of the end mark (None: a structural error ended the frame)
        self.checksum = None


def walk(data):
    """([Frame], (position, code) of the first structural error or None)"""
    data = bytes(data)
    n, pos, frames = len(data), 0, []

    def u32(at):
        return int.from_bytes(data[at: at + 4], "little")

    while pos < n:
        if n - pos < 4:
            return frames, (pos, E_TRUNCATED)
        magic = u32(pos)
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            if n - pos < 8 or n - pos - 8 < u32(pos + 4):
                return frames, (pos, E_TRUNCATED)
            pos += 8 + u32(pos + 4)
            continue
        if magic != MAGIC:
            return frames, (pos, E_MAGIC)
        if n - pos < 6:
            return frames, (pos, E_TRUNCATED)
        flg, bd = data[pos + 4], data[pos + 5]
        code = (bd >> 4) & 7
        if flg >> 6 != 1 or flg & 3 or code < 4 or bd & 0x8F:
            return frames, (pos, E_HEADER)
        dlen = 2 + (8 if flg & 8 else 0)
        if n - pos < 4 + dlen + 1:
            return frames, (pos, E_TRUNCATED)
        if data[pos + 4 + dlen] != (xxh32(data[pos + 4: pos + 4 + dlen]) >> 8) & 0xFF:
            return frames, (pos, E_HEADER_CHECKSUM)
        f = Frame()
        f.flg, f.bmax = flg, 1 << (8 + 2 * code)
        if flg & 8:
            f.declared = int.from_bytes(data[pos + 6: pos + 14], "little")
        frames.append(f)
        trailer = 4 if flg & 0x10 else 0
        p = pos + 4 + dlen + 1
        while True:
            if n - p < 4:
                return frames, (p, E_TRUNCATED)
            word = u32(p)
            if word == 0:
                if flg & 4:
                    if n - p - 4 < 4:
                        return frames, (p, E_TRUNCATED)
                    f.checksum = u32(p + 4)
                f.end = p
                p += 4 + (4 if flg & 4 else 0)
                break
            k = word & 0x7FFFFFFF
            if k > f.bmax:
                return frames, (p, E_BLOCK_SIZE)
            if n - p - 4 < k + trailer:
                return frames, (p, E_TRUNCATED)
            f.blocks.append((p, bool(word >> 31), data[p + 4: p + 4 + k], u32(p + 4 + k) if trailer else None))
            p += 4 + k + trailer
        pos = p
    return frames, None


def model(data, oracle, flags=0):
    """(sizes entry, result entry, decoded bytes or None): what _load and _decode report for this input."""
    frames, structural = walk(data)
    errs = [structural] if structural else []
    sizes = {}
    total = 0
    for f in frames:
        fsz = 0
        for (p, stored, payload, ck) in f.blocks:
            s = len(payload) if stored else block_size(payload, f.bmax)
            if ck is not None and not flags & SKIP_BLOCK_CHECKSUM and xxh32(payload) != ck:
                errs.append((p, E_BLOCK_CHECKSUM))          # (the checksum covers the bytes as stored: it is judged first)
            elif s is None:
                errs.append((p, E_BLOCK))
            sizes[p] = s
            fsz += s or 0
        if f.end is not None and f.declared is not None and f.declared != fsz:
            errs.append((f.end, E_CONTENT_SIZE))
        total += fsz
    if errs:
        code = min(errs)[1]
        return code, code, None
    out = bytearray()
    derr = []
    for f in frames:
        linked = not f.flg & 0x20
        fo = bytearray()
        ok = True
        for (p, stored, payload, _ck) in f.blocks:
            if stored:
                fo += payload
                continue
            if not payload:
                continue
            window = bytes(fo[-65536:]) if linked else None
            r, got = oracle.decompress_block(payload, sizes[p], window)
            if r != sizes[p]:
                derr.append((p, E_BLOCK))
                ok = False
                if linked:
                    break
                fo += bytes(sizes[p])
            else:
                fo += got
        if ok and f.checksum is not None and not flags & SKIP_CONTENT_CHECKSUM and xxh32(fo) != f.checksum:
            derr.append((f.end, E_CONTENT_CHECKSUM))
        fo += bytes(sum((sizes[b[0]] for b in f.blocks)) - len(fo))
        out += fo
    if derr:
        return total, min(derr)[1], None
    return total, total, bytes(out)
