"""Model of the shared-dictionary calls: LZ4_loadDict (cbits/lz4.c:1475-1515) restated over the oracle's compress stream, then the
oracle's own LZ4_compress_fast_continue.

oracle/lz4_oracle.h exposes orc_cstream {uint32 table[4096]; uint32 currentOffset; const uint8_t *dict; uint32 dictSize} and
orc_compress_fast_continue.  model_load fills such a struct as LZ4_loadDict would: currentOffset = 65536; for len >= 8 (HASH_UNIT
of the reference's 64-bit build) dict points at the last min(len, 65536) bytes and every third position p <= dictEnd - 8 gets
table[hash5(p)] = p + 65536 - keep, in ascending order, so a bucket keeps its last writer.  tests/test_dict_host.py holds the
model to the golden the reference wrote (tests/golden/dict_vectors.json) and, where oracle/_ref exists, to the reference itself.

Test infrastructure only.
"""
import ctypes as C

import numpy as np

from oracle.oracle import Oracle

_u8p = C.POINTER(C.c_uint8)
_PAD = 64
PRIME5 = np.uint64(889523592379)


class OrcCStream(C.Structure):
    _fields_ = [("table", C.c_uint32 * 4096), ("currentOffset", C.c_uint32), ("dict", C.c_void_p), ("dictSize", C.c_uint32)]


_oracle = None


def _lib():
    global _oracle
    if _oracle is None:
        _oracle = Oracle()
        f = _oracle.lib.orc_compress_fast_continue
        f.restype = C.c_int
        f.argtypes = [C.POINTER(OrcCStream), _u8p, _u8p, C.c_int, C.c_int, C.c_int]
    return _oracle.lib


def compress_bound(n):
    return n + n // 255 + 16


def hash5(buf, pos):
    """the byU32 hash5 of the 64-bit little-endian build (cbits/lz4.c:706-716) at every position of pos"""
    v = np.zeros(len(pos), dtype=np.uint64)
    for k in range(8):
        v |= buf[pos + k].astype(np.uint64) << np.uint64(8 * k)
    return (((v << np.uint64(24)) * PRIME5) >> np.uint64(52)).astype(np.int64)


class Loaded:
    """an orc_cstream as LZ4_loadDict leaves it, with the memory its dictionary pointer names kept alive"""

    def __init__(self, dict_bytes, first_writer_wins=False):
        d = np.frombuffer(bytes(dict_bytes), dtype=np.uint8)
        self.s = OrcCStream()
        self.s.currentOffset = 65536
        self.keep = 0
        self.buf = None
        if d.size >= 8:
            keep = min(d.size, 65536)
            self.buf = np.zeros(keep + _PAD, dtype=np.uint8)
            self.buf[:keep] = d[d.size - keep:]
            self.keep = keep
            pos = np.arange(0, keep - 8 + 1, 3, dtype=np.int64)
            h = hash5(self.buf, pos)
            idx = (pos + (65536 - keep)).astype(np.uint32)
            table = np.zeros(4096, dtype=np.uint32)
            if first_writer_wins:                         # (the wrong rule, for the test that the grid can tell the two apart)
                h, idx = h[::-1], idx[::-1]
            for a, b in zip(h.tolist(), idx.tolist()):    # ascending positions: the last writer of a bucket stays
                table[a] = b
            C.memmove(self.s.table, table.ctypes.data, 4096 * 4)
            self.s.dict = self.buf.ctypes.data
            self.s.dictSize = keep

    def copy(self):
        c = OrcCStream()
        C.memmove(C.byref(c), C.byref(self.s), C.sizeof(OrcCStream))
        return c


def model_load(dict_bytes, first_writer_wins=False):
    return Loaded(dict_bytes, first_writer_wins)


def _continue(stream, block, accel, keep):
    n = len(block)
    src = np.zeros(n + _PAD, dtype=np.uint8)
    src[:n] = np.frombuffer(bytes(block), dtype=np.uint8)
    keep.append(src)                                      # the stream's next dictionary
    cap = compress_bound(n)
    dst = np.zeros(cap + _PAD, dtype=np.uint8)
    r = _lib().orc_compress_fast_continue(C.byref(stream), src.ctypes.data_as(_u8p), dst.ctypes.data_as(_u8p), n, cap, int(accel))
    return int(r), dst[:max(r, 0)].tobytes()


def model_compress(loaded, block, accel=1):
    """(code, bytes) of LZ4_compress_fast_continue on a COPY of the loaded stream, cap = LZ4_compressBound(n); loaded may be the
    dictionary's bytes"""
    if not isinstance(loaded, Loaded):
        loaded = model_load(loaded)
    return _continue(loaded.copy(), block, accel, [])


def model_stream(loaded, blocks, accel=1):
    """[(code, bytes)] of the blocks continued one after the other on a copy of the loaded stream"""
    if not isinstance(loaded, Loaded):
        loaded = model_load(loaded)
    s, keep = loaded.copy(), []
    return [_continue(s, b, accel, keep) for b in blocks]


def framed_block(code, comp, n, header_kind):
    """the slot bytes the engine writes for a block: [compLen][uncompLen for kind 8][data]"""
    h = int(code).to_bytes(4, "little") + (int(n).to_bytes(4, "little") if header_kind == 8 else b"")
    return h + comp
