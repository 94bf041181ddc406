"""The model the decode-streams tests hold the engine to, and the streams they feed it (test infrastructure only).

A stream is a list of Block; the model is the reference's LZ4_decompress_safe_continue over separately allocated blocks
(cbits/lz4.c:2322-2359) restated with the CPU oracle: prev = None; per block r, b = decompress_block(comp, cap, prev); r > 0
makes b the next dictionary; a header-rejected block gets its header code and changes nothing.

The inputs are linked streams as the reference's compressChunksD writes them: Oracle.frame_compress(linked=True) for blocks
of one length, and the same call sequence (orc_compress_fast_continue on one stream, every array its own allocation) for
blocks of mixed lengths -- linked_stream() is checked against frame_compress in tests/test_dstreams_host.py.
"""
import collections
import ctypes as C
import glob
import os

import numpy as np

BLK_E_COMPLEN = -0x7F000001
BLK_E_CHECKSUM = -0x7F000004
_u8p = C.POINTER(C.c_uint8)

# framed: the block as it lies in the framed buffer; comp: its compressed bytes; cap: the capacity it is decoded into;
# hdr: 0, or the code its header is rejected with (then comp is not looked at)
Block = collections.namedtuple("Block", "framed comp cap hdr")

_DATA = {}


def data(oracle, kind, nbytes, first=0):
    """text-like bytes of the oracle's generator, or Python source (the standard library's, as tests/test_compress_streams_gpu.py)"""
    key = (kind, nbytes, first)
    if key not in _DATA:
        if kind == "pysrc":
            buf = bytearray()
            for f in sorted(glob.glob(os.path.join(os.path.dirname(os.__file__), "*.py"))):
                buf += open(f, "rb").read()
                if len(buf) >= nbytes + first:
                    break
            while len(buf) < nbytes + first:
                buf = buf + buf
            _DATA[key] = bytes(buf[first:first + nbytes])
        else:
            _DATA[key] = oracle.gen("text", 1, nbytes + first).tobytes()[first:]
    return _DATA[key]


def cut(buf, lens):
    out, p = [], 0
    for n in lens:
        out.append(buf[p:p + n])
        p += n
    assert p <= len(buf)
    return out


def linked_stream(oracle, arrays, accel=1, ragged=False):
    """The compressed blocks of ONE linked stream over `arrays`: frame_compress(linked=True) when they are blocks of one length
    (a shorter last one allowed), else -- or with ragged=True -- its call sequence for ragged arrays."""
    lens = [len(a) for a in arrays]
    if not ragged and lens and all(n == lens[0] for n in lens[:-1]) and 0 < lens[-1] <= lens[0]:
        framed = oracle.frame_compress(b"".join(arrays), lens[0], accel, 8, True)
        out, p = [], 0
        while p < len(framed):
            c = int.from_bytes(framed[p:p + 4], "little")
            out.append(framed[p + 8:p + 8 + c])
            p += 8 + c
        assert len(out) == len(arrays)
        return out
    L = oracle.lib
    L.orc_compress_fast_continue.restype = C.c_int
    L.orc_compress_fast_continue.argtypes = [C.c_void_p, _u8p, _u8p, C.c_int, C.c_int, C.c_int]
    st = C.create_string_buffer(16384 + 256)
    L.orc_cstream_init(st)
    out, keep = [], []
    for a in arrays:
        src = np.zeros(len(a) + 64, dtype=np.uint8)          # its own allocation, like a Haskell Array
        src[: len(a)] = np.frombuffer(bytes(a), dtype=np.uint8)
        cap = oracle.compress_bound(len(a))
        dst = np.zeros(cap + 64, dtype=np.uint8)
        r = L.orc_compress_fast_continue(st, src.ctypes.data_as(_u8p), dst.ctypes.data_as(_u8p), len(a), cap, int(accel))
        assert r > 0
        out.append(dst[:r].tobytes())
        keep = keep[-1:] + [src]                             # the previous array stays alive: it is the dictionary
    return out


def xxh32(b):
    import streamly_lz4_amd as S
    a = np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(1, dtype=np.uint8)
    return int(S.lib.slz4_xxh32(a.ctypes.data_as(_u8p), len(b), 0))


def frame(comp, uncomp, kind, checksum=False, bad_checksum=False):
    """| compLen | uncompLen (kind 8) | data | xxh32 of the data (checksums) |"""
    out = bytearray(len(comp).to_bytes(4, "little"))
    if kind == 8:
        out += int(uncomp).to_bytes(4, "little")
    out += comp
    if checksum:
        out += ((xxh32(comp) ^ (1 if bad_checksum else 0)) & 0xFFFFFFFF).to_bytes(4, "little")
    return bytes(out)


def good_block(comp, uncomp, kind, checksum=False):
    return Block(frame(comp, uncomp, kind, checksum), comp, uncomp, 0)


def rejected_block(kind, checksum=False):
    """compLen = 0: MI355LZ4_BLK_E_COMPLEN, a header and (with checksums) a trailer and nothing between"""
    return Block(frame(b"", 0, kind, checksum), b"", 0, BLK_E_COMPLEN)


def bad_checksum_block(comp, uncomp, kind):
    return Block(frame(comp, uncomp, kind, True, bad_checksum=True), comp, uncomp, BLK_E_CHECKSUM)


def make_stream(oracle, arrays, kind, checksum=False):
    return [good_block(c, len(a), kind, checksum) for c, a in zip(linked_stream(oracle, arrays), arrays)]


def model(oracle, blocks, prev=None):
    """([code per block], [bytes per block], the dictionary after the last block)"""
    codes, outs = [], []
    for b in blocks:
        if b.hdr:
            codes.append(b.hdr)
            outs.append(b"")
            continue
        r, got = oracle.decompress_block(b.comp, b.cap, dict_bytes=prev)
        codes.append(r)
        outs.append(got)
        if r > 0:
            prev = got
    return codes, outs, prev


def assert_dependent(oracle, blocks):
    """every block after the stream's first fails on its own: no test passes by accident on a decoder without dictionaries"""
    for i, b in enumerate(blocks[1:], 1):
        if b.hdr == 0 and b.cap > 0:
            r, _ = oracle.decompress_block(b.comp, b.cap)
            assert r < 0, "block %d decodes without its dictionary (%d)" % (i, r)


def first_offset_pos(comp):
    """index of the low byte of the first sequence's offset field"""
    tok = comp[0]
    lit, p = tok >> 4, 1
    if lit == 15:
        while True:
            lit += comp[p]
            p += 1
            if comp[p - 1] != 255:
                break
    return p + lit


def corrupt_first_offset(comp):
    """one flipped offset byte: the first match's offset gets its high byte inverted"""
    p = first_offset_pos(comp) + 1
    assert p < len(comp)
    return comp[:p] + bytes([comp[p] ^ 0xFF]) + comp[p + 1:]


# ---- the streams of tests 1, 2, 5, 9: five streams of six blocks, every length of the set in every stream ---------------------
CUT_LENS = [
    [65536, 1000, 40, 4096, 70000, 262144],     # a dictionary of exactly 64 KiB, then short ones
    [262144, 65536, 70000, 40, 1000, 4096],     # longer than 64 KiB: only the tail is kept
    [40, 4096, 1000, 65536, 262144, 70000],     # a tiny first block
    [70000, 262144, 4096, 1000, 65536, 40],
    [4096, 70000, 65536, 262144, 1000, 40],
]
CUT_DATA = ["text", "pysrc", "pysrc", "pysrc", "text"]
CUT_SLOTS = [5, 0, 7, 2, 3]                     # of a set of eight: not the identity
# blocks of each stream per call
PARTITIONS = {
    "one": [[1] * 5] * 6,
    "two_three": [[2, 3, 2, 3, 2], [3, 2, 3, 2, 3], [1, 1, 1, 1, 1]],
    "uneven": [[2, 1, 6, 0, 3], [0, 4, 0, 1, 0], [4, 1, 0, 5, 3]],
}
_CUT = {}


def cut_arrays(oracle):
    out = []
    for s, lens in enumerate(CUT_LENS):
        buf = data(oracle, CUT_DATA[s], sum(lens), first=s * 1000)
        out.append(cut(buf, lens))
    return out


def cut_streams(oracle, kind, checksum=False):
    """(the five streams as lists of Block, the arrays they were compressed from)"""
    key = (kind, checksum)
    if key not in _CUT:
        arrays = cut_arrays(oracle)
        _CUT[key] = ([make_stream(oracle, a, kind, checksum) for a in arrays], arrays)
    return _CUT[key]


def failing_stream(oracle, kind, checksum=False):
    """test 3: two good blocks, a corrupted one, a zero-byte array, a header-rejected block, then a good block that depends on
    the second -- the last block with r > 0 in front of it"""
    buf = data(oracle, "text", 3 * 4096, first=777)
    arrays = cut(buf, [4096, 4096, 4096])
    comps = linked_stream(oracle, arrays)
    bad = corrupt_first_offset(comps[2])
    return [good_block(comps[0], 4096, kind, checksum), good_block(comps[1], 4096, kind, checksum),
            good_block(bad, 4096, kind, checksum), good_block(b"\x00", 0, kind, checksum), rejected_block(kind, checksum),
            good_block(comps[2], 4096, kind, checksum)], arrays
