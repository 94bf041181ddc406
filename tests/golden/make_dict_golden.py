"""Writes tests/golden/dict_vectors.json: what the reference's LZ4_loadDict + LZ4_compress_fast_continue (cbits/lz4.c:1475-1515,
1565-1637) and LZ4_decompress_safe_usingDict (:2404-2417) return and write on the inputs of tests/dict_cases.py.  Needs
oracle/_ref/liblz4ref.so (make oracle, where the reference sources are present); it calls the codec's public functions through
ctypes and changes nothing under oracle/.  The file it writes holds data only -- return codes and sha256 sums, the inputs are
rebuilt from seeds by tests/dict_cases.py -- and a re-run leaves it byte-identical.

    python tests/golden/make_dict_golden.py

Layout:
    compress: {"d<dict length>/b<block length>/a<accel>": [code, sha256 of the compressed bytes]}
              LZ4_loadDict once per dictionary, every block on a COPY of the loaded LZ4_stream_t, dstCapacity = LZ4_compressBound(n)
    stream:   {"<dict length>": [[code, sha256], x3]}   dict_cases.stream_blocks() continued on one loaded stream, accel 1
    decode:   [[name, dict length, code, sha256 of the max(code, 0) bytes written]]   dict_cases.decode_cases(), in order

Every source, destination and dictionary lies in a region of its own, a gap apart: neither side's prefix mode (a block directly
behind its dictionary) is ever taken."""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dict_cases as DC  # noqa: E402

STREAMSIZE = 16416        # LZ4_STREAMSIZE, cbits/lz4.h:623
GAP = 4096


def load_reference():
    L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "liblz4ref.so"))
    vp = C.c_void_p
    for name, res, args in (("LZ4_compressBound", C.c_int, [C.c_int]),
                            ("LZ4_initStream", vp, [vp, C.c_size_t]),
                            ("LZ4_loadDict", C.c_int, [vp, vp, C.c_int]),
                            ("LZ4_compress_fast_continue", C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int]),
                            ("LZ4_decompress_safe_usingDict", C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


class Arena:
    """one allocation; every region handed out lies GAP bytes behind the one before"""

    def __init__(self, size):
        self.buf = (C.c_uint8 * size)()
        self.base = C.addressof(self.buf)
        self.size, self.pos = size, GAP

    def put(self, data):
        at = self.take(len(data))
        C.memmove(at, bytes(data), len(data))
        return at

    def take(self, n):
        at = self.base + self.pos
        self.pos = (self.pos + n + GAP + 63) & ~63
        assert self.pos <= self.size, "arena too small"
        return at


def sha(b):
    return hashlib.sha256(b).hexdigest()


def loaded_stream(L, dict_at, dict_len):
    s = (C.c_uint64 * (STREAMSIZE // 8))()
    assert L.LZ4_initStream(C.addressof(s), STREAMSIZE)
    L.LZ4_loadDict(C.addressof(s), dict_at, dict_len)
    return s


def continue_block(L, s, ar, data, accel):
    n = len(data)
    cap = L.LZ4_compressBound(n)
    src, dst = ar.put(data), ar.take(cap)
    r = L.LZ4_compress_fast_continue(C.addressof(s), src, dst, n, cap, accel)
    return [r, sha(C.string_at(dst, max(r, 0)))]


def main():
    L = load_reference()
    compress, stream = {}, {}
    for dl in DC.DICT_LENS:
        ar = Arena(8 << 20)
        d_at = ar.put(DC.dictionary(dl))
        loaded = loaded_stream(L, d_at, dl)
        for bl in DC.BLOCK_LENS:
            for accel in DC.ACCELS:
                s = (C.c_uint64 * (STREAMSIZE // 8))()
                C.memmove(s, loaded, STREAMSIZE)          # a copy of the loaded stream per block
                compress[DC.compress_key(dl, bl, accel)] = continue_block(L, s, ar, DC.block(bl), accel)
        s = (C.c_uint64 * (STREAMSIZE // 8))()
        C.memmove(s, loaded, STREAMSIZE)
        stream[str(dl)] = [continue_block(L, s, ar, b, DC.STREAM_ACCEL) for b in DC.stream_blocks()]
    decode = []
    for name, dl, blk, cap in DC.decode_cases():
        ar = Arena(1 << 20)
        d_at, src = ar.put(DC.dictionary(dl)), ar.put(blk + bytes(64))
        dst = ar.take(max(cap, 0) + 64)
        r = L.LZ4_decompress_safe_usingDict(src, dst, len(blk), cap, d_at, dl)
        decode.append([name, dl, r, sha(C.string_at(dst, max(r, 0)))])
    path = os.path.join(HERE, "dict_vectors.json")
    with open(path, "w") as f:
        json.dump({"note": "LZ4_loadDict + LZ4_compress_fast_continue and LZ4_decompress_safe_usingDict of the reference on "
                           "tests/dict_cases.py's inputs (make_dict_golden.py)",
                   "compress": compress, "stream": stream, "decode": decode}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d compress cases, %d streams, %d decode cases, %d bytes"
          % (path, len(compress), len(stream), len(decode), os.path.getsize(path)))


if __name__ == "__main__":
    main()
