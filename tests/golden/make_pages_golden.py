"""Writes tests/golden/pages_vectors.json: what the reference's LZ4_compress_destSize (cbits/lz4.c:1382-1414) returns, consumes and
writes on the grid of tests/pages_cases.py.  Needs oracle/_ref/liblz4ref.so (make oracle, where the reference sources are
present); it calls the codec's public function through ctypes and changes nothing under oracle/.  The file it writes holds data
only -- return values, consumed counts and truncated sha256 sums; the inputs are rebuilt from seeds by tests/pages_cases.py -- and
a re-run leaves it byte-identical.

    python tests/golden/make_pages_golden.py

Layout: {"<series>": {"ret": [...], "used": [...], "sha": "<6 hex digits per page>"}}, one entry per page:
    ret   the return value
    used  *srcSizePtr after the call (the reference leaves it alone when it returns 0 or hands over to the unlimited encoder)
    sha   the first 6 hex digits of the sha256 of the max(ret, 0) bytes written
  "grid/..", "seam/..", "bound/.."   pages_cases.singles(): one call per pageSize of the series, in order
  "chain/<input>/<pageSize>"         pages_cases.CHAINS: page k is the call on the bytes behind what pages 0..k-1 consumed, until the
                                     input is consumed or a page consumes nothing
"""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pages_cases as PC  # noqa: E402

SHA_DIGITS = 6


def load_reference():
    L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "liblz4ref.so"))
    L.LZ4_compress_destSize.restype = C.c_int
    L.LZ4_compress_destSize.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int]
    return L


def sha(b):
    return hashlib.sha256(b).hexdigest()[:SHA_DIGITS]


def dest_size(L, src_buf, pos, remaining, target):
    """one call on src_buf[pos : pos + remaining]: (ret, used, bytes)"""
    dst = (C.c_uint8 * (max(target, 0) + 64))()
    n = C.c_int(remaining)
    r = L.LZ4_compress_destSize(C.addressof(src_buf) + pos, dst, C.byref(n), target)
    return r, n.value, bytes(dst[:max(r, 0)])


def series_of(pages):
    return {"ret": [p[0] for p in pages], "used": [p[1] for p in pages], "sha": "".join(sha(p[2]) for p in pages)}


def chain(L, data, target):
    buf = (C.c_uint8 * (len(data) + 64)).from_buffer_copy(data + bytes(64))
    pos, pages = 0, []
    while True:
        r, used, out = dest_size(L, buf, pos, len(data) - pos, target)
        if r <= 0:
            break
        pages.append((r, used, out))
        pos += used
        if pos >= len(data) or used == 0:
            break
    return pages


def main():
    L = load_reference()
    out = {}
    for key, name, sizes in PC.singles():
        data = PC.input_bytes(name)
        buf = (C.c_uint8 * (len(data) + 64)).from_buffer_copy(data + bytes(64))
        out[key] = series_of([dest_size(L, buf, 0, len(data), t) for t in sizes])
    for name, t in PC.CHAINS:
        out[PC.chain_key(name, t)] = series_of(chain(L, PC.input_bytes(name), t))
    path = os.path.join(HERE, "pages_vectors.json")
    with open(path, "w") as f:
        f.write("{\n")
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(out[k], sort_keys=True, separators=(",", ":"))) for k in sorted(out)))
        f.write("\n}\n")
    print("%s: %d series, %d pages, %d bytes" % (path, len(out), sum(len(v["ret"]) for v in out.values()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
