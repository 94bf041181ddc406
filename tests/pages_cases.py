"""The inputs and the grid of the fixed-size page tests (mi355lz4_compress_pages_device), rebuilt from seeds.
tests/golden/make_pages_golden.py runs the reference's LZ4_compress_destSize over exactly these (tests/golden/pages_vectors.json
holds its return values, consumed counts and truncated sha256 sums, no input bytes); tests/native/fill_model.c is the model the
GPU is compared with byte by byte.

The grid.
  grid/   five inputs of 2048 bytes -- zeros, random bytes, word text, a period-7 string, and 300 random + 700 zeros + 1048 text --
          against every pageSize in 0..600; zeros of 65000 and of 70000 bytes against every pageSize in 1..600 (shortened matches
          with length fields of 1 to 270 bytes, on both table types)
  seam/   word text of 65546, 65547 and 65548 bytes at pageSize 4096 and 60000: LZ4_64Klimit, where the table type changes
  bound/  lengths 0, 1, 12, 13, 14, 100, 2048, each at compressBound(n) - 1, compressBound(n) and compressBound(n) + 1: the
          branch that hands over to the unlimited encoder
  chains  2048 text bytes at pageSize 1, 2, 3, 16, 64, 256 and 4096; 70000 text bytes at pageSize 4096, where the table type
          changes inside the chain

Test infrastructure only (imported by tests, like dict_cases.py).
"""
import numpy as np

from dict_cases import text

_CACHE = {}


def compress_bound(n):
    return n + n // 255 + 16


def _build(name):
    kind, n = name.rstrip("0123456789"), int(name[len(name.rstrip("0123456789")):])
    if kind == "zeros":
        return bytes(n)
    if kind == "random":
        return np.random.RandomState(7100 + n).randint(0, 256, size=n).astype(np.uint8).tobytes()
    if kind == "text":
        if n in (65546, 65547, 65548):  # the seam: prefixes of ONE text, so that only the table type tells them apart
            return text(7200000 + 65548, 65548)[:n]
        return text(7200000 + n, n)
    if kind == "period":                 # period 7
        unit = np.random.RandomState(7300).randint(0, 256, size=7).astype(np.uint8).tobytes()
        return (unit * (n // 7 + 1))[:n]
    if kind == "mixed":
        assert n == 2048
        return _build("random300") + bytes(700) + _build("text1048")
    raise KeyError(name)


def input_bytes(name):
    """the input called `name`: <kind><length>"""
    if name not in _CACHE:
        _CACHE[name] = _build(name)
    return _CACHE[name]


GRID_SMALL = ("zeros2048", "random2048", "text2048", "period2048", "mixed2048")
GRID_LONG = ("zeros65000", "zeros70000")
SEAM = ("text65546", "text65547", "text65548")
BOUND_LENS = (0, 1, 12, 13, 14, 100, 2048)


def singles():
    """[(series name, input name, [pageSize, ...])]: every entry is one LZ4_compress_destSize call (maxPages == 1)"""
    s = [("grid/" + name, name, list(range(0, 601))) for name in GRID_SMALL]
    s += [("grid/" + name, name, list(range(1, 601))) for name in GRID_LONG]
    s += [("seam/" + name, name, [4096, 60000]) for name in SEAM]
    s += [("bound/text%d" % n, "text%d" % n, [compress_bound(n) - 1, compress_bound(n), compress_bound(n) + 1]) for n in BOUND_LENS]
    return s


CHAINS = [("text2048", t) for t in (1, 2, 3, 16, 64, 256, 4096)] + [("text70000", 4096)]


def chain_key(name, page_size):
    return "chain/%s/%d" % (name, page_size)


def min_progress(t):
    """what a page of pageSize t that leaves input behind consumes at the least: the all-literals page"""
    return (t - 1) - (t + 240) // 256
