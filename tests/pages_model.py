"""tests/native/fill_model.c -- the CPU restatement of LZ4_compress_destSize -- built with gcc and called through ctypes, plus the
golden's accessors.  Test infrastructure only (imported by tests, like dict_model.py)."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "fill_model.c")
RULES = ("none", "literal rewind", "token rewind", "shortened match", "adapted last run")
SHA_DIGITS = 6

_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)
_LIB = None
_GOLDEN = None


def available():
    return shutil.which("gcc") is not None


def lib():
    """the model as a shared object in a directory of this process's own"""
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="fillmodel")
        so = os.path.join(d, "libfillmodel.so")
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", so, SRC])
        L = C.CDLL(so)
        L.fill_model_page.restype = C.c_int
        L.fill_model_page.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.fill_model_chain.restype = C.c_int
        L.fill_model_chain.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, _i32p, _i32p, _i32p, _i32p]
        _LIB = L
    return _LIB


def as_array(data):
    return data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)


def page(data, target, pos=0, n=None):
    """one LZ4_compress_destSize call on data[pos : pos + n]: (ret, used, rule, the bytes written)"""
    a = as_array(data)
    if n is None:
        n = len(data) - pos
    dst = np.zeros(max(target, 1), dtype=np.uint8)
    used, rule = C.c_int(), C.c_int()
    r = lib().fill_model_page(a.ctypes.data + pos, n, dst.ctypes.data, target, C.byref(used), C.byref(rule))
    return r, used.value, rule.value, dst[:max(r, 0)].tobytes()


def chain(data, page_size, max_pages, header_kind=0):
    """the chain of one input as the device call lays it out: ([(page bytes with header, compLen, srcLen, rule)], consumed)"""
    a = as_array(data)
    n = len(data)
    stride = header_kind + max(page_size, 1)
    pages = np.zeros(max_pages * stride, dtype=np.uint8)
    sl, cl, ru = (np.zeros(max_pages, dtype=np.int32) for _ in range(3))
    cons = C.c_int32()
    k = lib().fill_model_chain(a.ctypes.data, n, page_size, max_pages, header_kind, pages.ctypes.data, stride,
                               sl.ctypes.data_as(_i32p), cl.ctypes.data_as(_i32p), ru.ctypes.data_as(_i32p), C.byref(cons))
    out = [(pages[j * stride: j * stride + header_kind + int(cl[j])].tobytes(), int(cl[j]), int(sl[j]), int(ru[j])) for j in range(k)]
    return out, cons.value


def sha(b):
    return hashlib.sha256(b).hexdigest()[:SHA_DIGITS]


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with open(os.path.join(ROOT, "tests", "golden", "pages_vectors.json")) as f:
            _GOLDEN = json.load(f)
    return _GOLDEN


def golden_pages(key):
    """[(ret, used, sha)] of one series"""
    g = golden()[key]
    return [(r, u, g["sha"][SHA_DIGITS * i: SHA_DIGITS * (i + 1)]) for i, (r, u) in enumerate(zip(g["ret"], g["used"]))]
