"""The argument contracts of the device compress calls, walked through all of them on live engines.

The block batches: mi355lz4_compress_batch_device, _streams_device, _dict_device, _hcdict_device, _fastdict_device,
_fastdict_multi_device and _streams_fast_device share one contract (api.cpp, batch_shape_check / dict_batch_shape_check /
batch_buffers_check) and differ in what the table CALLS says: the largest block, the words of the limit, what comes in front of the
shape (the stream table, the level).  The pages: mi355lz4_compress_pages_device, _pages_fast_device and _pages_fastdict_device share
another (api.cpp, pages_check), PAGE_CALLS.  In both the first failing check wins.  Every row is an error or the empty call: no kernel
is launched, and the outputs keep their pattern.  The rows that tests/native/hcdict_args_main.cpp already pins for the HC dictionary
call (its own block limit, the empty call, the null pointers, the short stride without checksums) are not repeated for it;
tests/native/dict_args_main.cpp and the _host suites stop at the null engine and the null set."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, E_ARG, E_CAPACITY = 0, -3, -4
N, LEN, KIND = 2, 64, 8
MAX_INPUT = 0x7E000000                # MI355LZ4_MAX_INPUT_SIZE
FILL = 0xA5
_i32p = C.POINTER(C.c_int32)

DICT_LIMIT = 4 << 20                  # HCDICT_MAX_BLOCK
# call -> (who, the largest maxBlockLen it takes, what nBlocks -1 says, what takes the bytes of a block above a dictionary call's
# limit (None: the limit is MI355LZ4_MAX_INPUT_SIZE, and above it the arguments are "bad"), (a level the call refuses, what it says))
CALLS = {
    "batch": ("compress_batch_device", MAX_INPUT, "bad arguments", None, None),
    "streams": ("compress_streams_device", MAX_INPUT, "bad stream table", None,       # the stream table is checked in front
                (9, "compression level 9; exact streams are level 0's encoder")),
    "dict": ("compress_dict_device", MAX_INPUT, "bad arguments", None, (9, "compression level 9; the dictionary batch is level 0's encoder")),
    "hcdict": ("compress_hcdict_device", DICT_LIMIT, "bad arguments", "a dictionary batch",
               (0, "compression level 0; level 0 against a dictionary is mi355lz4_compress_dict_device")),
    "fastdict": ("compress_fastdict_device", DICT_LIMIT, "bad arguments", "a dictionary batch",
                 (9, "compression level 9; levels 1..12 against a dictionary are mi355lz4_compress_hcdict_device")),
    "fastdict_multi": ("compress_fastdict_multi_device", DICT_LIMIT, "bad arguments", "a dictionary batch",
                       (9, "compression level 9; a dictionary set is level 0's encoder")),
    "streams_fast": ("compress_streams_fast_device", DICT_LIMIT, "bad stream table", "a fast stream's block",
                     (9, "compression level 9; fast streams are level 0's encoder")),
}
LEVEL = {"hcdict": 9}                 # the level a call's engine runs at (the others: 0)
PINNED_ELSEWHERE = {"hcdict": {"over_limit", "empty", "null_src", "null_slots", "null_framed_len", "short_stride"}}
ONLY = {"wrong_level": {k for k, v in CALLS.items() if v[4]}, "wrong_level_and_header_kind_5": {k for k, v in CALLS.items() if v[4]},
        "null_dict_idx": {"fastdict_multi"}, "null_dict_idx_and_src": {"fastdict_multi"}}


@pytest.fixture(scope="module")
def calls():
    """one engine per call, and device buffers for 2 blocks of 64 bytes; every entry is call(**overrides) -> (code, message)"""
    import torch
    import streamly_lz4_amd as S
    L, P = S.lib, S._dptr
    need = S.compress_bound(LEN) + KIND           # (slot_stride_ex rounds up: the bound itself is the limit)
    src = torch.full((N * LEN,), 7, dtype=torch.uint8, device=DEV)
    slots = torch.full((N * (need + 4),), FILL, dtype=torch.uint8, device=DEV)
    flen = torch.full((N,), -77, dtype=torch.int32, device=DEV)
    first, slot0 = (C.c_int32 * 2)(0, N), (C.c_int32 * 1)(0)
    empty_first = (C.c_int32 * 1)(0)
    idx = torch.zeros((N,), dtype=torch.int32, device=DEV)
    engines = {k: S.Engine(0) for k in CALLS}
    for k, level in LEVEL.items():
        engines[k].set_compression_level(level)
    cs = {k: S.CompressStreams(engines[k], 1) for k in ("streams", "dict")}
    fs = S.FastCompressStreams(engines["streams_fast"], 1)
    hd = {k: S.HcDict(engines[k]) for k in ("hcdict", "fastdict", "fastdict_multi")}
    dset = S.DictSet(engines["fastdict_multi"], [hd["fastdict_multi"]])

    def make(kind_of_call):
        eng = engines[kind_of_call]

        def call(nb=N, kind=KIND, mx=LEN, src=src, slots=slots, stride=need, flen=flen, checksum=False, level=None, idx=idx):
            eng.set_block_checksum(checksum)
            if level is not None:
                eng.set_compression_level(level)
            try:
                a = (P(src), None, None, LEN, mx, nb)
                b = (kind, P(slots), stride, P(flen))
                f, ns = (first, 1) if nb != 0 else (empty_first, 0)
                table = (C.cast(f, _i32p), C.cast(slot0, _i32p), ns)
                if kind_of_call == "batch":
                    rc = L.mi355lz4_compress_batch_device(eng.ctx, *a, 1, *b)
                elif kind_of_call == "streams":
                    rc = L.mi355lz4_compress_streams_device(eng.ctx, cs["streams"]._h, *a, *table, 1, *b)
                elif kind_of_call == "dict":
                    rc = L.mi355lz4_compress_dict_device(eng.ctx, cs["dict"]._h, 0, *a, 1, *b)
                elif kind_of_call == "hcdict":
                    rc = L.mi355lz4_compress_hcdict_device(eng.ctx, hd["hcdict"]._h, *a, *b)
                elif kind_of_call == "fastdict":
                    rc = L.mi355lz4_compress_fastdict_device(eng.ctx, hd["fastdict"]._h, *a, 1, *b)
                elif kind_of_call == "fastdict_multi":
                    rc = L.mi355lz4_compress_fastdict_multi_device(eng.ctx, dset._h, P(idx), *a, 1, *b)
                else:
                    rc = L.mi355lz4_compress_streams_fast_device(eng.ctx, fs._h, *a, *table, 1, *b)
                return rc, (L.mi355lz4_last_error() or b"").decode()
            finally:
                eng.set_block_checksum(False)
                eng.set_compression_level(LEVEL.get(kind_of_call, 0))
        return call

    yield {k: make(k) for k in CALLS}, need, slots, flen
    for e in engines.values():
        e.synchronize()
    assert (slots == FILL).all() and (flen == -77).all(), "an argument error or an empty call wrote an output"
    dset.close()
    for h in hd.values():
        h.close()
    fs.close()
    for c in cs.values():
        c.close()
    for e in engines.values():
        e.close()


def rows(who, limit, negative_count, need, takes=None, refused=None):
    """row -> (overrides, code, message): the parent's wording, the order in which its checks win"""
    bad = "%s: bad arguments" % who
    over = bad if takes is None else "%s: maxBlockLen %d above the %d bytes %s takes" % (who, limit + 1, limit, takes)
    level, says = refused or (None, "")
    return {
        "wrong_level": (dict(level=level), E_ARG, "%s: %s" % (who, says)),
        "wrong_level_and_header_kind_5": (dict(level=level, kind=5), E_ARG, "%s: %s" % (who, says)),      # the level is looked at first
        "null_dict_idx": (dict(idx=None), E_ARG, "%s: null dictIdx" % who),
        "null_dict_idx_and_src": (dict(idx=None, src=None), E_ARG, "%s: null dictIdx" % who),     # ... in front of the buffers
        "header_kind_5": (dict(kind=5), E_ARG, bad),
        "negative_block_len": (dict(mx=-1), E_ARG, bad),
        "over_limit": (dict(mx=limit + 1), E_ARG, over),
        "negative_count": (dict(nb=-1), E_ARG, "%s: %s" % (who, negative_count)),
        "empty": (dict(nb=0, src=None, slots=None, flen=None), OK, None),
        "null_src": (dict(src=None), E_ARG, "%s: null src" % who),
        "null_slots": (dict(slots=None), E_ARG, "%s: null output" % who),
        "null_framed_len": (dict(flen=None), E_ARG, "%s: null output" % who),
        "short_stride": (dict(stride=need - 1), E_CAPACITY, "%s: slotStride %d < bound" % (who, need - 1)),
        "short_stride_with_checksums": (dict(stride=need + 3, checksum=True), E_CAPACITY, "%s: slotStride %d < bound" % (who, need + 3)),
        "two_faults": (dict(kind=5, stride=need - 1), E_ARG, bad),       # the header kind is looked at first
    }


CASES = [(which, row) for which in sorted(CALLS) for row in sorted(rows("x", 0, "x", 0))
         if row not in PINNED_ELSEWHERE.get(which, ()) and which in ONLY.get(row, CALLS)]


@pytest.mark.parametrize("which,row", CASES)
def test_contract(calls, which, row):
    table, need, _, _ = calls
    who, limit, negative_count, takes, refused = CALLS[which]
    overrides, code, message = rows(who, limit, negative_count, need, takes, refused)[row]
    rc, said = table[which](**overrides)
    assert rc == code, (which, row, rc, said)
    if message is not None:
        assert said == message, (which, row)


# ---- the page calls: 2 inputs of 64 bytes, 2 pages each ----
MAX_PAGES, PAGE = 2, 32
# call -> (who, the kind of pages in the level's message; None: the exact form takes any level)
PAGE_CALLS = {
    "pages": ("compress_pages_device", None),
    "pages_fast": ("compress_pages_fast_device", "fast"),
    "pages_fastdict": ("compress_pages_fastdict_device", "dictionary"),
}
PAGE_POINTERS = ("src", "src_off", "src_len", "page_size", "pages", "page_src_len", "page_comp_len", "n_pages", "consumed")


@pytest.fixture(scope="module")
def page_calls():
    """one engine per call; every entry is call(**overrides) -> (code, message)"""
    import torch
    import streamly_lz4_amd as S
    L, P = S.lib, S._dptr
    stride = KIND + PAGE
    i32 = lambda n, v: torch.full((n,), v, dtype=torch.int32, device=DEV)      # noqa: E731
    bufs = dict(src=torch.full((N * LEN,), 7, dtype=torch.uint8, device=DEV),
                src_off=torch.tensor([0, LEN], dtype=torch.int64, device=DEV), src_len=i32(N, LEN), page_size=i32(N, PAGE),
                pages=torch.full((N * MAX_PAGES * stride,), FILL, dtype=torch.uint8, device=DEV),
                page_src_len=i32(N * MAX_PAGES, -77), page_comp_len=i32(N * MAX_PAGES, -77), n_pages=i32(N, -77), consumed=i32(N, -77))
    outputs = ("pages", "page_src_len", "page_comp_len", "n_pages", "consumed")
    engines = {k: S.Engine(0) for k in PAGE_CALLS}
    hd = S.HcDict(engines["pages_fastdict"])

    def make(kind_of_call):
        eng = engines[kind_of_call]

        def call(ni=N, max_pages=MAX_PAGES, kind=KIND, stride=stride, checksum=False, level=0, null=()):
            p = {k: (None if k in null else P(v)) for k, v in bufs.items()}
            eng.set_block_checksum(checksum)
            eng.set_compression_level(level)
            try:
                a = (p["src"], p["src_off"], p["src_len"], ni, p["page_size"], max_pages)
                b = (kind, p["pages"], stride, p["page_src_len"], p["page_comp_len"], p["n_pages"], p["consumed"])
                if kind_of_call == "pages":
                    rc = L.mi355lz4_compress_pages_device(eng.ctx, *a, *b)
                elif kind_of_call == "pages_fast":
                    rc = L.mi355lz4_compress_pages_fast_device(eng.ctx, *a, 1, *b)
                else:
                    rc = L.mi355lz4_compress_pages_fastdict_device(eng.ctx, hd._h, *a, 1, *b)
                return rc, (L.mi355lz4_last_error() or b"").decode()
            finally:
                eng.set_block_checksum(False)
                eng.set_compression_level(0)
        return call

    yield {k: make(k) for k in PAGE_CALLS}
    for e in engines.values():
        e.synchronize()
    assert (bufs["pages"] == FILL).all() and all((bufs[k] == -77).all() for k in outputs[1:]), "an argument error or an empty call wrote an output"
    hd.close()
    for e in engines.values():
        e.close()


def page_rows(who, fast_kind):
    """row -> (overrides, code, message), in the order in which the checks win: the arguments, the checksums, the level (the wave
    encoder's two forms), the empty call, the pointers"""
    bad = "%s: bad arguments" % who
    sums = "%s: block checksums are on; pages carry no trailer" % who
    level = "%s: compression level 9; %s pages are level 0's encoder" % (who, fast_kind)
    null = "%s: null pointer" % who
    out = {
        "negative_count": (dict(ni=-1), E_ARG, bad),
        "max_pages_0": (dict(max_pages=0), E_ARG, bad),
        "short_stride": (dict(stride=KIND), E_ARG, bad),               # no room for the header and one byte
        "checksums_on": (dict(checksum=True), E_ARG, sums),
        "empty": (dict(ni=0, null=PAGE_POINTERS), OK, None),
        "empty_with_checksums": (dict(ni=0, checksum=True), E_ARG, sums),                # the empty call comes behind the switches
        "bad_kind_and_checksums": (dict(kind=5, checksum=True), E_ARG, bad),
        "checksums_and_null_pointer": (dict(checksum=True, null=("src",)), E_ARG, sums),
    }
    for kind in (-4, 1, 2, 5, 12):
        out["header_kind_%s" % str(kind).replace("-", "minus_")] = (dict(kind=kind), E_ARG, bad)
    for name in PAGE_POINTERS:
        out["null_" + name] = (dict(null=(name,)), E_ARG, null)
    if fast_kind:
        out["level_9"] = (dict(level=9), E_ARG, level)
        out["checksums_and_level_9"] = (dict(checksum=True, level=9), E_ARG, sums)
        out["level_9_and_null_pointer"] = (dict(level=9, null=("pages",)), E_ARG, level)
        out["empty_at_level_9"] = (dict(ni=0, level=9), E_ARG, level)
    return out


PAGE_CASES = [(which, row) for which in sorted(PAGE_CALLS) for row in sorted(page_rows(*PAGE_CALLS[which]))]


@pytest.mark.parametrize("which,row", PAGE_CASES)
def test_page_contract(page_calls, which, row):
    overrides, code, message = page_rows(*PAGE_CALLS[which])[row]
    rc, said = page_calls[which](**overrides)
    assert rc == code, (which, row, rc, said)
    if message is not None:
        assert said == message, (which, row)
