"""The batch argument contract of the four device compress calls, walked through all of them on live engines:
mi355lz4_compress_batch_device, mi355lz4_compress_streams_device, mi355lz4_compress_dict_device and mi355lz4_compress_hcdict_device
share it (api.cpp, batch_shape_check / batch_buffers_check) and differ in what the table below says.  Every row is an error or the
empty call: no kernel is launched, and the outputs keep their pattern.  The rows that tests/native/hcdict_args_main.cpp already pins
for the HC dictionary call (its own block limit, the empty call, the null pointers, the short stride without checksums) are not
repeated for it; tests/native/dict_args_main.cpp and the two _host suites stop at the null engine and the null set."""
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

# call -> (who, the largest maxBlockLen it takes, what nBlocks -1 says)
CALLS = {
    "batch": ("compress_batch_device", MAX_INPUT, "bad arguments"),
    "streams": ("compress_streams_device", MAX_INPUT, "bad stream table"),       # the stream table is checked in front
    "dict": ("compress_dict_device", MAX_INPUT, "bad arguments"),
    "hcdict": ("compress_hcdict_device", 4 << 20, "bad arguments"),
}
PINNED_ELSEWHERE = {"hcdict": {"over_limit", "empty", "null_src", "null_slots", "null_framed_len", "short_stride"}}


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
    engines = {k: S.Engine(0) for k in CALLS}
    engines["hcdict"].set_compression_level(9)
    cs = {k: S.CompressStreams(engines[k], 1) for k in ("streams", "dict")}
    hd = S.HcDict(engines["hcdict"])

    def make(kind_of_call):
        eng = engines[kind_of_call]

        def call(nb=N, kind=KIND, mx=LEN, src=src, slots=slots, stride=need, flen=flen, checksum=False):
            eng.set_block_checksum(checksum)
            try:
                a = (P(src), None, None, LEN, mx, nb)
                b = (kind, P(slots), stride, P(flen))
                if kind_of_call == "batch":
                    rc = L.mi355lz4_compress_batch_device(eng.ctx, *a, 1, *b)
                elif kind_of_call == "streams":
                    f, ns = (first, 1) if nb != 0 else (empty_first, 0)
                    rc = L.mi355lz4_compress_streams_device(eng.ctx, cs["streams"]._h, *a, C.cast(f, _i32p), C.cast(slot0, _i32p), ns, 1, *b)
                elif kind_of_call == "dict":
                    rc = L.mi355lz4_compress_dict_device(eng.ctx, cs["dict"]._h, 0, *a, 1, *b)
                else:
                    rc = L.mi355lz4_compress_hcdict_device(eng.ctx, hd._h, *a, *b)
                return rc, (L.mi355lz4_last_error() or b"").decode()
            finally:
                eng.set_block_checksum(False)
        return call

    yield {k: make(k) for k in CALLS}, need, slots, flen
    for e in engines.values():
        e.synchronize()
    assert (slots == FILL).all() and (flen == -77).all(), "an argument error or an empty call wrote an output"
    hd.close()
    for c in cs.values():
        c.close()
    for e in engines.values():
        e.close()


def rows(who, limit, negative_count, need):
    """row -> (overrides, code, message): the parent's wording, the order in which its checks win"""
    bad = "%s: bad arguments" % who
    return {
        "header_kind_5": (dict(kind=5), E_ARG, bad),
        "negative_block_len": (dict(mx=-1), E_ARG, bad),
        "over_limit": (dict(mx=limit + 1), E_ARG, bad),
        "negative_count": (dict(nb=-1), E_ARG, "%s: %s" % (who, negative_count)),
        "empty": (dict(nb=0, src=None, slots=None, flen=None), OK, None),
        "null_src": (dict(src=None), E_ARG, "%s: null src" % who),
        "null_slots": (dict(slots=None), E_ARG, "%s: null output" % who),
        "null_framed_len": (dict(flen=None), E_ARG, "%s: null output" % who),
        "short_stride": (dict(stride=need - 1), E_CAPACITY, "%s: slotStride %d < bound" % (who, need - 1)),
        "short_stride_with_checksums": (dict(stride=need + 3, checksum=True), E_CAPACITY, "%s: slotStride %d < bound" % (who, need + 3)),
        "two_faults": (dict(kind=5, stride=need - 1), E_ARG, bad),       # the header kind is looked at first
    }


CASES = [(which, row) for which in sorted(CALLS) for row in sorted(rows("x", 0, "x", 0)) if row not in PINNED_ELSEWHERE.get(which, ())]


@pytest.mark.parametrize("which,row", CASES)
def test_contract(calls, which, row):
    table, need, _, _ = calls
    who, limit, negative_count = CALLS[which]
    overrides, code, message = rows(who, limit, negative_count, need)[row]
    rc, said = table[which](**overrides)
    assert rc == code, (which, row, rc, said)
    if message is not None:
        assert said == message, (which, row)
