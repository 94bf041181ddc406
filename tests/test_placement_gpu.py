"""Every device call with its blocks placed anywhere, beyond 4 GiB too (include/mi355lz4.h, "Where a call's regions may lie").

tests/placement.py lays a call's regions out in four ways inside far buffers of 2^31 + 2^32 + 2^27 bytes: "dense" (the control),
"permuted" (starts not monotonic: a block below its predecessor, one below the call's first block), "far" (regions near 0,
straddling and above 2^31, straddling and above 2^32) and "far_permuted" (a block more than 2^32 bytes from its predecessor).
Every call runs under all four.  Expected codes and bytes always come from the oracle, never from the dense run; outputs lie in
guard windows with equal windows at every 32-bit alias of the region, and at every alias of an input lies other valid input.
The encoders' bytes must also be the same under all four layouts.  tests/test_placement.py pins the helper and the layouts
used here without a GPU.

A linked device call has no argument for a caller's dictionary: what is in force before a call's first block reaches the
device API as the seam of mi355lz4_decompress_linked_begin (lookBack = 1), as a dstreams slot or as the dictionary of
mi355lz4_decompress_dict_device -- those three are what run here with that dictionary far away."""
import ctypes as C
import random

import numpy as np
import pytest

import confinement_cases as CC
import dstreams_model as DM
import guarded as G
import lz4_synth as SY
import placement as P
from conftest import DECODERS
from test_parity_gpu import LINKED_VARIANTS, split_blocks
from test_write_confinement_gpu import ENCODERS, _linked_expect, _slot_check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = list(P.MODES)
# The fixed-stride forms: 20 strides of 2^28 and a little are 4.75 GiB behind the pointer, which the view behind a front pad of
# 2^31 (4.125 GiB) does not hold.  Those calls get the same allocation with a front pad of 2^30: every zero-extended alias and
# the sign-extended ones of slots / blocks 12.. still lie inside it; those of 8..11 would not (the kernels form these products in
# size_t / uint64_t: kernels/encode.inc, checksum.inc, compact.inc).
WIDE = P.Space(32, front=1 << 30)
STRIDE_SLOT = (1 << 28) + 37
STRIDE_BLOCK = (1 << 28) + 5
DSLOTS, DSLOT_BYTES = 65600, 65600     # more than 65 472 slots: state past 2^31 and 2^32 bytes
CSLOTS, CSLOT_BYTES = 52400, 81984     # more than 52 388
ENC_NAMES = ["level0_auto", "level0_noseg", "level0_seg2", "level0_linked", "level1", "level9", "exact", "level1_linked", "level9_linked"]
# the linked hash-chain call (k_encode_hc with the linked switch on): the other kernel that looks at where the predecessor lies
ENC = dict(ENCODERS, level1_linked=dict(level=1, linked=True), level9_linked=dict(level=9, linked=True))


def _t(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _off(starts):
    return _t(np.array(list(starts) + [0], dtype=np.int64))


class _Far:
    def __init__(self):
        self.inp, self.out, self.state = P.new_far(DEV), P.new_far(DEV), P.new_far(DEV)


@pytest.fixture(scope="module")
def far():
    """three far buffers, one per role (input, output, state), allocated once for the file"""
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(0)
    if free < P.MIN_FREE:
        pytest.skip("needs 40 GiB of free device memory")
    f = _Far()
    yield f
    f.inp = f.out = f.state = None
    torch.cuda.empty_cache()


def decoys(datas):
    """for every input another one of the list with another length: the longest shorter one, else the shortest longer one"""
    out = []
    for d in datas:
        shorter = [x for x in datas if len(x) < len(d)]
        longer = [x for x in datas if len(x) > len(d)]
        out.append(max(shorter, key=len) if shorter else (min(longer, key=len) if longer else bytes(len(d) + 1)))
    return out


def put_in(far, mode, datas, residue=1, buf=None, zones=None):
    starts = P.place([len(d) for d in datas], mode, first_residue=residue, zones=zones)
    P.put_inputs(far.inp if buf is None else buf, starts, datas, decoys(datas))
    return starts


def put_out(far, mode, sizes, seed, residue=5):
    starts = P.place(sizes, mode, first_residue=residue)
    win = P.Windows(starts, sizes, seed=seed)
    win.fill(far.out)
    return starts, win


def check_out(far, starts, plan, got, win, what):
    """plan: [(code, bytes)] per block, the oracle's.  Wrong bytes and disturbed windows are reported together: a truncated
    offset shows as both."""
    for i, (code, data) in enumerate(plan):
        assert got[i] == code, (what, i, got[i], code)
    wrong = [i for i, (code, data) in enumerate(plan) if code > 0 and P.read(far.out, starts[i], code) != data]
    count, found = win.violations(far.out)
    assert not wrong and count == 0, (what, "blocks whose bytes differ", wrong, "%d bytes written outside the allowed ranges; (offset, "
                                      "nearest region, distance from its start (<0) or end (>0), value)" % count, found[:8])


def frame8(payload, cap):
    return len(payload).to_bytes(4, "little") + int(cap).to_bytes(4, "little") + payload


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- independent decode ---------------------------------------------------------------------------------------------------------

def indep_cases(oracle):
    """sixteen blocks: oracle-written text / lzsynth of 1 .. 100001 bytes, one of 1 MiB (the workgroup form's 32 KiB segments),
    one with a corrupted payload, and cases of lz4_synth's offset and end families.  Blocks 5, 6 and 11 are the ones the far
    layouts put across 2^31 and 2^32: the long ones."""
    def make():
        def ow(kind, bl):
            d = oracle.gen(kind, (bl + 65535) // 65536, min(bl, 65536), first_block=bl + 1).tobytes()[:bl]
            return CC.DCase("oracle", "%s %d" % (kind, bl), oracle.compress_block(d, 1), bl, bl)
        rng = random.Random(5)
        good = ow("text", 4096)
        while True:
            p = bytearray(good.payload)
            p[rng.randrange(len(p))] ^= 1 << rng.randrange(8)
            if oracle.decompress_block(bytes(p), 4096)[0] < 0:
                break
        bad = CC.DCase("corrupted", "text 4096", bytes(p), 4096, 4096, True)
        syn = [CC.DCase("synth:" + c.family, c.name, c.block, c.cap, None, not c.valid)
               for fam in (SY.offset_family(), SY.end_family()) for c in fam[:: max(1, len(fam) // 4)][:4]]
        return [ow("text", 1), ow("lzsynth", 13), ow("text", 300), ow("lzsynth", 4096), bad, ow("lzsynth", 100001),
                ow("text", 1 << 20)] + syn[:4] + [ow("text", 65536)] + syn[4:]
    return cached("indep", make)


def indep_plan(oracle, kind, capmode):
    """(fixedUncomp, [(outCap or None, bytes the block may write, code, bytes)])"""
    def make():
        cases = indep_cases(oracle)
        fixed = max(c.cap for c in cases) if kind == 4 else 0
        plan = []
        for i, c in enumerate(cases):
            ocap = c.cap + (0, 1, 7, 64)[i % 4] if capmode == "present" else None
            cap = ocap if ocap is not None else (c.cap if kind == 8 else fixed)
            code, dec = oracle.decompress_block(c.payload, cap)
            plan.append((ocap, cap, code, dec))
        return fixed, plan
    return cached(("indep_plan", kind, capmode), make)


def indep_framed(oracle, kind):
    return [len(c.payload).to_bytes(4, "little") + (c.cap.to_bytes(4, "little") if kind == 8 else b"") + c.payload
            for c in indep_cases(oracle)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("capmode", ["absent", "present"])
@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("decoder", DECODERS + [0])
def test_decompress_batch_device(engine, oracle, far, decoder, kind, capmode, mode):
    """decompress_batch_device, every decoder: the oracle's codes and bytes wherever framed blocks and outputs lie; the
    corrupted block gets the oracle's negative code and its neighbours stand."""
    import torch
    fixed, plan = indep_plan(oracle, kind, capmode)
    assert sum(1 for p in plan if p[2] < 0) >= 1 and sum(1 for p in plan if p[2] > 0) >= 10
    framed = indep_framed(oracle, kind)
    n = len(framed)
    boff = put_in(far, mode, framed)
    ooff, win = put_out(far, mode, [p[1] for p in plan], seed=100 + kind)
    res = G.GuardedArray(n, torch.int32, 7, DEV)
    ocap = _t(np.array([p[0] for p in plan], dtype=np.int32)) if capmode == "present" else None
    engine.set_decoder(decoder)
    try:
        engine.decompress_batch_device(P.view(far.inp), P.FAR.view_len, _off(boff), n, P.view(far.out), _off(ooff), res.view,
                                       header_kind=kind, fixed_uncomp=fixed, out_cap=ocap)
        engine.synchronize()
    finally:
        engine.set_decoder(0)
    what = ("decompress_batch_device", decoder, kind, capmode, mode)
    check_out(far, ooff, [(p[2], p[3]) for p in plan], res.view.cpu().tolist(), win, what)
    res.check(what="%r: result[]" % (what,))


# ---- linked decode of one stream ------------------------------------------------------------------------------------------------------

def linked_streams(oracle):
    """{"clean", "corrupted": a reference-written linked stream of 24 text blocks of 64 KiB, every block reaching into its
    predecessor, and the same with one corrupted block in the middle; "big": eight blocks of 1 MiB}, each with the oracle's
    linked decode [(uncompLen, code, bytes or None, code on its own)]"""
    def make():
        out = {}
        raw = oracle.gen("text", 24, 65536, first_block=4242).tobytes()
        fr = oracle.frame_compress(raw, 65536, 1, 8, True)
        blocks = split_blocks(fr)
        rng = random.Random(9)
        start = sum(len(b) for b in blocks[:12]) + 8
        while True:
            bad = bytearray(fr)
            bad[start + rng.randrange(len(blocks[12]) - 8)] ^= 1 << rng.randrange(8)
            if _linked_expect(oracle, bytes(bad))[12][1] < 0:
                break
        big = oracle.frame_compress(oracle.gen("text", 128, 65536, first_block=99).tobytes(), 1 << 20, 1, 8, True)
        for name, f in (("clean", fr), ("corrupted", bytes(bad)), ("big", big)):
            out[name] = (f, _linked_expect(oracle, f))
        assert all(e[3] < 0 < e[1] for e in out["clean"][1][1:]), "a block of the stream decodes without its predecessor"
        assert all(e[3] < 0 < e[1] for e in out["big"][1][1:])
        return out
    return cached("linked", make)


_paths_seen = {}


def linked_call(engine, far, mode, fr, exp, how, what, look_back=0, streams=None, record=None):
    """one linked call over the framed stream(s) `fr` ([(stream, expectation)] when `streams`): how = "one" (linked = 1),
    "streams", "begin_end" (with look_back the first block is the seam: decoded by the oracle, placed between _begin and _end)"""
    import torch
    import streamly_lz4_amd as S_
    blocks = split_blocks(fr)
    lb = 1 if look_back else 0
    n = len(blocks) - lb
    boff = put_in(far, mode, blocks[lb:])
    sizes = [e[0] for e in exp]
    ooff, win = put_out(far, mode, sizes, seed=21)
    res = G.GuardedArray(n, torch.int32, 22, DEV, lead=1)
    vin, vout = P.view(far.inp), P.view(far.out)
    boff_t, ooff_t = _off(boff), _off(ooff)                             # (alive until _end has run: the range keeps the pointers)
    if how == "one":
        engine.decompress_batch_device(vin, P.FAR.view_len, boff_t, n, vout, ooff_t, res.view, linked=True)
    elif how == "streams":
        engine.decompress_streams_device(vin, P.FAR.view_len, boff_t, n, _t(np.array(streams, dtype=np.int32)), len(streams) - 1,
                                         vout, ooff_t, res.view)
    else:
        seam = exp[0][2] if lb else None
        before = None
        if lb:
            res.all[0] = len(seam)
            before = P.read(far.out, ooff[0], sizes[0])
        engine.decompress_linked_begin(vin, P.FAR.view_len, boff_t, n, vout, ooff_t, res.all if lb else res.view, lb)
        engine.synchronize()
        if lb:                                                          # _begin reads and writes nothing of the seam's slot
            assert P.read(far.out, ooff[0], sizes[0]) == before, (what, "the seam's slot was written by _begin")
            P._store(far.out, ooff[0] + P.FAR.front, seam)
        engine.decompress_linked_end_last()
        engine.decompress_linked_end()
    engine.synchronize()
    got = res.view.cpu().tolist()
    if lb:
        assert P.read(far.out, ooff[0], len(exp[0][2])) == exp[0][2], (what, "the seam's slot was written")
    check_out(far, ooff[lb:], [(e[1], e[2]) for e in exp[lb:]], got, win, what)
    res.check(lo=-lb, what="%r: result[]" % (what,))
    if record is not None and how == "one":
        st = (C.c_int * 5)()
        S_.lib.mi355lz4_debug_runin_state(engine.ctx, st, None)
        record("placement_linked_paths", {"what": repr(what), "path": int(st[4])})
        # How the call was finished does not depend on the layout.  (Compared with whichever layout ran first in this process:
        # vacuous when one layout is selected alone; and LinkedPath is Pointer for the pointer, replay and serial variants alike,
        # so for those it says little.  The oracle comparison above is what holds every run.)
        seen = _paths_seen.setdefault(what[:-1], (what[-1], int(st[4])))
        assert int(st[4]) == seen[1], (what, "LinkedPath %d, but %d under layout %s" % (st[4], seen[1], seen[0]))


@pytest.fixture(params=list(LINKED_VARIANTS) + ["big_blocks"])
def linked_variant(request, monkeypatch):
    for k, v in LINKED_VARIANTS.get(request.param, {}).items():
        monkeypatch.setenv(k, v)
    if request.param == "big_blocks":
        monkeypatch.delenv("MI355LZ4_LINKED_BIG", raising=False)
    return request.param


@pytest.mark.parametrize("mode", MODES)
def test_linked_decode(engine, oracle, far, record, linked_variant, mode):
    """decompress_batch_device(linked = 1) through every second pass of LINKED_VARIANTS (the run-in decode with pieces of 1 and 3
    among them) and, for the 1 MiB blocks, the big-block path: the clean stream and the one with a corrupted block in the
    middle give the oracle's linked decode, codes and bytes, wherever the blocks lie."""
    streams = linked_streams(oracle)
    for name in (["big"] if linked_variant == "big_blocks" else ["clean", "corrupted"]):
        fr, exp = streams[name]
        linked_call(engine, far, mode, fr, exp, "one", ("linked", linked_variant, name, mode), record=record)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("look_back", [0, 1])
@pytest.mark.parametrize("variant", ["default", "pointer_pass_forced"])
def test_linked_begin_end(engine, oracle, far, monkeypatch, variant, look_back, mode):
    """_begin / _end_last / _end; with lookBack = 1 the first block's dictionary is the seam at outOff[-1], placed by the
    caller wherever the layout puts it -- below the range or 2^32 bytes away."""
    for k, v in LINKED_VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    for name in ("clean", "corrupted"):
        fr, exp = linked_streams(oracle)[name]
        linked_call(engine, far, mode, fr, exp, "begin_end", ("begin_end", variant, look_back, name, mode), look_back=look_back)


def many_streams(oracle):
    """six linked streams of four blocks of 16 KiB, the second block of stream 2 corrupted: (framed, expectation, streamFirst)"""
    def make():
        frs = []
        for s in range(6):
            frs.append(oracle.frame_compress(oracle.gen("text", 4, 16384, first_block=10 * s + 3).tobytes(), 16384, 1, 8, True))
        blk = split_blocks(frs[2])
        bad = bytearray(frs[2])
        bad[len(blk[0]) + 8] = 0x1F                                     # (test_parity_gpu.test_linked_streams_error_is_local)
        frs[2] = bytes(bad)
        exp = [e for fr in frs for e in _linked_expect(oracle, fr)]
        assert any(e[1] < 0 for e in exp) and sum(1 for e in exp if e[3] < 0 < e[1]) >= 12
        return b"".join(frs), exp, [4 * s for s in range(7)]
    return cached("many", make)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", ["default", "pointer_pass_forced", "serial_only"])
def test_decompress_streams_device(engine, oracle, far, monkeypatch, variant, mode):
    for k, v in LINKED_VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    fr, exp, first = many_streams(oracle)
    linked_call(engine, far, mode, fr, exp, "streams", ("streams", variant, mode), streams=first)


# ---- partial decode, dictionary batches, decode streams ----------------------------------------------------------------------------------

def partial_blocks(oracle):
    def make():
        out = []
        for i, bl in enumerate((13, 300, 4096, 5000, 65536, 100001, 20000, 262144)):
            d = oracle.gen(("text", "lzsynth")[i % 2], (bl + 65535) // 65536, min(bl, 65536), first_block=300 + i).tobytes()[:bl]
            out.append((d, frame8(oracle.compress_block(d, 1), bl)))
        return out
    return cached("partial", make)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("decoder", [1, 2, 4])
def test_decompress_partial_device(engine, oracle, far, decoder, mode):
    """targets 0, 1, 4096 and past the end, every block under each: a well-formed block of n bytes gives min(target, n) and the
    prefix of its data (include/mi355lz4.h), and nothing behind the prefix is written"""
    import torch
    blocks = partial_blocks(oracle)
    n = len(blocks)
    engine.set_decoder(decoder)
    try:
        for shift in range(4):
            tg = [(0, 1, 4096, len(d) + 100)[(i + shift) % 4] for i, (d, _) in enumerate(blocks)]
            want = [min(t, len(d)) for t, (d, _) in zip(tg, blocks)]
            boff = put_in(far, mode, [b for _, b in blocks])
            ooff, win = put_out(far, mode, want, seed=30 + shift, residue=shift)
            res = G.GuardedArray(n, torch.int32, 8, DEV)
            engine.decompress_partial_device(P.view(far.inp), P.FAR.view_len, _off(boff), n, P.view(far.out), _off(ooff),
                                             _t(np.array(tg, dtype=np.int32)), res.view)
            engine.synchronize()
            what = ("partial", decoder, mode, shift)
            check_out(far, ooff, [(w, d[:w]) for w, (d, _) in zip(want, blocks)], res.view.cpu().tolist(), win, what)
            res.check(what="%r: result[]" % (what,))
    finally:
        engine.set_decoder(0)


def dict_batch(oracle):
    """a 64 KiB dictionary, another one for its alias, and eight blocks compressed against the first by the reference's
    LZ4_compress_fast_continue on a copy of the loaded stream (tests/dict_model.py)"""
    def make():
        import dict_model as DMod
        text = oracle.gen("text", 4, 65536, first_block=808).tobytes()
        d, other = text[:65536], text[70000:70000 + 60000]
        raws = [text[131072 + 5000 * i:131072 + 5000 * i + n] for i, n in enumerate((4096, 1, 16384, 65536, 13, 4095, 2000, 300))]
        loaded = DMod.model_load(d)
        comps = [DMod.model_compress(loaded, r)[1] for r in raws]
        plan = [oracle.decompress_block(c, len(r), d) for c, r in zip(comps, raws)]
        assert [p[1] for p in plan] == raws
        assert sum(1 for c, r in zip(comps, raws) if oracle.decompress_block(c, len(r)) != (len(r), r)) >= 4, "the blocks do not use the dictionary"
        return d, other, raws, comps, plan
    return cached("dict", make)


def far_zone(mode, n=1):
    """where a call's single far region goes: above 2^32 ("far"), across it ("far_permuted")"""
    return {"far": [4] * n, "far_permuted": [3] + [4] * (n - 1)}.get(mode)


@pytest.mark.parametrize("mode", MODES)
def test_decompress_dict_device(engine, oracle, far, mode):
    """decompress_dict_device with the dictionary itself far away (above 2^32, or across it) and another dictionary at its alias"""
    import torch
    d, other, raws, comps, plan = dict_batch(oracle)
    dstart = P.place([len(d)], mode, first_residue=3, zones=far_zone(mode))[0]
    P.put_inputs(far.state, [dstart], [d], [other])
    framed = [frame8(c, len(r)) for c, r in zip(comps, raws)]
    n = len(framed)
    boff = put_in(far, mode, framed)
    ooff, win = put_out(far, mode, [len(r) for r in raws], seed=40)
    res = G.GuardedArray(n, torch.int32, 9, DEV)
    engine.decompress_dict_device(P.view(far.inp), P.FAR.view_len, _off(boff), n, P.view(far.state)[dstart:], len(d), P.view(far.out),
                                  _off(ooff), res.view)
    engine.synchronize()
    check_out(far, ooff, plan, res.view.cpu().tolist(), win, ("decompress_dict_device", mode))
    res.check(what="dict: result[]")
    assert P.read(far.state, dstart, len(d)) == d, "the dictionary was written"


@pytest.fixture(scope="module")
def dset(far, engine):
    """a dstreams set whose state passes 2^31 and 2^32 bytes"""
    import streamly_lz4_amd as S_
    assert DSLOTS * DSLOT_BYTES > (1 << 32) and DSLOT_BYTES == 65600
    ds = S_.DecompressStreams(engine, DSLOTS)
    yield ds
    ds.close()


D_SLOTS = [5, 40000, 65500]            # state offsets below 2^31, between the marks and above 2^32


def dstream_streams(oracle):
    def make():
        out = []
        for s in range(3):
            arrays = DM.cut(DM.data(oracle, "text", 4 * 16384, first=s * 777), [16384] * 4)
            st = DM.make_stream(oracle, arrays, 8)
            DM.assert_dependent(oracle, st)
            out.append((st, DM.model(oracle, st)))
        return out
    return cached("dstreams", make)


@pytest.mark.parametrize("mode", MODES)
def test_decompress_dstreams_device(engine, oracle, far, dset, mode):
    """three streams continued over two calls in slots whose state lies below 2^31, between the marks and above 2^32: the model's
    codes and bytes; the slots a truncated state offset would name keep their reset state"""
    import torch
    assert [s * DSLOT_BYTES >> 31 for s in D_SLOTS] == [0, 1, 2]
    streams = dstream_streams(oracle)
    dset.reset()
    trunc = [(s * DSLOT_BYTES) % (1 << 32) // DSLOT_BYTES for s in D_SLOTS[2:]]
    for call in range(2):
        blocks = [b for st, _ in streams for b in st[2 * call:2 * call + 2]]
        plan = [(m[0][i], m[1][i]) for _, m in streams for i in (2 * call, 2 * call + 1)]
        n = len(blocks)
        boff = put_in(far, mode, [b.framed for b in blocks], residue=call)
        ooff, win = put_out(far, mode, [b.cap for b in blocks], seed=50 + call, residue=7 + call)
        res = G.GuardedArray(n, torch.int32, 10, DEV)
        engine.decompress_dstreams_device(dset, P.view(far.inp), P.FAR.view_len, _off(boff), n, [0, 2, 4, 6], D_SLOTS, P.view(far.out),
                                          _off(ooff), res.view)
        engine.synchronize()
        check_out(far, ooff, plan, res.view.cpu().tolist(), win, ("dstreams", mode, call))
        res.check(what="dstreams: result[]")
        win.fill(far.out)                                               # the slot owns its copy: the outputs may go
        for slot, (st, m) in zip(D_SLOTS, streams):
            assert dset.state(slot)[0] == min(65536, len(m[1][2 * call + 1])), (mode, call, slot)
        for slot in trunc + [t + 1 for t in trunc]:
            assert dset.state(slot)[0] == 0, (mode, call, "slot %d was written" % slot)


# ---- scans and small kernels ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("trailers", [False, True])
def test_decoded_size_device(oracle, far, slz4, trailers, mode):
    import torch
    datas = [d for d, _ in partial_blocks(oracle)]
    comps = [oracle.compress_block(d, 1) for d in datas]
    framed = [DM.frame(c, len(d), 4, trailers) for c, d in zip(comps, datas)]
    n = len(framed)
    eng = slz4.Engine(0)
    try:
        eng.set_block_checksum(trailers)
        boff = put_in(far, mode, framed)
        size = G.GuardedArray(n, torch.int32, 11, DEV)
        ooff = G.GuardedArray(n + 1, torch.int64, 12, DEV)
        eng.decoded_size_device(P.view(far.inp), P.FAR.view_len, _off(boff), n, size.view, ooff.view, header_kind=4, max_uncomp=1 << 20)
        eng.synchronize()
        assert size.view.cpu().tolist() == [len(d) for d in datas], (mode, trailers)
        assert ooff.view.cpu().tolist() == np.concatenate([[0], np.cumsum([len(d) for d in datas])]).tolist()
        size.check(what="decoded_size size[]")
        ooff.check(what="decoded_size outOff[]")
    finally:
        eng.close()


INDEX_ULEN = [0x7E000000, 5, 0x7E000000, 0x7E000000, 65536, 0x7E000000, 0x7E000000, 1]
XXH_LENS = (1, 15, 16, 4096, 70001, 17, 3, 100, 1000, 31, 32, 33)      # (blocks 3, 4 and 8 lie across the marks)
INTERLEAVE_SIZES = [1, 15, 16, 4097, 70000, 17, 1000, 16, 70000, 1, 4097, 15]


def index_framed():
    return [frame8(bytes([0x10 + i]) * (60 + i), u) for i, u in enumerate(INDEX_ULEN)]


@pytest.mark.parametrize("mode", MODES)
def test_index_device(engine, far, mode):
    """headers whose uncompLen makes the scan pass 2^31 and 2^32: outOff[] is the uint64 cumulative sum"""
    import torch
    ulen = INDEX_ULEN
    framed = index_framed()
    boff = put_in(far, mode, framed)
    ooff = G.GuardedArray(len(ulen) + 1, torch.int64, 13, DEV)
    engine.index_device(P.view(far.inp), P.FAR.view_len, _off(boff), len(ulen), ooff.view)
    engine.synchronize()
    want = np.concatenate([[0], np.cumsum(np.array(ulen, dtype=np.uint64))]).astype(np.uint64)
    assert int(want[-1]) > (1 << 33)
    assert ooff.view.cpu().numpy().astype(np.uint64).tolist() == want.tolist(), mode
    ooff.check(what="index outOff[]")


@pytest.mark.parametrize("mode", MODES)
def test_xxh32_device(engine, far, slz4, mode):
    import torch
    rng = random.Random(6)
    datas = [rng.randbytes(x) for x in XXH_LENS]
    off = put_in(far, mode, datas)
    out = G.GuardedArray(len(datas), torch.int32, 14, DEV)
    engine.xxh32_device(P.view(far.inp), _off(off), _t(np.array([len(d) for d in datas], dtype=np.int32)), len(datas), 7, out.view)
    engine.synchronize()
    assert out.view.cpu().numpy().astype(np.uint32).tolist() == [slz4.xxh32(d, 7) for d in datas], mode
    out.check(what="xxh32 out[]")


@pytest.mark.parametrize("mode", MODES)
def test_interleave_device(engine, far, mode):
    """rank g's local blocks go to global + globalOff[j * nRanks + g], far and permuted, and nowhere else"""
    rng = random.Random(4)
    n_ranks, n_local = 2, 6
    sizes = INTERLEAVE_SIZES
    goff = P.place(sizes, mode, first_residue=2)
    for rank in range(n_ranks):
        mine = [j * n_ranks + rank for j in range(n_local)]
        datas = [rng.randbytes(sizes[g]) for g in mine]
        loff = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.int64)
        win = P.Windows([goff[g] for g in mine], [sizes[g] for g in mine], seed=60 + rank)
        other = P.Windows([goff[g] for g in range(len(sizes)) if g not in mine], [0] * (len(sizes) - n_local), seed=70 + rank)
        other.fill(far.out)                                             # the other ranks' places: all guard
        win.fill(far.out)
        engine.interleave_device(_t(np.frombuffer(b"".join(datas) + b"\0", dtype=np.uint8).copy()), _t(loff), n_local, rank, n_ranks,
                                 P.view(far.out), _off(goff))
        engine.synchronize()
        for g, d in zip(mine, datas):
            assert P.read(far.out, goff[g], len(d)) == d, (mode, rank, g)
        win.check(far.out, ("interleave", mode, rank))
        if mode in ("far", "far_permuted"):                             # (in the dense layouts the two sets of windows overlap)
            other.check(far.out, ("interleave, the other ranks' places", mode, rank))


@pytest.mark.parametrize("mode", MODES)
def test_compact_device(engine, oracle, far, mode):
    """slotStride 2^28 + 37, 24 slots: seventeen with framedLen just under the stride, then real framed blocks, so that denseOff
    passes 2^32 inside the call.  denseOff[] is the uint64 cumulative sum; the real blocks and two of the padding blocks
    arrive byte for byte; in the far layouts denseCap cuts the stream above 2^32, inside a block, and nothing lies behind the
    last block that fits.  The layouts move where `dense` starts: a compact call has no other freedom."""
    import torch
    n, stride = 24, STRIDE_SLOT
    real = [frame8(oracle.compress_block(d, 1), len(d)) for d, _ in partial_blocks(oracle)[:7]]
    flen = [stride - 40 - 3 * i for i in range(17)] + [len(b) for b in real]
    slots = far.inp                                                     # the whole allocation: 24 strides need 6.0 GiB
    assert (n - 1) * stride + max(flen[17:]) <= P.FAR.total
    for i in (0, 3, 16):                                                # pattern as contents (slot 16's copy crosses 2^32)
        G.fill(slots[i * stride:i * stride + flen[i]], seed=90 + i)
    for i, b in enumerate(real):
        P._store(slots, (17 + i) * stride, b)
    offs = np.concatenate([[0], np.cumsum(np.array(flen, dtype=np.uint64))]).astype(np.uint64)
    assert int(offs[16]) < (1 << 32) < int(offs[17])
    cut = mode in ("far", "far_permuted")
    cap = int(offs[20]) + flen[20] // 2 if cut else int(offs[-1])
    fitted = [i for i in range(n) if int(offs[i + 1]) <= cap]
    assert len(fitted) == (20 if cut else n) and cap > (1 << 32)
    base = {"dense": 0, "permuted": 7, "far": 16, "far_permuted": 1000003}[mode]
    dense = far.out[base:]
    assert base + cap + G.END_GUARD <= P.FAR.total
    end = int(offs[fitted[-1] + 1])
    guard = dense[end:cap + G.END_GUARD]                                # behind the last block that fits, and behind denseCap
    guard[:] = G.pattern(end, guard.numel(), 17, like=dense)
    compared = [0, 3, 16] + [k for k in range(17, n) if k in fitted]
    for i in compared:                                                  # (no stale copy of an earlier run can pass for this one's)
        G.fill(dense[int(offs[i]):int(offs[i + 1])], seed=190 + i)
    doff = G.GuardedArray(n + 1, torch.int64, 18, DEV)
    engine.compact_device(slots, stride, _t(np.array(flen, dtype=np.int32)), n, dense, cap, doff.view)
    engine.synchronize()
    assert doff.view.cpu().numpy().astype(np.uint64).tolist() == offs.tolist(), mode
    doff.check(what="denseOff[]")
    for i in compared:
        assert torch.equal(dense[int(offs[i]):int(offs[i + 1])], slots[i * stride:i * stride + flen[i]]), (mode, i)
    assert torch.equal(guard, G.pattern(end, guard.numel(), 17, like=dense)), (mode, "written behind the last block that fits")


# ---- compress --------------------------------------------------------------------------------------------------------------------------

def enc_blocks(oracle):
    """twenty blocks: confinement_cases.ENC_LENGTHS incompressible and as text, a text block of 100 000 bytes, an incompressible
    one of that length (the call's largest: it fills its slot to the worst case), four more text blocks.  With a fixed
    stride of 2^28 and a little, blocks 8.. lie past 2^31 and blocks 16.. past 2^32; the far layouts put blocks 6 and 13 (far)
    or 7 and 6 (far_permuted) across the marks: long ones."""
    def make():
        assert sorted((0, 1, 12, 65535, 13, 65536, 65537)) == sorted(CC.ENC_LENGTHS)
        out = []
        for nb in (0, 1, 12, 65535, 13, 65536, 65537):                  # ENC_LENGTHS, a long block at 6 and 7 (see below)
            for kind in ("random", "text"):
                out.append(oracle.gen(kind, 2, 65536, first_block=100 + nb)[:nb].tobytes())
        out.append(oracle.gen("text", 2, 65536, first_block=7).tobytes()[:100000])
        out.append(oracle.gen("random", 2, 65536, first_block=8).tobytes()[:100000])
        out += [oracle.gen("text", 1, 65536, first_block=20 + i).tobytes()[:nb] for i, nb in enumerate((4096, 300, 65536, 20000))]
        assert len(out) == 20 and max(len(b) for b in out) == 100000
        return out
    return cached("enc", make)


UNIT = 4                               # a linked compress call's blocks lie back to back in units of four


def src_layout(far, mode, blocks, linked, form):
    """(view of src, srcOff or None, blockStride, per block: its predecessor lies directly in front)"""
    n = len(blocks)
    if form == "blockstride":
        starts = [i * STRIDE_BLOCK for i in range(n)]
        P.put_inputs(far.inp, starts, blocks, decoys(blocks), space=WIDE)
        return P.view(far.inp, WIDE), None, STRIDE_BLOCK, [False] * n
    if linked:
        groups = [blocks[i:i + UNIT] for i in range(0, n, UNIT)]
        joined = [b"".join(g) for g in groups]
        ustarts = put_in(far, mode, joined, residue=9)
        starts = P.units(ustarts, [[len(b) for b in g] for g in groups])
        return P.view(far.inp), starts, 0, [i % UNIT != 0 for i in range(n)]
    return P.view(far.inp), put_in(far, mode, blocks, residue=9), 0, [False] * n


def slot_layout(far, mode, n, need, stride, form):
    """(view of the slots, their starts in it, the windows)"""
    if form == "slotstride":
        starts = [i * STRIDE_SLOT for i in range(n)]
        win = P.Windows(starts, [need] * n, space=WIDE, seed=80)
        win.fill(far.out)
        return P.view(far.out, WIDE), starts, win, STRIDE_SLOT
    base = P.place([n * stride], mode, first_residue=stride % 16, zones=far_zone(mode))[0]
    starts = [base + i * stride for i in range(n)]
    win = P.Windows(starts, [need] * n, seed=81)
    win.fill(far.out)
    return P.view(far.out)[base:], starts, win, stride


_enc_seen = {}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", ["srcoff", "slotstride", "blockstride"])
@pytest.mark.parametrize("encoder", ENC_NAMES)
def test_compress_batch_device(oracle, far, encoder, form, mode):
    """compress_batch_device under every encoder (the linked hash-chain call at levels 1 and 9 included), addressed by srcOff[] from place(), by slotStride = 2^28 + 37 (slots 8.. past
    2^31, 16.. past 2^32; checksums on) and by blockStride = 2^28 + 5 with srcOff NULL: header, bound, the oracle decodes
    every slot (with its predecessor as dictionary only where that lies directly in front), the reference's bytes for
    `exact`, nothing outside the slots, and the same bytes under all four layouts."""
    import torch
    import streamly_lz4_amd as S_
    enc = ENC[encoder]
    blocks = enc_blocks(oracle)
    n, mx = len(blocks), 100000
    checksum = form == "slotstride"
    need = S_.slot_stride_ex(mx, 8, checksum)
    linked = bool(enc.get("linked"))
    eng = S_.Engine(0)
    try:
        eng.set_block_checksum(checksum)
        if "segments" in enc:
            eng.set_segments(enc["segments"])
        if linked:
            eng.set_linked_compress(True)
        if "level" in enc:
            eng.set_compression_level(enc["level"])
        if enc.get("exact"):
            eng.set_compress_exact(True)
        src, soff, bstride, has_prev = src_layout(far, mode, blocks, linked, form)
        slots, sstarts, win, stride = slot_layout(far, mode, n, need, need + 37, form)
        flen = G.GuardedArray(n, torch.int32, 19, DEV)
        eng.compress_batch_device(src, n, mx, slots, stride, flen.view, accel=1, header_kind=8,
                                  src_off=None if soff is None else _off(soff), src_len=_t(np.array([len(b) for b in blocks], dtype=np.int32)),
                                  block_stride=bstride)
        eng.synchronize()
    finally:
        eng.close()
    what = ("compress_batch_device", encoder, form, mode)
    fl = flen.view.cpu().tolist()
    flen.check(what="%r: framedLen[]" % (what,))
    space = WIDE if form == "slotstride" else P.FAR
    assert all(0 < f <= need for f in fl), (what, fl)
    got = [np.frombuffer(P.read(far.out, s, f, space), dtype=np.uint8) for s, f in zip(sstarts, fl)]
    win.check(far.out, what)
    comps, d = [], None
    for i, b in enumerate(blocks):
        if enc.get("exact"):
            dict_bytes = d                                              # one stream, whatever the placement
        else:
            dict_bytes = d if (linked and has_prev[i]) else None
            if linked and not has_prev[i]:
                d = None
        comps.append(_slot_check(oracle, S_, got[i], fl[i], b, 8, checksum, dict_bytes, (what, i, len(b))))
        if len(b) > 0:
            d = b
    if enc.get("exact"):
        from test_exact_compress_gpu import OracleStream
        assert comps == OracleStream().compress(blocks, 1), (what, "not the reference's bytes")
    if linked and form != "blockstride":                                # the predecessors in front were really used ...
        used = [i for i, b in enumerate(blocks) if has_prev[i] and oracle.decompress_block(comps[i], len(b)) != (len(b), b)]
        assert len(used) >= 2, (what, "no block of the call reaches into the block in front of it", used)
    # (... and nowhere else: a unit's first block, and every block of the other calls, was decoded above without a dictionary)
    # The comparison across layouts is with whichever layout ran first in this process: it says nothing when one layout is
    # selected alone.  Every run is compared with the oracle above whatever ran before.
    seen = _enc_seen.setdefault((encoder, form), (mode, comps))
    assert comps == seen[1], (what, "the bytes differ from those under layout %s" % seen[0])


@pytest.fixture(scope="module")
def cset(far, engine):
    """a cstreams set whose state passes 2^31 and 2^32 bytes"""
    import streamly_lz4_amd as S_
    assert CSLOTS * CSLOT_BYTES > (1 << 32) and S_.CompressStreams.SLOT_BYTES == CSLOT_BYTES
    cs = S_.CompressStreams(engine, CSLOTS)
    yield cs
    cs.close()


C_SLOTS = [3, 30000, 52395]            # state offsets below 2^31, between the marks and above 2^32
C_DICT_SLOT = 52398


def _compress_placed(engine, far, mode, blocks, call, what, seed):
    """the common part of the two cstreams calls: src from place(), slots behind one another at a far base; returns the slots'
    compressed bytes after the header checks"""
    import torch
    import streamly_lz4_amd as S_
    n, mx = len(blocks), max(len(b) for b in blocks)
    need = S_.slot_stride_ex(mx, 8, False)
    soff = put_in(far, mode, blocks, residue=seed % 16)
    slots, sstarts, win, stride = slot_layout(far, mode, n, need, need + 37, "srcoff")
    flen = G.GuardedArray(n, torch.int32, seed, DEV)
    call(P.view(far.inp), n, mx, slots, stride, flen.view, _off(soff), _t(np.array([len(b) for b in blocks], dtype=np.int32)))
    engine.synchronize()
    fl = flen.view.cpu().tolist()
    flen.check(what="%r: framedLen[]" % (what,))
    assert all(0 < f <= need for f in fl), (what, fl)
    win.check(far.out, what)
    out = []
    for i, (s, f, b) in enumerate(zip(sstarts, fl, blocks)):
        fr = P.read(far.out, s, f)
        assert int.from_bytes(fr[:4], "little") == f - 8 and int.from_bytes(fr[4:8], "little") == len(b), (what, i)
        out.append(fr[8:])
    return out


@pytest.mark.parametrize("mode", MODES)
def test_compress_streams_device(engine, oracle, far, cset, mode):
    """three exact streams continued over two calls in slots whose state lies below 2^31, between the marks and above 2^32: the
    reference's bytes (OracleStream), which the oracle decodes with the block before as dictionary"""
    from test_exact_compress_gpu import OracleStream
    assert [s * CSLOT_BYTES >> 31 for s in C_SLOTS] == [0, 1, 2]
    cset.reset(C_SLOTS)
    arrays = [DM.cut(DM.data(oracle, "text", 200000, first=s * 501), [65536, 300, 40000, 65536]) for s in range(3)]
    refs = [OracleStream() for _ in arrays]
    # where a slot offset truncated to 32 bits would land: inside slots that no test uses and that stay as _create left them
    alias = sorted({(s * CSLOT_BYTES) % (1 << 32) // CSLOT_BYTES + k for s in C_SLOTS if s * CSLOT_BYTES >= (1 << 32) for k in (0, 1)})
    assert alias == [7, 8] and not set(alias) & set(C_SLOTS + [C_DICT_SLOT])
    fed = [0] * 3
    for c in range(2):
        blocks = [b for a in arrays for b in a[2 * c:2 * c + 2]]
        want = [x for r, a in zip(refs, arrays) for x in r.compress(a[2 * c:2 * c + 2], 1)]
        got = _compress_placed(engine, far, mode, blocks,
                               lambda src, n, mx, slots, stride, fl, soff, slen: engine.compress_streams_device(
                                   cset, src, n, mx, [0, 2, 4, 6], C_SLOTS, slots, stride, fl, src_off=soff, src_len=slen, block_stride=0),
                               ("compress_streams_device", mode, c), 23 + c)
        assert got == want, (mode, c, "not the reference's bytes")
        for k, (slot, a) in enumerate(zip(C_SLOTS, arrays)):            # the true slots moved on (currentOffset, the saved tail) ...
            cur, dsize, saved = cset.state(slot)
            assert cur > fed[k] and saved == min(65536, len(a[2 * c + 1])), (mode, c, slot, cur, dsize, saved)
            fed[k] = cur
        for slot in alias:                                              # ... and the slots at their 32-bit aliases did not
            assert cset.slot_bytes(slot) == bytes(CSLOT_BYTES), (mode, c, "slot %d was written" % slot)
    # (what the reference wrote decodes, block after block)
    comps = [x for r, a in zip([OracleStream() for _ in arrays], arrays) for x in r.compress(a, 1)]
    flat = [b for a in arrays for b in a]
    for i, (cp, b) in enumerate(zip(comps, flat)):
        assert oracle.decompress_block(cp, len(b), flat[i - 1] if i % 4 else None) == (len(b), b)


@pytest.mark.parametrize("mode", MODES)
def test_compress_dict_device(engine, oracle, far, cset, mode):
    """compress_dict_device against a slot above 2^32 bytes of state, loaded from a dictionary that lies far away itself:
    LZ4_loadDict and a copy of the loaded stream per block (tests/dict_model.py), decoded by the oracle with the dictionary"""
    import dict_model as DMod
    d, other, raws, _, _ = dict_batch(oracle)
    assert C_DICT_SLOT * CSLOT_BYTES > (1 << 32)
    dstart = P.place([len(d)], mode, first_residue=11, zones=far_zone(mode))[0]
    P.put_inputs(far.state, [dstart], [d], [other])
    cset.load_dict(C_DICT_SLOT, P.view(far.state)[dstart:], len(d))
    loaded = DMod.model_load(d)
    want = [DMod.model_compress(loaded, r)[1] for r in raws]
    got = _compress_placed(engine, far, mode, raws,
                           lambda src, n, mx, slots, stride, fl, soff, slen: engine.compress_dict_device(
                               cset, C_DICT_SLOT, src, n, mx, slots, stride, fl, src_off=soff, src_len=slen, block_stride=0),
                           ("compress_dict_device", mode), 27)
    assert got == want, (mode, "not the reference's bytes")
    for cp, r in zip(got, raws):
        assert oracle.decompress_block(cp, len(r), d) == (len(r), r)


# ---- what tests/test_placement.py pins without a GPU --------------------------------------------------------------------------------------

def region_lists(oracle):
    """{name: the sizes of the regions a test above hands to placement.place}"""
    out = {}
    for kind in (8, 4):
        out["independent framed %d" % kind] = [len(b) for b in indep_framed(oracle, kind)]
        for cm in ("absent", "present"):
            out["independent out %d %s" % (kind, cm)] = [p[1] for p in indep_plan(oracle, kind, cm)[1]]
    for name, (fr, exp) in linked_streams(oracle).items():
        out["linked framed " + name] = [len(b) for b in split_blocks(fr)]
        out["linked out " + name] = [e[0] for e in exp]
    fr, exp, _ = many_streams(oracle)
    out["streams framed"] = [len(b) for b in split_blocks(fr)]
    out["streams out"] = [e[0] for e in exp]
    out["partial framed"] = [len(b) for _, b in partial_blocks(oracle)]
    for shift in range(4):
        out["partial out, shift %d" % shift] = [min((0, 1, 4096, len(d) + 100)[(i + shift) % 4], len(d)) for i, (d, _) in enumerate(partial_blocks(oracle))]
    for tr in (False, True):
        out["decoded_size framed, trailers %s" % tr] = [len(oracle.compress_block(d, 1)) + 4 + 4 * tr for d, _ in partial_blocks(oracle)]
    out["index framed"] = [len(b) for b in index_framed()]
    out["xxh32 ranges"] = list(XXH_LENS)
    out["interleave global"] = list(INTERLEAVE_SIZES)
    arrays = [[65536, 300, 40000, 65536]] * 3
    for c in range(2):
        out["compress_streams src, call %d" % c] = [n for a in arrays for n in a[2 * c:2 * c + 2]]
    d, other, raws, comps, _ = dict_batch(oracle)
    out["dict framed"] = [len(c) + 8 for c in comps]
    out["dict out"] = [len(r) for r in raws]
    st = dstream_streams(oracle)
    out["dstreams framed"] = [len(b.framed) for s, _ in st for b in s[:2]]
    out["dstreams out"] = [b.cap for s, _ in st for b in s[:2]]
    blocks = enc_blocks(oracle)
    out["compress src"] = [len(b) for b in blocks]
    out["compress src, linked units"] = [sum(len(b) for b in blocks[i:i + UNIT]) for i in range(0, len(blocks), UNIT)]
    return out
