"""No kernel writes outside the memory a call hands it (include/mi355lz4.h, "What a call may write").

Every case does three things: it compares results and bytes with the oracle, it runs the guard checker of tests/guarded.py over
every output array of the call -- every block, whatever its result -- and it checks that every input tensor is bit-identical
after the call.  Outputs lie in guarded layouts: every block's output (every slot) starts at its own alignment mod 16 with at
least a wave-wide store of position-dependent pattern between it and its neighbours and a workgroup segment of it at both ends
of the allocation.  Inputs lie in such layouts too, and calls are repeated with different bytes in every gap: a result that
changes was read from outside the call's blocks.  tests/test_guarded.py pins the helper and the input sets without a GPU."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import confinement_cases as CC
import guarded as G
from conftest import DECODERS
from test_parity_gpu import LINKED_VARIANTS, split_blocks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
E_UNCOMPLEN = -0x7F000003


def _t(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


class _Inputs:
    """the input tensors of a call, with copies: same() asserts that the call left every one of them as it was"""

    def __init__(self, **tensors):
        self.t = {k: v for k, v in tensors.items() if v is not None}
        self.copy = {k: v.clone() for k, v in self.t.items()}

    def same(self, what=""):
        import torch
        for k, v in self.t.items():
            assert torch.equal(v, self.copy[k]), (what, "input written", k)


@pytest.fixture(scope="module")
def dcases(oracle, golden):
    return CC.capacity_classes(CC.decode_cases(oracle, golden))


_expect_cache = {}


def _expect(oracle, c, cap):
    k = (c.payload, cap)                 # by content: an id() is handed out again once its case has been collected
    if k not in _expect_cache:
        _expect_cache[k] = oracle.decompress_block(c.payload, cap)
    return _expect_cache[k]


def _plan(oracle, cases, kind, capmode):
    """per block: (outCap or None, allowed bytes, expected code, expected bytes); the call's fixedUncomp"""
    fixed, sizes = CC.region_sizes(cases, kind, capmode)
    plan = []
    for c, (ocap, allowed) in zip(cases, sizes):
        if kind == 8 and ocap is not None and c.cap > ocap:
            plan.append((ocap, 0, E_UNCOMPLEN, b""))                   # rejected for its uncompLen: the block may write nothing
            continue
        cap = (c.cap if kind == 8 else fixed) if (kind == 8 or ocap is None) else ocap
        code, dec = _expect(oracle, c, cap)
        plan.append((ocap, allowed, code, dec))
    return fixed, plan


def _framed_layout(cases, kind):
    """the framed blocks, each a region of a guarded input layout: (layout, [header + payload])"""
    blocks = [len(c.payload).to_bytes(4, "little") + (c.cap.to_bytes(4, "little") if kind == 8 else b"") + c.payload for c in cases]
    return G.layout([len(b) for b in blocks]), blocks


def _decode_guarded(engine, oracle, cases, kind, capmode, what, dbg=None, both_fillings=False):
    """one decompress_batch_device call over `cases` in guarded input and output layouts; every check of this file"""
    import torch
    import streamly_lz4_amd as S_
    n = len(cases)
    fixed, plan = _plan(oracle, cases, kind, capmode)
    lay_in, blocks = _framed_layout(cases, kind)
    lay = G.layout([p[1] for p in plan])
    outs = []
    for filling, host in enumerate(G.pair(lay_in, blocks)[: 2 if both_fillings else 1]):
        seed = 11 + filling
        out = G.new_torch(lay.total, seed, DEV)
        res = G.GuardedArray(n, torch.int32, seed + 50, DEV)
        ocap = _t(np.array([p[0] for p in plan], dtype=np.int32)) if capmode != "absent" else None
        inp = _Inputs(framed=_t(host), boff=_t(np.array(lay_in.starts, dtype=np.int64)),
                      ooff=_t(np.array(lay.starts, dtype=np.int64)), ocap=ocap)
        if dbg is not None:
            S_.lib.mi355lz4_debug_cu(engine.ctx, C.c_void_p(dbg.data_ptr()))
        try:
            engine.decompress_batch_device(inp.t["framed"], lay_in.total, inp.t["boff"], n, out, inp.t["ooff"], res.view,
                                           header_kind=kind, fixed_uncomp=fixed, out_cap=ocap)
            engine.synchronize()
        finally:
            if dbg is not None:
                S_.lib.mi355lz4_debug_cu(engine.ctx, None)
        got = res.view.cpu().tolist()
        host_out = out.cpu().numpy()
        for i, (c, p) in enumerate(zip(cases, plan)):
            assert got[i] == p[2], (what, i, c, p[0], got[i], p[2])
            if p[2] >= 0:
                s = lay.starts[i]
                assert host_out[s:s + p[2]].tobytes() == p[3], (what, i, c, "bytes differ")
        G.assert_confined(out, lay.ranges(), seed, "%s: out" % (what,))
        res.check(what="%s: result[]" % (what,))
        inp.same(what)
        outs.append((got, host_out))
    if both_fillings:                                                   # what lies between the framed blocks is never read
        assert outs[0][0] == outs[1][0], (what, "results depend on the bytes between the blocks")
        for i, p in enumerate(plan):
            if p[2] >= 0:
                s = lay.starts[i]
                assert np.array_equal(outs[0][1][s:s + p[2]], outs[1][1][s:s + p[2]]), (what, i)
    return lay, plan


# ---- decoders ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("capmode", ["absent", "larger", "smaller"])
@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("decoder", DECODERS)
def test_decode_confined(engine, oracle, dcases, decoder, kind, capmode):
    """Every decoder kernel over oracle-written blocks, every lz4_synth family, the fuzz corruptions (1 MiB and 4 MiB blocks among
    them), the huge length fields and golden.json's malformed blocks: codes and bytes are the oracle's and nothing outside
    [outOff[i], outOff[i] + cap_i) is written, whatever the block's result.  The workgroup decoder's diagnostics say that both
    its parallel parse and its fallbacks ran."""
    import torch
    engine.set_decoder(decoder)
    try:
        for cls, cases in dcases.items():
            dbg = torch.zeros(len(cases) * 16, dtype=torch.int32, device=DEV) if decoder == 4 else None
            _, plan = _decode_guarded(engine, oracle, cases, kind, capmode, (decoder, kind, capmode, cls), dbg,
                                      both_fillings=(capmode == "absent" and kind == 8))
            if capmode == "smaller" and kind == 8:
                assert sum(1 for p in plan if p[2] == E_UNCOMPLEN) > len(cases) // 2
            if dbg is not None and cls == "small" and not (capmode == "smaller" and kind == 8):
                d = dbg.view(len(cases), 16).cpu().numpy().astype(np.uint32)
                whys = {int(r[0]) for r in d if r[15] != 0}
                assert any(r[15] != 0 and r[0] == 0 and (r[1] & 0xFFFF) > 0 for r in d), "the parallel parse never ran"
                assert {2, 5} <= whys, ("a fallback of the parallel parse (why 2, why 5) was not reached", sorted(whys))
    finally:
        engine.set_decoder(0)


@pytest.mark.parametrize("nblk", [256, 257])
def test_decode_confined_both_sides_of_variant_0(engine, oracle, nblk):
    """Variant 0 takes the workgroup decoder for calls of up to 256 blocks and the lane-parallel one beyond (the diagnostics say
    which ran); clean and corrupted 16 KiB blocks, guarded."""
    import torch
    rng = random.Random(nblk)
    cases = []
    for i in range(nblk):
        d = oracle.gen("text", 1, 16384, first_block=i).tobytes()
        p = bytearray(oracle.compress_block(d, 1))
        if i % 5 == 3:
            p[rng.randrange(len(p))] ^= 1 << rng.randrange(8)
        if i % 11 == 7:
            p = p[: rng.randrange(1, len(p))]
        cases.append(CC.DCase("v0", str(i), bytes(p), 16384, 16384, True))
    engine.set_decoder(0)
    dbg = torch.zeros(nblk * 16, dtype=torch.int32, device=DEV)
    _, plan = _decode_guarded(engine, oracle, cases, 8, "absent", ("variant 0", nblk), dbg)
    assert any(p[2] < 0 for p in plan) and any(p[2] == 16384 for p in plan)
    ran = bool((dbg.view(nblk, 16)[:, 15] != 0).any().item())
    assert ran == (nblk <= 256), (nblk, ran)


def test_decode_huge_length_fields_confined_with_neighbours(engine, oracle):
    """The huge-length blocks between valid neighbours, decoder chosen by the library: the neighbours' bytes stand."""
    good = CC.oracle_written(oracle)[:6]
    cases = []
    for h in CC.huge():
        cases += [good[len(cases) % 6], h]
    _decode_guarded(engine, oracle, cases, 8, "absent", "huge between neighbours")


# ---- linked decodes ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(params=list(LINKED_VARIANTS) + ["big_blocks"])
def linked_variant(request, monkeypatch):
    for k, v in LINKED_VARIANTS.get(request.param, {}).items():
        monkeypatch.setenv(k, v)
    if request.param == "big_blocks":
        monkeypatch.delenv("MI355LZ4_LINKED_BIG", raising=False)
    return request.param


_streams_cache = {}


def _linked_streams(oracle):
    """[(name, framed stream, block length)]: reference-written and engine-written linked streams of 64 KiB, 256 KiB and 1 MiB
    blocks, clean and with one corrupted block in the middle"""
    if "s" in _streams_cache:
        return _streams_cache["s"]
    import streamly_lz4_amd as S_
    rng = random.Random(3)
    eng = S_.Engine(0)
    out = []
    try:
        eng.set_linked_compress(True)
        for bl, nblk in ((65536, 10), (262144, 5), (1 << 20, 4)):
            raw = oracle.gen("text", nblk * bl // 65536, 65536, first_block=bl >> 12).tobytes()[: nblk * bl - 333]   # a ragged last block
            ref = oracle.frame_compress(raw, bl, 1, 8, True)
            own = eng.compress_batch([raw[i:i + bl] for i in range(0, len(raw), bl)])[0]
            for writer, fr in (("reference", ref), ("engine", own)):
                out.append(("%s %d clean" % (writer, bl), fr, bl))
                blocks = split_blocks(fr)
                bi = nblk // 2
                start = sum(len(b) for b in blocks[:bi]) + 8
                bad = bytearray(fr)
                bad[start + rng.randrange(len(blocks[bi]) - 8)] ^= 1 << rng.randrange(8)
                out.append(("%s %d corrupted" % (writer, bl), bytes(bad), bl))
    finally:
        eng.close()
    _streams_cache["s"] = out
    return out


def _linked_expect(oracle, fr):
    """the oracle's linked decode, block by block: [(uncompLen, code, bytes or None, code when decoded on its own)]"""
    d, res = None, []
    for b in split_blocks(fr):
        u = int.from_bytes(b[4:8], "little")
        code, dec = oracle.decompress_block(b[8:], u, d)
        res.append((u, code, dec if code >= 0 else None, oracle.decompress_block(b[8:], u)[0]))
        if code > 0:
            d = dec
    return res


def _linked_call(engine, oracle, frs, mode, what, look_back=False):
    """the streams `frs` through one guarded call: mode "one" (linked = 1; one stream), "streams", or "begin_end" (one stream;
    with look_back the stream's first block is the seam: decoded beforehand, placed between _begin and _end)"""
    import torch
    exp = [_linked_expect(oracle, fr) for fr in frs]
    assert all(any(e[3] < 0 <= e[1] for e in ex) for ex in exp), (what, "no dependent block: the second pass would not run")
    blocks = [b for fr in frs for b in split_blocks(fr)]
    flat = [e for ex in exp for e in ex]
    lb = 1 if look_back else 0
    lay_in = G.layout([len(b) for b in blocks[lb:]])
    lay = G.layout([e[0] for e in flat])                               # (with look_back region 0 is the seam's slot)
    n = len(blocks) - lb
    host = G.pair(lay_in, blocks[lb:])[0]
    out = G.new_torch(lay.total, 21, DEV)
    res = G.GuardedArray(n, torch.int32, 22, DEV, lead=1)              # one item in front: result[-1]
    ooff = _t(np.array(lay.starts, dtype=np.int64))
    inp = _Inputs(framed=_t(host), boff=_t(np.array(lay_in.starts, dtype=np.int64)), ooff=ooff)
    if mode == "one":
        engine.decompress_batch_device(inp.t["framed"], lay_in.total, inp.t["boff"], n, out, ooff, res.view, linked=True)
    elif mode == "streams":
        first = np.cumsum([0] + [len(ex) for ex in exp]).astype(np.int32)
        inp.t["sf"] = _t(first)
        inp.copy["sf"] = inp.t["sf"].clone()
        engine.decompress_streams_device(inp.t["framed"], lay_in.total, inp.t["boff"], n, inp.t["sf"], len(frs), out, ooff, res.view)
    else:
        seam = flat[0][2] if lb else None
        if lb:
            res.all[0] = len(seam)                                      # result[-1]: the seam's size, the caller's
        engine.decompress_linked_begin(inp.t["framed"], lay_in.total, inp.t["boff"], n, out, ooff, res.all if lb else res.view, lb)
        engine.synchronize()
        if lb:                                                          # _begin reads and writes nothing of the seam's slot
            G.assert_confined(out, lay.ranges()[1:], 21, "%s: out after _begin" % (what,))
            s = lay.starts[0]
            out[s:s + len(seam)] = _t(np.frombuffer(seam, dtype=np.uint8))
        engine.decompress_linked_end_last()
        engine.decompress_linked_end()
    engine.synchronize()
    got = res.view.cpu().tolist()
    host_out = out.cpu().numpy()
    for i, e in enumerate(flat):
        s = lay.starts[i]
        if i < lb:
            assert host_out[s:s + e[0]].tobytes() == e[2], (what, "the seam's slot was written")
            continue
        assert got[i - lb] == e[1], (what, i, got[i - lb], e[1])
        if e[2] is not None:
            assert host_out[s:s + e[1]].tobytes() == e[2], (what, i, "bytes differ")
    G.assert_confined(out, lay.ranges(), 21, "%s: out" % (what,))
    res.check(lo=-lb, what="%s: result[]" % (what,))                  # (without look_back result[-1] is guard)
    if lb:
        assert int(res.all[0].item()) == len(flat[0][2]), (what, "result[-1] was written")
    inp.same(what)


def test_linked_decode_confined(engine, oracle, linked_variant):
    """Every second pass (LINKED_VARIANTS, and the big-block path for the 1 MiB streams) over reference- and engine-written
    linked streams, clean and corrupted: the oracle's codes and bytes, nothing outside the blocks' outputs, result[] only in
    [0, nBlocks)."""
    for name, fr, bl in _linked_streams(oracle):
        if linked_variant == "big_blocks" and bl < (1 << 20):
            continue
        if linked_variant not in ("default", "big_blocks", "pointer_pass_forced", "replay_only", "runin", "async") and \
                (bl > 65536 and "engine" in name):
            continue                                    # (the products trimmed for wall time: every path still sees every block size)
        _linked_call(engine, oracle, [fr], "one", (linked_variant, name))


def test_linked_big_block_path_ran(engine, oracle, monkeypatch):
    """The clean 1 MiB streams really go through the big-block path (path 6) by default."""
    import streamly_lz4_amd as S_
    monkeypatch.delenv("MI355LZ4_LINKED_BIG", raising=False)
    for name, fr, bl in _linked_streams(oracle):
        if bl == (1 << 20) and "reference" in name and "clean" in name:
            _linked_call(engine, oracle, [fr], "one", ("path", name))
            st = (C.c_int * 5)()
            S_.lib.mi355lz4_debug_runin_state(engine.ctx, st, None)
            assert st[4] == 6, st[4]


@pytest.mark.parametrize("variant", ["default", "pointer_pass_forced", "replay_only", "serial_only"])
def test_linked_streams_call_confined(engine, oracle, monkeypatch, variant):
    for k, v in LINKED_VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    frs = [fr for _, fr, _ in _linked_streams(oracle)]
    _linked_call(engine, oracle, frs, "streams", ("streams", variant))


@pytest.mark.parametrize("look_back", [0, 1])
@pytest.mark.parametrize("variant", ["default", "pointer_pass_forced", "pointer_segments_of_2"])
def test_linked_begin_end_confined(engine, oracle, monkeypatch, variant, look_back):
    """_begin / _end_last / _end: with lookBack = 1 the seam block's slot and result[-1] are the caller's, never written."""
    for k, v in LINKED_VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    for name, fr, bl in _linked_streams(oracle):
        if "reference" in name or bl == 65536:
            _linked_call(engine, oracle, [fr], "begin_end", ("begin_end", variant, look_back, name), look_back=bool(look_back))


# ---- encoders ------------------------------------------------------------------------------------------------------------------------

ENCODERS = {
    "level0_auto": dict(segments=-1), "level0_noseg": dict(segments=0), "level0_seg2": dict(segments=2),
    "level0_seg64": dict(segments=64), "level0_linked": dict(linked=True), "level1": dict(level=1), "level9": dict(level=9),
    "exact": dict(exact=True),
}


def _slot_check(oracle, S_, slot, flen, block, kind, checksum, dict_bytes, what):
    fr = slot[:flen].tobytes()
    comp_len = int.from_bytes(fr[:4], "little")
    assert flen == kind + comp_len + (4 if checksum else 0), (what, flen, comp_len)
    if kind == 8:
        assert int.from_bytes(fr[4:8], "little") == len(block), what
    comp = fr[kind:kind + comp_len]
    assert 0 < comp_len <= oracle.compress_bound(len(block)), (what, comp_len)
    assert oracle.decompress_block(comp, len(block), dict_bytes) == (len(block), block), (what, "the oracle does not decode the slot")
    if checksum:
        assert int.from_bytes(fr[kind + comp_len:], "little") == S_.xxh32(comp), (what, "trailer")
    return comp


def _encode_guarded(eng, oracle, blocks, kind, checksum, extra, mode, what, stream=None):
    """one compress_batch_device call: src in a guarded layout (back to back when the call links its blocks), slots at
    slot_stride_ex + extra, framedLen guarded; returns the slots' framed bytes"""
    import torch
    import streamly_lz4_amd as S_
    n = len(blocks)
    mx = max(len(b) for b in blocks)
    need = S_.slot_stride_ex(mx, kind, checksum)
    stride = need + extra
    linked = bool(mode.get("linked"))
    if linked:                                                          # block i - 1 directly in front of block i
        lay_src = G.layout([sum(len(b) for b in blocks)])
        starts = (lay_src.starts[0] + np.cumsum([0] + [len(b) for b in blocks[:-1]])).tolist()
        hosts = G.pair(lay_src, [b"".join(blocks)])
    else:
        lay_src = G.layout([len(b) for b in blocks])
        starts = lay_src.starts
        hosts = G.pair(lay_src, blocks)
    lay = G.layout([need] * n, stride=stride, first_residue=extra)
    results = []
    for filling, host in enumerate(hosts if not (linked or mode.get("exact")) else hosts[:1]):
        seed = 31 + filling
        buf = G.new_torch(lay.total, seed, DEV)
        flen = G.GuardedArray(n, torch.int32, seed + 50, DEV)
        inp = _Inputs(src=_t(host), off=_t(np.array(starts, dtype=np.int64)), ln=_t(np.array([len(b) for b in blocks], dtype=np.int32)))
        slots = buf[lay.starts[0]:]
        eng.compress_batch_device(inp.t["src"], n, mx, slots, stride, flen.view, accel=1, header_kind=kind,
                                  src_off=inp.t["off"], src_len=inp.t["ln"], block_stride=0)
        eng.synchronize()
        fl = flen.view.cpu().tolist()
        G.assert_confined(buf, lay.ranges(), seed, "%s: slots" % (what,))
        flen.check(what="%s: framedLen[]" % (what,))
        inp.same(what)
        hb = buf.cpu().numpy()
        results.append((fl, [hb[s:s + f].copy() for s, f in zip(lay.starts, fl)]))
    fl, slots_h = results[0]
    d = getattr(stream, "last", None)                                   # (an exact stream carries its dictionary from call to call)
    comps = []
    for i, b in enumerate(blocks):
        dict_bytes = d if (linked or mode.get("exact")) else None
        comps.append(_slot_check(oracle, S_, slots_h[i], fl[i], b, kind, checksum, dict_bytes, (what, i, len(b))))
        if len(b) > 0:
            d = b
    if stream is not None:                                              # exact mode: the reference's bytes, across calls
        stream.last = d
        assert comps == stream.compress(blocks, 1), (what, "not the reference's bytes")
    if len(results) == 2:                                               # what lies between the blocks of src is never read
        assert results[0][0] == results[1][0], (what, "framedLen depends on the bytes between the blocks")
        assert all(np.array_equal(a, b) for a, b in zip(results[0][1], results[1][1])), (what, "slots depend on the bytes between the blocks")
    return slots_h


@pytest.mark.parametrize("checksum", [False, True])
@pytest.mark.parametrize("kind", [8, 4])
@pytest.mark.parametrize("encoder", list(ENCODERS))
def test_encode_confined(oracle, encoder, kind, checksum):
    """Every encoder over ragged blocks (0, 1, 12, 13, 64 Ki +- 1 bytes, incompressible ones that fill their slot to the worst
    case, test_fuzz_encode_gpu._make's inputs) with slotStride = slot_stride_ex and larger by an odd amount: nothing outside
    [slot, slot + slot_stride_ex) and framedLen[0, nBlocks) is written, the inputs stand, and the same call over src with
    other bytes between the blocks gives the same slots."""
    import streamly_lz4_amd as S_
    mode = ENCODERS[encoder]
    blocks = CC.encode_blocks(oracle)
    if mode.get("segments", 0) == 64:
        blocks = blocks[:20] + [oracle.gen("text", 1, 300000, first_block=3).tobytes()]   # (64 segments need 256 KiB and more)
    eng = S_.Engine(0)
    try:
        eng.set_block_checksum(checksum)
        if "segments" in mode:
            eng.set_segments(mode["segments"])
        if mode.get("linked"):
            eng.set_linked_compress(True)
        if "level" in mode:
            eng.set_compression_level(mode["level"])
        stream = None
        if mode.get("exact"):
            from test_exact_compress_gpu import OracleStream
            eng.set_compress_exact(True)
            stream = OracleStream()
        for extra in (0, 37):
            if stream is not None:
                eng.reset_compress_stream()
                stream.reset()
                stream.last = None
            _encode_guarded(eng, oracle, blocks, kind, checksum, extra, mode, (encoder, kind, checksum, extra), stream)
            if stream is not None:                                      # a second call continues the stream
                _encode_guarded(eng, oracle, blocks[::-1][:30], kind, checksum, extra, mode, (encoder, kind, checksum, extra, "2nd"), stream)
    finally:
        eng.close()


@pytest.mark.parametrize("encoder", ["level0_auto", "level1", "level9"])
def test_encode_confined_fixed_stride(oracle, encoder):
    """The other way to address src: block i at src + i * blockStride with blockStride > srcLen[i] (no srcOff).  The bytes
    between a block's end and the next stride are never read -- the same call with other bytes there gives the same slots --
    and the slots and framedLen[] are confined as above."""
    import torch
    import streamly_lz4_amd as S_
    rng = random.Random(12)
    mx, stride = 4096, 4096 + G.GAP
    lens = [0, 1, 12, 13, 4095, 4096] + [rng.randrange(mx + 1) for _ in range(20)] + [4096]
    blocks = [oracle.gen(("text", "lzsynth", "random")[i % 3], 1, mx, first_block=200 + i)[:n].tobytes() for i, n in enumerate(lens)]
    n = len(blocks)
    lay_src = G.layout(lens, stride=stride, first_residue=3)
    need = S_.slot_stride_ex(mx, 8, False)
    lay = G.layout([need] * n, stride=need + 37, first_residue=37)
    eng = S_.Engine(0)
    try:
        if "level" in ENCODERS[encoder]:
            eng.set_compression_level(ENCODERS[encoder]["level"])
        results = []
        for filling, host in enumerate(G.pair(lay_src, blocks)):
            seed = 61 + filling
            buf = G.new_torch(lay.total, seed, DEV)
            flen = G.GuardedArray(n, torch.int32, seed + 50, DEV)
            inp = _Inputs(src=_t(host), ln=_t(np.array(lens, dtype=np.int32)))
            eng.compress_batch_device(inp.t["src"][lay_src.starts[0]:], n, mx, buf[lay.starts[0]:], need + 37, flen.view, accel=1,
                                      header_kind=8, src_len=inp.t["ln"], block_stride=stride)
            eng.synchronize()
            fl = flen.view.cpu().tolist()
            G.assert_confined(buf, lay.ranges(), seed, (encoder, "fixed stride: slots"))
            flen.check(what=(encoder, "fixed stride: framedLen[]"))
            inp.same((encoder, "fixed stride"))
            hb = buf.cpu().numpy()
            results.append((fl, [hb[s:s + f].copy() for s, f in zip(lay.starts, fl)]))
        for i, b in enumerate(blocks):
            _slot_check(oracle, S_, results[0][1][i], results[0][0][i], b, 8, False, None, (encoder, "fixed stride", i, len(b)))
        assert results[0][0] == results[1][0], (encoder, "framedLen depends on the bytes between the blocks")
        assert all(np.array_equal(a, b) for a, b in zip(results[0][1], results[1][1])), (encoder, "slots depend on the bytes between the blocks")
    finally:
        eng.close()


# ---- small kernels --------------------------------------------------------------------------------------------------------------------

def _compressed_slots(engine, slz4, oracle, n=16, bl=4096):
    import torch
    raw = oracle.gen("lzsynth", n, bl, first_block=3).tobytes()
    stride = slz4.slot_stride(bl, 8)
    slots = torch.empty(n * stride, dtype=torch.uint8, device=DEV)
    flen = torch.empty(n, dtype=torch.int32, device=DEV)
    engine.compress_batch_device(_t(np.frombuffer(raw, dtype=np.uint8).copy()), n, bl, slots, stride, flen)
    engine.synchronize()
    return raw, slots, stride, flen


@pytest.mark.parametrize("cap_kind", ["mid_block", "exact", "zero", "block_edge"])
def test_compact_confined(engine, slz4, oracle, cap_kind):
    """compact_device with denseCap inside a block, exactly the stream's size, at a block's edge and zero: guards on both sides
    of dense and of denseOff; blocks that fit are the slots' bytes."""
    import torch
    n = 16
    raw, slots, stride, flen = _compressed_slots(engine, slz4, oracle, n)
    fl = flen.cpu().tolist()
    offs = np.concatenate([[0], np.cumsum(fl)]).astype(np.int64)
    need = int(offs[-1])
    cap = {"mid_block": int(offs[7]) + fl[7] // 2 + 1, "exact": need, "zero": 0, "block_edge": int(offs[9])}[cap_kind]
    for residue in (0, 5):
        lay = G.layout([cap], first_residue=residue)
        dense = G.new_torch(lay.total, 41, DEV)
        doff = G.GuardedArray(n + 1, torch.int64, 42, DEV)
        inp = _Inputs(slots=slots, flen=flen)
        engine.compact_device(slots, stride, flen, n, dense[lay.starts[0]:], cap, doff.view)
        engine.synchronize()
        assert doff.view.cpu().tolist() == offs.tolist()
        G.assert_confined(dense, lay.ranges(), 41, ("compact", cap_kind, residue))
        doff.check(what="denseOff[]")
        inp.same("compact")
        s = lay.starts[0]
        fitted = [i for i in range(n) if offs[i + 1] <= cap]
        assert len(fitted) == {"mid_block": 7, "exact": n, "zero": 0, "block_edge": 9}[cap_kind]
        for i in fitted:
            assert torch.equal(dense[s + int(offs[i]):s + int(offs[i + 1])], slots[i * stride:i * stride + fl[i]])
        if fitted:                                                      # the bytes of blocks that did not fit are not written either
            G.assert_confined(dense, [(s, s + int(offs[fitted[-1] + 1]))], 41, ("compact, skipped blocks", cap_kind))


def test_index_confined(engine, oracle):
    import torch
    cases = CC.oracle_written(oracle)[:40]
    lay_in, blocks = _framed_layout(cases, 8)
    n = len(cases)
    ooff = G.GuardedArray(n + 1, torch.int64, 43, DEV)
    inp = _Inputs(framed=_t(G.pair(lay_in, blocks)[0]), boff=_t(np.array(lay_in.starts, dtype=np.int64)))
    engine.index_device(inp.t["framed"], lay_in.total, inp.t["boff"], n, ooff.view)
    engine.synchronize()
    assert ooff.view.cpu().tolist() == np.concatenate([[0], np.cumsum([c.cap for c in cases])]).tolist()
    ooff.check(what="index outOff[]")
    inp.same("index")


def test_interleave_confined(engine):
    """rank g's local blocks go to global blocks j * nRanks + g and nowhere else: the other ranks' places stay pattern."""
    import torch
    rng = random.Random(4)
    n_ranks, n_local = 3, 7
    sizes = [rng.choice([0, 1, 15, 16, 17, 1000, 4097]) for _ in range(n_ranks * n_local)]
    lay = G.layout(sizes)
    for rank in range(n_ranks):
        mine = [j * n_ranks + rank for j in range(n_local)]
        datas = [rng.randbytes(sizes[g]) for g in mine]
        loff = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.int64)
        glob = G.new_torch(lay.total, 44, DEV)
        inp = _Inputs(local=_t(np.frombuffer(b"".join(datas) + b"\0", dtype=np.uint8).copy()), loff=_t(loff),
                      goff=_t(np.array(lay.starts, dtype=np.int64)))
        engine.interleave_device(inp.t["local"], inp.t["loff"], n_local, rank, n_ranks, glob, inp.t["goff"])
        engine.synchronize()
        G.assert_confined(glob, [lay.ranges()[g] for g in mine], 44, ("interleave", rank))
        h = glob.cpu().numpy()
        for g, d in zip(mine, datas):
            assert h[lay.starts[g]:lay.starts[g] + len(d)].tobytes() == d
        inp.same("interleave")


@pytest.mark.parametrize("kind", ["random", "lzsynth", "text"])
def test_generate_confined(engine, oracle, kind):
    for bl, n in ((1, 5), (13, 7), (4097, 3), (65536, 2)):
        lay = G.layout([bl * n], first_residue=bl)
        buf = G.new_torch(lay.total, 45, DEV)
        engine.generate(kind, buf[lay.starts[0]:], bl, n, first_block=9)
        engine.synchronize()
        G.assert_confined(buf, lay.ranges(), 45, ("generate", kind, bl))
        s = lay.starts[0]
        assert buf[s:s + bl * n].cpu().numpy().tobytes() == oracle.gen(kind, n, bl, first_block=9).tobytes()


def test_xxh32_confined(engine, slz4):
    """out[i] is written for len[i] >= 0 (zero included) and left alone for len[i] < 0; nothing else is."""
    import torch
    rng = random.Random(6)
    lens = [0, -1, 1, 15, -5, 16, 17, 0, 4096, -(1 << 31), 70001, 3, -2]
    datas = [rng.randbytes(max(0, x)) for x in lens]
    lay = G.layout([len(d) for d in datas])
    out = G.GuardedArray(len(lens), torch.int32, 46, DEV)
    before = out.view.clone()
    inp = _Inputs(base=_t(G.pair(lay, datas)[0]), off=_t(np.array(lay.starts, dtype=np.int64)), ln=_t(np.array(lens, dtype=np.int32)))
    engine.xxh32_device(inp.t["base"], inp.t["off"], inp.t["ln"], len(lens), 7, out.view)
    engine.synchronize()
    got = out.view.cpu().numpy().astype(np.uint32).tolist()
    for i, (x, d) in enumerate(zip(lens, datas)):
        if x >= 0:
            assert got[i] == slz4.xxh32(d, 7), (i, x)
        else:
            assert out.view[i] == before[i], ("out[%d] written for a negative length" % i, x)
    out.check(what="xxh32 out[]")
    inp.same("xxh32")


# ---- host-buffer calls ----------------------------------------------------------------------------------------------------------------

HOST_CHILD = r'''
import os, sys
ROOT = %r
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "streamly-lz4_amd"))
import test_write_confinement_gpu as T
from oracle.oracle import Oracle
T.host_calls(Oracle())
print("host calls ok")
'''


def host_calls(oracle):
    """_compress_batch / _decompress_batch / _decompress_streams and the _multi_ calls on numpy buffers inside guarded arrays, cap
    exactly what is needed, the per-block arrays guarded behind nBlocks"""
    import streamly_lz4_amd as S_
    L = S_.lib
    u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    blocks = [b for b in CC.encode_blocks(oracle, n_fuzz=30)] + [oracle.gen("text", 1, 65536, first_block=i).tobytes() for i in range(40)]
    n = len(blocks)
    raw = b"".join(blocks)
    lay_src = G.layout([len(b) for b in blocks])
    src = G.pair(lay_src, blocks)[0]
    src_copy = src.copy()
    ptrs = (u8p * n)(*[C.cast(src.ctypes.data + s, u8p) for s in lay_src.starts])
    lens = np.array([len(b) for b in blocks], dtype=np.int32)
    eng, multi = S_.Engine(0), S_.MultiEngine([0, 0])
    try:
        streams = {}
        for who in ("engine", "multi", "engine_linked"):
            if who == "engine_linked":
                eng.set_linked_compress(True)
            # first call: learn the size; second: cap exactly that
            fr, _ = (eng if who != "multi" else multi).compress_batch(blocks)
            cap = len(fr)
            lay = G.layout([cap], first_residue=3)
            buf = G.new_numpy(lay.total, 51)
            fl, st = G.GuardedArray(n, np.int32, 52), G.GuardedArray(n, np.int32, 53)
            olen = C.c_size_t()
            dst = C.cast(buf.ctypes.data + lay.starts[0], u8p)
            if who == "multi":
                rc = L.mi355lz4_multi_compress_batch(multi._h, ptrs, lens.ctypes.data_as(i32p), n, 1, 8, dst, C.c_size_t(cap), C.byref(olen),
                                                     fl.view.ctypes.data_as(i32p), st.view.ctypes.data_as(i32p))
            else:
                rc = L.mi355lz4_compress_batch(eng.ctx, ptrs, lens.ctypes.data_as(i32p), n, 1, 8, dst, cap, C.byref(olen),
                                               fl.view.ctypes.data_as(i32p), st.view.ctypes.data_as(i32p))
            assert rc == 0 and olen.value == cap, (who, rc, olen.value, cap)
            G.assert_confined(buf, lay.ranges(), 51, (who, "framedOut"))
            fl.check(what=(who, "blockFramedLen"))
            st.check(what=(who, "status"))
            assert np.array_equal(src, src_copy), (who, "src written")
            got = buf[lay.starts[0]:lay.starts[0] + cap].tobytes()
            assert got == fr and sum(fl.view.tolist()) == cap
            assert oracle.frame_decompress(got, len(raw), 8, 0, True) == raw, who
            streams[who] = got
            eng.set_linked_compress(False)
        streams["reference_linked"] = oracle.frame_compress(b"".join(blocks[-40:]), 65536, 1, 8, True)
        # one block of the engine's stream overwritten until the oracle says it fails (and the others stand)
        parts = split_blocks(streams["engine"])
        k = n - 20
        rng = random.Random(8)
        while True:
            p = bytearray(parts[k])
            at = 8 + rng.randrange(len(p) - 16)
            p[at:at + 8] = b"\xff" * 8
            if oracle.decompress_block(bytes(p[8:]), len(blocks[k]))[0] < 0:
                break
        streams["corrupted"] = b"".join(parts[:k]) + bytes(p) + b"".join(parts[k + 1:])
        codes = {who: [oracle.decompress_block(b[8:], int.from_bytes(b[4:8], "little"))[0] for b in split_blocks(fr)]
                 for who, fr in streams.items() if who in ("engine", "multi", "corrupted")}
        for who, fr in streams.items():
            want = raw if who != "reference_linked" else b"".join(blocks[-40:])
            nb = len(split_blocks(fr))
            linked = who in ("engine_linked", "reference_linked")
            lay_in = G.layout([len(fr)], first_residue=5)
            fin = G.pair(lay_in, [fr])[0]
            fin_copy = fin.copy()
            cap = len(want)
            lay = G.layout([cap], first_residue=7)
            for call in (("batch", "streams", "multi") if not linked else ("batch", "streams")):
                buf = G.new_numpy(lay.total, 54)
                bl = G.GuardedArray(nb, np.int32, 55)
                olen, got_n = C.c_size_t(), C.c_int()
                a_in = C.cast(fin.ctypes.data + lay_in.starts[0], u8p)
                a_out = C.cast(buf.ctypes.data + lay.starts[0], u8p)
                if call == "batch":
                    rc = L.mi355lz4_decompress_batch(eng.ctx, a_in, len(fr), 8, 0, int(linked), None, 0, a_out, cap, C.byref(olen),
                                                     bl.view.ctypes.data_as(i32p), nb, C.byref(got_n))
                elif call == "streams":
                    sf = np.array([0, nb] if linked else [0, 0], dtype=np.int32)
                    sf_copy = sf.copy()
                    rc = L.mi355lz4_decompress_streams(eng.ctx, a_in, len(fr), 8, 0, sf.ctypes.data_as(i32p), 1, a_out, cap,
                                                       C.byref(olen), bl.view.ctypes.data_as(i32p), nb, C.byref(got_n))
                    assert np.array_equal(sf, sf_copy)
                else:
                    rc = L.mi355lz4_multi_decompress_batch(multi._h, a_in, C.c_size_t(len(fr)), 8, 0, a_out, C.c_size_t(cap), C.byref(olen),
                                                           bl.view.ctypes.data_as(i32p), nb, C.byref(got_n))
                assert rc == (0 if who != "corrupted" else -5) and got_n.value == nb, (who, call, rc, got_n.value)
                G.assert_confined(buf, lay.ranges(), 54, (who, call, "out"))
                bl.check(what=(who, call, "blockLen"))
                assert np.array_equal(fin, fin_copy), (who, call, "framedIn written")
                if who != "corrupted":
                    assert olen.value == cap and buf[lay.starts[0]:lay.starts[0] + cap].tobytes() == want, (who, call)
                    assert bl.view.tolist() == [len(b) for b in (blocks if who != "reference_linked" else blocks[-40:])]
                else:
                    assert bl.view.tolist() == codes[who] and sum(1 for x in codes[who] if x < 0) == 1, (who, call)
    finally:
        eng.close()
        multi.close()


def test_host_calls_confined(oracle):
    host_calls(oracle)


def test_host_calls_confined_many_groups():
    """once more with groups of 1 MiB (read once per process: a child), the way tests/test_host_pipeline_gpu.py starts one"""
    env = dict(os.environ, MI355LZ4_GROUP_MB="1")
    r = subprocess.run([sys.executable, "-c", HOST_CHILD % ROOT], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "host calls ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
