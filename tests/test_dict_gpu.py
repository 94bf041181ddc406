"""Shared-dictionary batches on the GPU: mi355lz4_cstreams_load_dict (LZ4_loadDict on a slot), mi355lz4_compress_dict_device (a batch,
every block from a copy of the loaded slot) and mi355lz4_decompress_dict_device (LZ4_decompress_safe_usingDict's external-dictionary
path).  Bytes and codes are those of tests/dict_model.py -- which tests/test_dict_host.py holds to the reference's golden,
tests/golden/dict_vectors.json -- and of the golden itself, over the grid of tests/dict_cases.py."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dict_cases as DC  # noqa: E402
import dict_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG = -3
BLK_E_CHECKSUM = -0x7F000004
BLK_E_COMPLEN = -0x7F000001
MAXLEN = max(DC.BLOCK_LENS)
APART = 7                     # sources and outputs lie 7 bytes apart: every alignment occurs
FILL = 0xA5
_u8p = C.POINTER(C.c_uint8)


def sha(b):
    return hashlib.sha256(b).hexdigest()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "dict_vectors.json")) as f:
        return json.load(f)


_LOADED, _EXPECT = {}, {}


def loaded(dl):
    if dl not in _LOADED:
        _LOADED[dl] = M.model_load(DC.dictionary(dl))
    return _LOADED[dl]


def expect(dl, bl, accel):
    """the model's (code, bytes) for one case of the grid; computed once, never changed"""
    key = (dl, bl, accel)
    if key not in _EXPECT:
        _EXPECT[key] = M.model_compress(loaded(dl), DC.block(bl), accel)
    return _EXPECT[key]


def spaced(datas, apart=APART, lead=3):
    """(buffer, offsets): the byte strings APART bytes apart in one buffer of FILL bytes"""
    off, pos = [], lead
    for d in datas:
        off.append(pos)
        pos += len(d) + apart
    buf = np.full(pos + 64, FILL, dtype=np.uint8)
    for o, d in zip(off, datas):
        buf[o:o + len(d)] = np.frombuffer(bytes(d), dtype=np.uint8)
    return buf, off


def dict_tensor(dl):
    """the dictionary on the device (one byte at least, so that the tensor has a pointer), and its length"""
    return _t(np.frombuffer(DC.dictionary(dl) + b"\x00", dtype=np.uint8).copy()), dl


class Batch:
    """all block lengths of the grid in one compress_dict_device call's arguments"""

    def __init__(self, S, kind, checksum=False, lens=None):
        import torch
        self.blocks = [DC.block(bl) for bl in DC.BLOCK_LENS]
        self.n = len(self.blocks)
        buf, off = spaced(self.blocks)
        self.src, self.off = _t(buf), _t(np.array(off, dtype=np.int64))
        self.len = _t(np.array([len(b) for b in self.blocks] if lens is None else lens, dtype=np.int32))
        self.kind = kind
        self.stride = S.slot_stride_ex(MAXLEN, kind, checksum)
        self.slots = torch.full((self.n * self.stride,), FILL, dtype=torch.uint8, device=DEV)
        self.flen = torch.full((self.n,), -77, dtype=torch.int32, device=DEV)

    def run(self, eng, cs, slot, accel):
        self.slots.fill_(FILL)
        self.flen.fill_(-77)
        eng.compress_dict_device(cs, slot, self.src, self.n, MAXLEN, self.slots, self.stride, self.flen, accel=accel,
                                 header_kind=self.kind, src_off=self.off, src_len=self.len, block_stride=0)
        eng.synchronize()
        fl = self.flen.cpu().tolist()
        hb = self.slots.cpu().numpy()
        return fl, [hb[i * self.stride:i * self.stride + max(fl[i], 0)].tobytes() for i in range(self.n)]


@pytest.fixture(scope="module")
def setup():
    import streamly_lz4_amd as S
    eng = S.Engine(0)
    cs = S.CompressStreams(eng, 3)
    yield S, eng, cs
    cs.close()
    eng.close()


@pytest.mark.parametrize("dl", DC.DICT_LENS)
def test_bytes(setup, vectors, dl):
    """one call carries every block length; framedLen, headers and bytes are the model's and the golden's, for accel 1 and 7 and
    both header kinds; the loaded slot is LZ4_loadDict's state, and no call writes it"""
    S, eng, cs = setup
    d, n = dict_tensor(dl)
    cs.reset()
    cs.load_dict(1, d, n)
    eng.synchronize()
    state = cs.slot_bytes(1)
    m = loaded(dl)
    assert cs.state(1) == (65536, m.keep, m.keep)
    assert state[:16384] == bytes(m.s.table), "the table differs from LZ4_loadDict's"
    assert state[16384 + 64:16384 + 64 + m.keep] == DC.dictionary(dl)[len(DC.dictionary(dl)) - m.keep:] if m.keep else True
    assert cs.state(0) == cs.state(2) == (0, 0, 0)
    for kind in (8, 4):
        b = Batch(S, kind)
        for accel in DC.ACCELS:
            fl, got = b.run(eng, cs, 1, accel)
            for i, bl in enumerate(DC.BLOCK_LENS):
                code, comp = expect(dl, bl, accel)
                assert [code, sha(comp)] == vectors["compress"][DC.compress_key(dl, bl, accel)]
                assert fl[i] == kind + code, (dl, bl, accel, kind)
                assert got[i] == M.framed_block(code, comp, bl, kind), (dl, bl, accel, kind)
            fl2, got2 = b.run(eng, cs, 1, accel)
            assert (fl2, got2) == (fl, got), "the same call gave other bytes the second time"
    assert cs.slot_bytes(1) == state, "a compress_dict_device call wrote the shared slot"


def test_bad_length_is_framed_len_zero(setup):
    """a length outside 0..maxBlockLen: framedLen 0 for that block, its slot untouched, the others unaffected"""
    S, eng, cs = setup
    dl = 4095
    d, n = dict_tensor(dl)
    cs.load_dict(1, d, n)
    lens = [len(DC.block(bl)) for bl in DC.BLOCK_LENS]
    lens[3], lens[6] = -1, MAXLEN + 1
    b = Batch(S, 8, lens=lens)
    fl, got = b.run(eng, cs, 1, 1)
    hb = b.slots.cpu().numpy()
    for i, bl in enumerate(DC.BLOCK_LENS):
        if i in (3, 6):
            assert fl[i] == 0 and (hb[i * b.stride:(i + 1) * b.stride] == FILL).all()
        else:
            code, comp = expect(dl, bl, 1)
            assert got[i] == M.framed_block(code, comp, bl, 8)


def run_stream(S, eng, cs, slot, blocks, cuts, accel):
    """the blocks through compress_streams_device on one slot, cut into calls of cuts[] blocks; [framed bytes per block]"""
    import torch
    out, at = [], 0
    mx = max(len(b) for b in blocks)
    stride = S.slot_stride_ex(mx, 8, False)
    for k in cuts:
        part = blocks[at:at + k]
        at += k
        buf, off = spaced(part)
        slots = torch.full((max(k, 1) * stride,), FILL, dtype=torch.uint8, device=DEV)
        flen = torch.full((max(k, 1),), -77, dtype=torch.int32, device=DEV)
        eng.compress_streams_device(cs, _t(buf), k, mx, [0, k], [slot], slots, stride, flen, accel=accel, header_kind=8,
                                    src_off=_t(np.array(off + [0], dtype=np.int64)), src_len=_t(np.array([len(p) for p in part] + [0], dtype=np.int32)),
                                    block_stride=0)
        eng.synchronize()
        fl, hb = flen.cpu().tolist(), slots.cpu().numpy()
        out += [hb[i * stride:i * stride + fl[i]].tobytes() for i in range(k)]
    return out


@pytest.mark.parametrize("dl", DC.DICT_LENS)
def test_loaded_stream_continues(setup, vectors, dl):
    """load_dict, then three blocks through compress_streams_device, cut into calls 1 + 2 and 3 + 0: LZ4_loadDict followed by
    LZ4_compress_fast_continue block after block -- also for dictionaries under 8 bytes, which leave only currentOffset 65536"""
    S, eng, cs = setup
    blocks = DC.stream_blocks()
    want = M.model_stream(loaded(dl), blocks, DC.STREAM_ACCEL)
    assert [[c, sha(b)] for c, b in want] == vectors["stream"][str(dl)]
    d, n = dict_tensor(dl)
    for cuts in ((1, 2), (3, 0)):
        cs.reset()
        cs.load_dict(2, d, n)
        got = run_stream(S, eng, cs, 2, blocks, cuts, DC.STREAM_ACCEL)
        assert got == [M.framed_block(c, b, len(src), 8) for (c, b), src in zip(want, blocks)], (dl, cuts)
        total = sum(len(b) for b in blocks)
        assert cs.state(2) == (65536 + total, len(blocks[-1]), min(len(blocks[-1]), 65536))


def decode_call(eng, blocks_caps, dict_t, dict_len, kind, with_cap, batch=False, fixed=None):
    """[(block, cap)] framed with `kind` headers, decoded into outputs APART bytes apart: (results, [bytes up to the capacity],
    whether every byte outside the outputs still holds FILL)"""
    import torch
    framed, boff = bytearray(), []
    for blk, cap in blocks_caps:
        boff.append(len(framed))
        framed += len(blk).to_bytes(4, "little") + (int(cap).to_bytes(4, "little") if kind == 8 else b"") + bytes(blk)
    caps = [c for _, c in blocks_caps]
    ooff, pos = [], 5
    for c in caps:
        ooff.append(pos)
        pos += c + APART
    n = len(caps)
    out = torch.full((pos + 64,), FILL, dtype=torch.uint8, device=DEV)
    res = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    fr = _t(np.frombuffer(bytes(framed) + b"\x00", dtype=np.uint8).copy())
    args = (fr, len(framed), _t(np.array(boff, dtype=np.int64)), n)
    kw = dict(header_kind=kind, fixed_uncomp=(max(caps) if fixed is None else fixed) if kind == 4 else 0,
              out_cap=_t(np.array(caps, dtype=np.int32)) if with_cap else None)
    oo = _t(np.array(ooff, dtype=np.int64))
    if batch:
        eng.decompress_batch_device(*args, out, oo, res, linked=False, **kw)
    else:
        eng.decompress_dict_device(*args, dict_t, dict_len, out, oo, res, **kw)
    eng.synchronize()
    hb, r = out.cpu().numpy(), res.cpu().tolist()
    keep = np.ones(hb.size, dtype=bool)
    for o, c in zip(ooff, caps):
        keep[o:o + c] = False
    return r, [hb[o:o + c].tobytes() for o, c in zip(ooff, caps)], bool((hb[keep] == FILL).all())


@pytest.mark.parametrize("dl", DC.DICT_LENS)
def test_decode_well_formed(setup, oracle, dl):
    """GPU blocks (accel 1) and model blocks (accel 7) decode to their sources with the dictionary; capacities exact (headers of
    kind 8, and outCap with kind 4) and 3 bytes larger"""
    S, eng, cs = setup
    d, n = dict_tensor(dl)
    cs.reset()
    cs.load_dict(1, d, n)
    _, got = Batch(S, 8).run(eng, cs, 1, 1)
    gpu_blocks = [g[8:] for g in got]
    model_blocks = [expect(dl, bl, 7)[1] for bl in DC.BLOCK_LENS]
    srcs = [DC.block(bl) for bl in DC.BLOCK_LENS] * 2
    for kind, extra, with_cap in ((8, 0, False), (4, 0, True), (4, 3, True)):
        bc = [(b, len(s) + extra) for b, s in zip(gpu_blocks + model_blocks, srcs)]
        r, outs, clean = decode_call(eng, bc, d, n, kind, with_cap)
        for i, ((blk, cap), s) in enumerate(zip(bc, srcs)):
            assert oracle.decompress_block(blk, cap, DC.dictionary(dl)) == (len(s), s)
            assert r[i] == len(s) and outs[i][:len(s)] == s, (dl, kind, extra, i)
        assert clean, "bytes outside the outputs were written"


def test_decode_without_dictionary_is_decompress_batch(setup, oracle):
    """dictLen 0 is LZ4_decompress_safe: the codes and bytes of decompress_batch_device, for blocks that need no dictionary and
    for blocks that miss theirs"""
    S, eng, cs = setup
    bc = [(expect(0, bl, 1)[1], bl) for bl in DC.BLOCK_LENS] + [(expect(4095, bl, 1)[1], bl) for bl in DC.BLOCK_LENS]
    d, _ = dict_tensor(0)
    for kind in (8, 4):
        a = decode_call(eng, bc, d, 0, kind, kind == 4)
        b = decode_call(eng, bc, None, 0, kind, kind == 4)
        c = decode_call(eng, bc, None, 0, kind, kind == 4, batch=True)
        want = [oracle.decompress_block(blk, cap) for blk, cap in bc]
        assert a[0] == b[0] == c[0] == [w[0] for w in want]
        assert a[2] and b[2] and c[2]
        for i, (code, dec) in enumerate(want):
            if code >= 0:
                assert a[1][i][:code] == b[1][i][:code] == c[1][i][:code] == dec
        assert any(w[0] < 0 for w in want[len(DC.BLOCK_LENS):]), "no block of the grid misses its dictionary"


@pytest.mark.parametrize("dl", DC.DECODE_DICT_LENS)
def test_decode_edges(setup, vectors, oracle, dl):
    """hand-built blocks on the dictionary's edges: codes and bytes are the oracle's and the golden's"""
    S, eng, cs = setup
    cases = [(i, c) for i, c in enumerate(DC.decode_cases()) if c[1] == dl]
    d, n = dict_tensor(dl)
    bc = [(blk, cap) for _, (_, _, blk, cap) in cases]
    r, outs, clean = decode_call(eng, bc, d, n, 4, True)
    assert clean, "bytes outside the outputs were written"
    for k, (i, (name, _, blk, cap)) in enumerate(cases):
        code, dec = oracle.decompress_block(blk, cap, DC.dictionary(dl))
        assert [name, dl, code, sha(dec)] == vectors["decode"][i]
        assert r[k] == code, (name, dl)
        if code >= 0:
            assert outs[k][:code] == dec, (name, dl)


def test_checksums(setup, oracle):
    """the compress call appends the trailer, the decode call verifies it; one flipped byte fails that block alone"""
    S, eng, cs = setup
    dl = 4095
    d, n = dict_tensor(dl)
    cs.reset()
    cs.load_dict(1, d, n)
    eng.set_block_checksum(True)
    try:
        import torch
        b = Batch(S, 8, checksum=True)
        fl, got = b.run(eng, cs, 1, 1)
        for i, bl in enumerate(DC.BLOCK_LENS):
            code, comp = expect(dl, bl, 1)
            x = int(S.lib.slz4_xxh32(np.frombuffer(comp, dtype=np.uint8).ctypes.data_as(_u8p), len(comp), 0))
            assert fl[i] == 8 + code + 4 and got[i] == M.framed_block(code, comp, bl, 8) + x.to_bytes(4, "little"), bl
        for flip in (None, 6):
            framed, boff = bytearray(), []
            for g in got:
                boff.append(len(framed))
                framed += g
            if flip is not None:
                framed[boff[flip] + 8 + 5] ^= 0x40
            ooff = np.cumsum([0] + [bl + APART for bl in DC.BLOCK_LENS])[:-1]
            out = torch.full((int(ooff[-1]) + MAXLEN + 64,), FILL, dtype=torch.uint8, device=DEV)
            res = torch.full((b.n,), -77, dtype=torch.int32, device=DEV)
            eng.decompress_dict_device(_t(np.frombuffer(bytes(framed), dtype=np.uint8).copy()), len(framed),
                                       _t(np.array(boff, dtype=np.int64)), b.n, d, n, out, _t(ooff.astype(np.int64)), res)
            eng.synchronize()
            r, hb = res.cpu().tolist(), out.cpu().numpy()
            for i, bl in enumerate(DC.BLOCK_LENS):
                if i == flip:
                    assert r[i] == BLK_E_CHECKSUM
                    assert (hb[ooff[i]:ooff[i] + bl] == FILL).all(), "a block that failed its checksum was decoded"
                else:
                    assert r[i] == bl and hb[ooff[i]:ooff[i] + bl].tobytes() == DC.block(bl), (flip, bl)
    finally:
        eng.set_block_checksum(False)


def test_host_buffer_forms(setup, oracle):
    """compress_dict / decompress_dict: the device calls' bytes through host buffers"""
    S, eng, cs = setup
    dl = 65537
    d, n = dict_tensor(dl)
    cs.reset()
    cs.load_dict(0, d, n)
    blocks = [DC.block(bl) for bl in DC.BLOCK_LENS]
    framed, flen = eng.compress_dict(blocks, cs, 0, accel=7)
    want = [M.framed_block(*expect(dl, bl, 7), bl, 8) for bl in DC.BLOCK_LENS]
    assert flen == [len(w) for w in want] and framed == b"".join(want)
    out, blen = eng.decompress_dict(framed, DC.dictionary(dl))
    assert blen == list(DC.BLOCK_LENS) and out == b"".join(blocks)
    out, blen = eng.decompress_dict(framed, b"", raise_on_block_error=False)
    assert any(x < 0 for x in blen) and out == b""


def test_cpp_mirror(tmp_path):
    """CompressStreams::loadDict, Engine::compressWithDict and Engine::decompressWithDict from a program of its own"""
    import subprocess
    dl, bl, n = 70000, 1000, 5
    records = b"".join(DC.text(7000 + i, bl) for i in range(n))
    exe = str(tmp_path / "dict_mirror")
    libdir = os.path.join(ROOT, "streamly-lz4_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-isystem", "/opt/rocm/include", os.path.join(ROOT, "tests", "native", "dict_mirror_main.cpp"), "-L", libdir,
                           "-lmi355lz4", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    (tmp_path / "dict.bin").write_bytes(DC.dictionary(dl))
    (tmp_path / "records.bin").write_bytes(records)
    r = subprocess.run([exe, str(tmp_path / "dict.bin"), str(tmp_path / "records.bin"), str(bl), str(tmp_path / "framed.bin"),
                        str(tmp_path / "decoded.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-300:], r.stderr)
    m = M.model_load(DC.dictionary(dl))
    want = [M.framed_block(*M.model_compress(m, records[i * bl:(i + 1) * bl], 1), bl, 8) for i in range(n)]
    assert [int(x) for x in r.stdout.split()] == [len(w) for w in want]
    assert (tmp_path / "framed.bin").read_bytes() == b"".join(want)
    assert (tmp_path / "decoded.bin").read_bytes() == records


def test_arguments(setup):
    """every MI355LZ4_E_ARG of the three device calls; nothing is enqueued: the outputs keep their pattern"""
    import torch
    S, eng, cs = setup
    L, P = S.lib, S._dptr
    d, n = dict_tensor(100)
    cs.reset()
    cs.load_dict(1, d, n)
    eng.synchronize()
    before = [cs.slot_bytes(k) for k in range(3)]
    H = cs._h
    # load_dict
    for args in ((None, H, 0, P(d), n), (eng.ctx, None, 0, P(d), n), (eng.ctx, H, -1, P(d), n), (eng.ctx, H, 3, P(d), n),
                 (eng.ctx, H, 0, P(d), -1), (eng.ctx, H, 0, None, 5)):
        assert L.mi355lz4_cstreams_load_dict(*args) == E_ARG, args
    # compress_dict_device
    b = Batch(S, 8)
    b.slots.fill_(FILL)
    b.flen.fill_(-77)

    def comp(ctx=eng.ctx, h=H, slot=1, src=b.src, nb=b.n, kind=8, mx=MAXLEN, slots=b.slots, flen=b.flen):
        return L.mi355lz4_compress_dict_device(ctx, h, slot, P(src), P(b.off), P(b.len), 0, mx, nb, 1, kind, P(slots), b.stride, P(flen))

    assert comp() == 0
    eng.synchronize()
    b.slots.fill_(FILL)
    b.flen.fill_(-77)
    for kw in (dict(ctx=None), dict(h=None), dict(slot=-1), dict(slot=3), dict(nb=-1), dict(kind=5), dict(mx=-1), dict(src=None),
               dict(slots=None), dict(flen=None)):
        assert comp(**kw) == E_ARG, kw
    eng.set_compression_level(3)
    try:
        assert comp() == E_ARG and b"compression level" in L.mi355lz4_last_error()
    finally:
        eng.set_compression_level(0)
    # decompress_dict_device
    blk = expect(100, 1000, 1)[1]
    framed = len(blk).to_bytes(4, "little") + (1000).to_bytes(4, "little") + blk
    fr, boff, ooff = _t(np.frombuffer(framed, dtype=np.uint8).copy()), _t(np.zeros(1, dtype=np.int64)), _t(np.zeros(1, dtype=np.int64))
    out = torch.full((1064,), FILL, dtype=torch.uint8, device=DEV)
    res = torch.full((1,), -77, dtype=torch.int32, device=DEV)

    def dec(ctx=eng.ctx, framed=fr, boff=boff, nb=1, kind=8, fixed=0, dct=d, dlen=n, ooff=ooff, res=res):
        return L.mi355lz4_decompress_dict_device(ctx, P(framed), len(framed) if framed is not None else 0, P(boff), nb, kind, fixed,
                                                 P(dct), dlen, P(out), P(ooff), None, P(res))

    for kw in (dict(ctx=None), dict(nb=-1), dict(fixed=-1), dict(kind=5), dict(framed=None), dict(boff=None), dict(ooff=None),
               dict(res=None), dict(dlen=-1), dict(dct=None)):
        assert dec(**kw) == E_ARG, kw
    eng.synchronize()
    assert (b.slots == FILL).all() and (b.flen == -77).all() and (out == FILL).all() and (res == -77).all()
    assert [cs.slot_bytes(k) for k in range(3)] == before
    assert dec() == 0 and dec(nb=0, framed=None, boff=None, ooff=None, res=None) == 0
    eng.synchronize()
    assert res.cpu().tolist() == [1000] and out[:1000].cpu().numpy().tobytes() == DC.block(1000)
