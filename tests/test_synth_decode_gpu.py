"""Every GPU decoder on the hand-built blocks of tests/lz4_synth.py: lengths, offsets, tokens and match ends placed on the
decoders' internal limits, parse-adversarial streams, deep dependence chains, end rules and capacities, dictionaries -- blocks
that no compressor writes on purpose.  Every result code and every byte must be the oracle's.  The workgroup-per-block decoder's
diagnostics (decode_cu.hpp, 16 words a block) say which of its forms ran: the tests check that the blocks meant to stay in the
parallel parse did, and that its fallbacks (why 2: too many candidates, 5: a sequential step failed, 6: the bail of variant 0)
were reached with the right answer all the same.  Why 4 (64 sweeps of the pointer jumping) is not reached by any valid stream:
a segment holds at most 32 768 output bytes, so no chain is deeper than 2^15 and 16 sweeps of every wave resolve any segment;
the bound only guarantees the loop's exit."""
import ctypes as C
import os

import numpy as np
import pytest

import lz4_synth as S
from conftest import DECODERS
from test_cu_decode_gpu import _linked_device_call
from test_parity_gpu import LINKED_VARIANTS, _decode_streams

pytestmark = pytest.mark.gpu

# variant 0 (the library's own choice) too, except in the experiment build's child run, which is about variant 3 alone
_VARIANTS = DECODERS + ([] if os.environ.get("MI355LZ4_TEST_ONLY_DECODER") else [0])


@pytest.fixture(scope="module")
def cases():
    return S.independent_cases()


@pytest.fixture(params=list(LINKED_VARIANTS))
def linked_variant(request, monkeypatch):
    for k, v in LINKED_VARIANTS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def _batches(cases, sizes=(37, 64, 5, 100, 1)):
    """ragged batches of cases, in order"""
    out, i, k = [], 0, 0
    while i < len(cases):
        n = sizes[k % len(sizes)]
        out.append(cases[i:i + n])
        i, k = i + n, k + 1
    return out


def _check_batch(oracle, batch, out, res, what):
    o = 0
    for c, r in zip(batch, res):
        code, dec = oracle.decompress_block(c.block, c.cap)
        assert r == code, (what, c, r, code)
        if code >= 0:
            assert out[o:o + code] == dec, (what, c, "bytes differ at",
                                            int(np.argmax(np.frombuffer(out[o:o + code], np.uint8) != np.frombuffer(dec, np.uint8))))
        o += c.cap


def _decode(engine, batch, dbg=None):
    import torch
    import streamly_lz4_amd as S_
    fr = S.framed([(c.block, c.cap) for c in batch])
    if dbg is None:
        out, res, _, _ = _decode_streams(engine, [fr], "batch")
        return out, res
    S_.lib.mi355lz4_debug_cu(engine.ctx, C.c_void_p(dbg.data_ptr()))
    try:
        out, res, _, _ = _decode_streams(engine, [fr], "batch")
    finally:
        S_.lib.mi355lz4_debug_cu(engine.ctx, None)
    torch.cuda.synchronize()
    return out, res


@pytest.mark.parametrize("decoder", _VARIANTS)
def test_synth_blocks(engine, oracle, cases, decoder):
    """Every family, ragged batches with 8-byte headers (every block carries its own capacity): the oracle's codes and bytes."""
    engine.set_decoder(decoder)
    try:
        for j, batch in enumerate(_batches(cases)):
            out, res = _decode(engine, batch)
            _check_batch(oracle, batch, out, res, (decoder, j))
    finally:
        engine.set_decoder(0)


def test_cu_form_was_exercised(engine, oracle, cases, record):
    """Variant 4 with its diagnostics: the blocks meant for the parallel parse end with why 0 and a first segment of sequences; the
    self-similar streams of 5 and more disjoint chains overflow the candidates (why 2); invalid blocks fail in a sequential step
    (why 5); the bytes and codes are the oracle's either way."""
    import torch
    engine.set_decoder(4)
    whys, wrong = {}, []
    try:
        for j, batch in enumerate(_batches(cases)):
            dbg = torch.zeros(len(batch) * 16, dtype=torch.int32, device="cuda:0")
            out, res = _decode(engine, batch, dbg)
            _check_batch(oracle, batch, out, res, ("cu", j))
            d = dbg.view(len(batch), 16).cpu().numpy().astype(np.uint32)
            for c, row in zip(batch, d):
                ran = row[15] != 0
                why = int(row[0]) if ran else None
                whys.setdefault((c.family, why), []).append(c.name)
                if c.form and not (ran and why == 0 and (row[1] & 0xFFFF) > 0):
                    wrong.append((c, why, int(row[1])))
                if c.name.startswith("self-similar period") and int(c.name.split()[-1]) >= 5 and why != 2:
                    wrong.append((c, why, int(row[1])))
    finally:
        engine.set_decoder(0)
    record("synth_cu_why", {"%s/%s" % k: v for k, v in sorted(whys.items(), key=str)})
    assert not wrong, wrong
    for fam in ("lengths", "offsets", "placement", "depth"):
        assert any(c.form for c in cases if c.family == fam), fam        # (each of them asserted one by one above)
    assert any(k[1] == 2 for k in whys), sorted(whys)
    assert any(k[1] == 5 for k in whys), sorted(whys)


def test_cu_bail_of_variant_0(engine, oracle):
    """A block whose segments end after under 2 KiB again and again (600-byte literal runs: a sequential step each) is taken back
    to the lane-parallel decoder by variant 0 (why 6), with the oracle's bytes."""
    import torch
    blk, n = S.bail_block()
    assert len(blk) * 16 <= n * 15                          # (else the kernel would not try it in this form at all)
    batch = [S.Case("bail", "bail", blk, n, True, False)] * 4
    dbg = torch.zeros(len(batch) * 16, dtype=torch.int32, device="cuda:0")
    engine.set_decoder(0)
    out, res = _decode(engine, batch, dbg)
    _check_batch(oracle, batch, out, res, "bail")
    d = dbg.view(len(batch), 16).cpu().numpy().astype(np.uint32)
    assert all(row[15] != 0 and row[0] == 6 for row in d), d[:, :2].tolist()


def _dict_expect(oracle, streams):
    """the oracle's linked decode of the streams one after another, as ONE stream: [(code, bytes or None)]"""
    return S.linked_expect(oracle, [x for st in streams for x in st])


def _check_linked(out, res, ulen, expect, what):
    o = 0
    for j, ((code, dec), u) in enumerate(zip(expect, ulen)):
        assert res[j] == code, (what, j, res[j], code)
        if dec is not None:
            assert out[o:o + len(dec)] == dec, (what, j)
        o += u


def test_synth_dictionary_linked(engine, oracle, linked_variant):
    """The dictionary family as one linked stream and as many streams, under every linked path: the oracle's block-by-block
    linked decode (a block's dictionary is the last block in front of it that decoded)."""
    streams = S.dictionary_streams()
    frs = [S.framed([(b, c) for _, b, c, _ in st]) for st in streams]
    out, res, ulen, _ = _decode_streams(engine, [b"".join(frs)], "one")
    _check_linked(out, res, ulen, _dict_expect(oracle, streams), (linked_variant, "one"))
    out, res, ulen, _ = _decode_streams(engine, frs, "streams")
    _check_linked(out, res, ulen, [e for st in streams for e in S.linked_expect(oracle, st)], (linked_variant, "streams"))


def test_synth_dictionary_given_to_the_call(engine, oracle):
    """decompress_batch(..., linked, dict_bytes): every tail of every dictionary stream, with the output of the last block in
    front of it that decoded as the call's dictionary."""
    for st in S.dictionary_streams():
        expect = S.linked_expect(oracle, st)
        for k in range(1, len(st)):
            d = next((dec for code, dec in reversed(expect[:k]) if code > 0), None)
            out, blen = engine.decompress_batch(S.framed([(b, c) for _, b, c, _ in st[k:]]), linked=True, dict_bytes=d,
                                                raise_on_block_error=False)
            assert blen == [code for code, _ in expect[k:]], (k, blen)
            if all(code >= 0 for code, _ in expect[k:]):          # (a call with a failed block delivers no bytes)
                assert out == b"".join(dec for code, dec in expect[k:]), k


@pytest.mark.parametrize("stop_after", [None, 2 * S.SPARSE_STEP])
def test_big_linked_sparse_dependence(engine, oracle, monkeypatch, stop_after):
    """Path 6 (big linked blocks, k_decode_cu_linked) on 1 MiB blocks whose dependence on the dictionary is 4 bytes carried every
    65535 bytes to the block's end: 65531 bytes between them come out the same pass after pass, just under the 64 KiB after which
    a pass stops early (decode_cu.hpp, `again`), so every later pass must decode the whole block.  With stop_after the dependence
    ends early in every block and the early stop fires.  Bytes and results: the oracle's and the pointer pass's (LINKED_BIG=0)."""
    import streamly_lz4_amd as S_
    monkeypatch.delenv("MI355LZ4_LINKED_BIG", raising=False)
    blocks = S.sparse_dependence_stream(stop_after=stop_after)
    nblk = len(blocks)
    fr = S.framed([(b, S.BIG) for b in blocks])
    expect = S.linked_expect(oracle, [("", b, S.BIG, True) for b in blocks])
    raw = b"".join(dec for _, dec in expect)
    assert [code for code, _ in expect] == [S.BIG] * nblk
    out, res, path = _linked_device_call(S_, engine, fr, nblk, S.BIG, len(raw))
    assert path == 6, path
    assert res == [S.BIG] * nblk
    if out != raw:
        a, b = np.frombuffer(out, np.uint8), np.frombuffer(raw, np.uint8)
        bad = np.nonzero(a != b)[0]
        raise AssertionError(("bytes differ", len(bad), (bad[:8] // S.BIG).tolist(), (bad[:8] % S.BIG).tolist()))
    monkeypatch.setenv("MI355LZ4_LINKED_BIG", "0")
    out0, res0, path0 = _linked_device_call(S_, engine, fr, nblk, S.BIG, len(raw))
    assert path0 != 6 and res0 == res and out0 == raw
