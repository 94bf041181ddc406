"""Linked-stream decode at a size where the rate means something: streams written by the
reference's own linked compressor (oracle on the host), decoded by the GPU in one call, checked
bit-exact, and the rate recorded in measurements/linked_rate.jsonl.  The oracle is only the data source
and the checker here; the timed region is the GPU call."""
import numpy as np
import pytest

from test_parity_gpu import _stream_layout

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_streams,blocks_per_stream", [(2048, 2), (512, 8), (8, 64)])
def test_linked_stream_rate(engine, slz4, oracle, n_streams, blocks_per_stream, record):
    import torch
    dev = torch.device("cuda:0")
    bl = 65536
    # a handful of distinct streams, repeated: host compression stays at a few seconds
    distinct = min(n_streams, 16)
    datas = [oracle.gen("text", blocks_per_stream, bl, first_block=1000 * s).tobytes() for s in range(distinct)]
    frs_d = [oracle.frame_compress(d, bl, 1, 8, True) for d in datas]
    frs = [frs_d[s % distinct] for s in range(n_streams)]
    blob, boff, first, ulen = _stream_layout(frs)
    nb = len(boff)
    buf = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    off = torch.tensor(boff, dtype=torch.int64, device=dev)
    ooff = torch.arange(nb + 1, dtype=torch.int64, device=dev) * bl
    out = torch.zeros(nb * bl, dtype=torch.uint8, device=dev)
    res = torch.zeros(nb, dtype=torch.int32, device=dev)
    sf = torch.tensor(first, dtype=torch.int32, device=dev)
    e0, e1 = slz4.Event(), slz4.Event()
    best = 1e9
    for _ in range(3):
        engine.record(e0)
        engine.decompress_streams_device(buf, len(blob), off, nb, sf, n_streams, out, ooff, res)
        engine.record(e1)
        engine.synchronize()
        best = min(best, engine.elapsed_ms(e0, e1))
    assert bool((res == bl).all().item())
    ref = torch.from_numpy(np.frombuffer(b"".join(datas), dtype=np.uint8).copy()).to(dev)
    per = blocks_per_stream * bl
    for s in range(0, n_streams, max(1, n_streams // 64)):
        d = s % distinct
        assert torch.equal(out[s * per:(s + 1) * per], ref[d * per:(d + 1) * per]), s
    # how many blocks really needed their predecessor
    engine.decompress_batch_device(buf, len(blob), off, nb, out, ooff, res, linked=False)
    engine.synchronize()
    dependent = int((res < 0).sum().item())
    rate = nb * bl / best / 1e6
    rec = {"streams": n_streams, "blocks_per_stream": blocks_per_stream, "block_len": bl, "data": "text, reference-linked",
           "dependent_blocks": dependent, "blocks": nb, "ms": round(best, 3), "GBps_uncompressed": round(rate, 2)}
    record("linked_rate", rec)
    print(rec)


def test_linked_flag_is_free_on_independent_blocks(engine, slz4, record):
    """linked = 1 on a stream in which every block decodes standalone (what this engine's compressor writes,
    and what the C++ mirror / LZ4_decompress_safe_continue always pass) must cost nothing measurable: the
    call only waits for the first pass to learn that no block needs a second one."""
    import torch
    dev = torch.device("cuda:0")
    bl, nb = 65536, 16384
    src = torch.empty(nb * bl, dtype=torch.uint8, device=dev)
    engine.generate("lzsynth", src, bl, nb)
    stride = slz4.slot_stride(bl, 8)
    slots = torch.empty(nb * stride, dtype=torch.uint8, device=dev)
    flen = torch.empty(nb, dtype=torch.int32, device=dev)
    dense = torch.empty(nb * stride, dtype=torch.uint8, device=dev)
    doff = torch.empty(nb + 1, dtype=torch.int64, device=dev)
    ooff = torch.arange(nb + 1, dtype=torch.int64, device=dev) * bl
    out = torch.empty(nb * bl, dtype=torch.uint8, device=dev)
    res = torch.empty(nb, dtype=torch.int32, device=dev)
    engine.compress_batch_device(src, nb, bl, slots, stride, flen)
    engine.compact_device(slots, stride, flen, nb, dense, nb * stride, doff)
    e0, e1 = slz4.Event(), slz4.Event()
    best = {}
    for linked in (False, True, False, True):
        t = 1e9
        for _ in range(4):
            engine.record(e0)
            engine.decompress_batch_device(dense, nb * stride, doff, nb, out, ooff, res, linked=linked)
            engine.record(e1)
            engine.synchronize()
            t = min(t, engine.elapsed_ms(e0, e1))
        assert bool((res == bl).all().item()) and torch.equal(out, src)
        best[linked] = min(best.get(linked, 1e9), t)
    rec = {"test": "linked flag on independent blocks", "blocks": nb, "ms_linked0": round(best[False], 4),
           "ms_linked1": round(best[True], 4)}
    record("linked_rate", rec)
    print(rec)
    # one stream synchronisation (tens of microseconds), never a walk over the blocks (tens of milliseconds)
    assert best[True] <= best[False] * 1.05 + 0.05, rec


@pytest.mark.parametrize("kind,n_blocks,repeat,bl", [("text", 1024, 1, 65536), ("lzsynth_shared", 512, 1, 65536),
                                                     ("text", 1024, 10, 65536), ("text", 256, 4, 262144),
                                                     ("text", 64, 4, 1 << 20)])
def test_single_linked_stream_rate(engine, slz4, oracle, kind, n_blocks, repeat, bl, record):
    """ONE long stream written by the reference's linked compressor (what a reference-written file is): the
    tolerant parallel pass + the data-parallel pointer pass (linked_ptr.hpp).  Bit-exact; the rate is recorded.
    repeat > 1: the framed stream is appended to itself (still one valid linked stream: a block written without
    a dictionary may follow any block), long enough to span several segments of the second pass (the 10 240-block case
    is above the span from which the run-in decode is the default: kernels/runin.inc, "RUN-IN DECODE")."""
    import torch
    dev = torch.device("cuda:0")
    if kind == "text":
        data = oracle.gen("text", n_blocks * (bl // 65536), 65536, first_block=7).tobytes()
    else:
        # every block built from the same vocabulary as its predecessor: long matches across the block seam
        base = oracle.gen("lzsynth", 2, bl, first_block=3).tobytes()
        rng = np.random.default_rng(5)
        parts = []
        for i in range(n_blocks):
            o = int(rng.integers(0, bl))
            parts.append(base[o:o + bl])
        data = b"".join(parts)
    fr = oracle.frame_compress(data, bl, 1, 8, True) * repeat
    data = data * repeat
    nb = n_blocks * repeat
    offs, pos = [], 0
    for _ in range(nb):
        offs.append(pos)
        pos += 8 + int.from_bytes(fr[pos:pos + 4], "little")
    assert pos == len(fr)
    buf = torch.from_numpy(np.frombuffer(fr, dtype=np.uint8).copy()).to(dev)
    off = torch.tensor(offs + [pos], dtype=torch.int64, device=dev)
    ooff = torch.arange(nb + 1, dtype=torch.int64, device=dev) * bl
    out = torch.zeros(nb * bl, dtype=torch.uint8, device=dev)
    res = torch.zeros(nb, dtype=torch.int32, device=dev)
    engine.decompress_batch_device(buf, len(fr), off, nb, out, ooff, res, linked=False)
    engine.synchronize()
    dependent = int((res < 0).sum().item())
    e0, e1 = slz4.Event(), slz4.Event()
    best = 1e9
    for _ in range(3):
        out.zero_()
        engine.record(e0)
        engine.decompress_batch_device(buf, len(fr), off, nb, out, ooff, res, linked=True)
        engine.record(e1)
        engine.synchronize()
        best = min(best, engine.elapsed_ms(e0, e1))
    assert bool((res == bl).all().item())
    ref = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    assert torch.equal(out, ref)
    rec = {"streams": 1, "blocks_per_stream": nb, "block_len": bl, "data": kind + ", reference-linked", "dependent_blocks": dependent,
           "ms": round(best, 3), "GBps_uncompressed": round(nb * bl / best / 1e6, 3), "ratio": round(nb * bl / len(fr), 3)}
    record("linked_rate", rec)
    print(rec)


@pytest.mark.parametrize("linked", [0, 1])
def test_single_linked_stream_host_api_rate(engine, slz4, oracle, linked, record):
    """The same kind of stream through the host-buffer call (page-locked caller memory, PCIe-inclusive):
    the call is cut into groups, and the second pass of a group looks back into the groups before it.
    linked = 0 on the engine's own independent blocks of the same data is the yardstick."""
    import ctypes as C
    import time
    import torch
    bl, nb0, repeat = 65536, 1024, 8
    data = oracle.gen("text", nb0, bl, first_block=7).tobytes()
    if linked:
        fr = oracle.frame_compress(data, bl, 1, 8, True) * repeat
    else:
        blocks = [data[i * bl:(i + 1) * bl] for i in range(nb0)]
        fr = engine.compress_batch(blocks)[0] * repeat
    data = data * repeat
    nb = nb0 * repeat
    u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    framed_t = torch.from_numpy(np.frombuffer(fr, dtype=np.uint8).copy()).pin_memory()
    out_t = torch.empty(nb * bl, dtype=torch.uint8).pin_memory()
    framed, out = framed_t.numpy(), out_t.numpy()
    blen = np.zeros(nb, dtype=np.int32)
    dlen, got = C.c_size_t(), C.c_int()
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        rc = slz4.lib.mi355lz4_decompress_batch(engine.ctx, framed.ctypes.data_as(u8p), framed.size, 8, 0, linked, None, 0,
                                                out.ctypes.data_as(u8p), out.size, C.byref(dlen), blen.ctypes.data_as(i32p),
                                                nb, C.byref(got))
        best = min(best, time.perf_counter() - t0)
        assert rc == 0 and dlen.value == nb * bl and got.value == nb, slz4.lib.mi355lz4_last_error()
    assert out.tobytes() == data
    rec = {"api": "host-buffer C API, page-locked caller memory", "streams": 1, "blocks_per_stream": nb, "block_len": bl,
           "data": "text, " + ("reference-linked" if linked else "independent blocks (this engine's)"), "linked": linked,
           "ms": round(best * 1e3, 3), "GBps_uncompressed": round(nb * bl / best / 1e9, 3)}
    record("linked_rate", rec)
    print(rec)


def test_long_linked_stream_default_is_runin_decode(engine, slz4, oracle, monkeypatch, record):
    """ONE reference-written linked stream long enough (9 216 blocks of 64 KiB and more) that the default path is the
    run-in decode (pieces of the stream, each decoded from 11 blocks in front of it, kernels/runin.inc): its output must be the
    input, and the same bytes as the pointer pass's (MI355LZ4_LINKED_RUNIN=0).  Rates go to linked_rate.jsonl."""
    import torch
    dev = torch.device("cuda:0")
    # Two copies of one stream of 6272 blocks laid end to end: still ONE valid linked stream, because the reference wrote the
    # copy's first block without a dictionary.  That block (index 6272) decodes in the first pass, so the pieces whose run-in
    # would cross it start behind it with their TRUE dictionary in the middle of a segment (the twin decode of this round's
    # first half got a case like it wrong in development: bench.py's check found it).  The last piece is ragged.
    bl, nb1, base = 65536, 6272, 1024
    d1 = oracle.gen("text", base, bl, first_block=555).tobytes()
    d1 = (d1 * ((nb1 + base - 1) // base))[: nb1 * bl]
    fr1 = oracle.frame_compress(d1, bl, 1, 8, True)
    cut, extra = 0, 250                                   # ... plus the first 250 blocks a third time (a ragged last piece)
    for _ in range(extra):
        cut += 8 + int.from_bytes(fr1[cut:cut + 4], "little")
    data, fr, nb = d1 + d1 + d1[: extra * bl], fr1 + fr1 + fr1[:cut], 2 * nb1 + extra
    assert nb - 1 >= 9216
    offs = np.zeros(nb + 1, dtype=np.int64)
    pos = 0
    for i in range(nb):
        offs[i] = pos
        pos += 8 + int.from_bytes(fr[pos:pos + 4], "little")
    offs[nb] = pos
    buf = torch.from_numpy(np.frombuffer(fr, dtype=np.uint8).copy()).to(dev)
    off = torch.from_numpy(offs).to(dev)
    ooff = torch.arange(nb + 1, dtype=torch.int64, device=dev) * bl
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    res = torch.zeros(nb, dtype=torch.int32, device=dev)
    e0, e1 = slz4.Event(), slz4.Event()
    rates = {}
    for label, env in (("run-in (default)", None), ("pointer pass", "0")):
        if env is None:
            monkeypatch.delenv("MI355LZ4_LINKED_RUNIN", raising=False)
        else:
            monkeypatch.setenv("MI355LZ4_LINKED_RUNIN", env)
        out = torch.zeros(nb * bl, dtype=torch.uint8, device=dev)
        best = 1e9
        for _ in range(2):
            engine.record(e0)
            engine.decompress_batch_device(buf, len(fr), off, nb, out, ooff, res, linked=True)
            engine.record(e1)
            engine.synchronize()
            best = min(best, engine.elapsed_ms(e0, e1))
        assert bool((res == bl).all().item()) and torch.equal(out, src), label
        rates[label] = round(nb * bl / best / 1e6, 2)
        del out
    rec = {"streams": 1, "blocks": nb, "block_len": bl, "data": "text, reference-linked, one stream", "GBps_uncompressed": rates}
    record("linked_rate", rec)
    print(rec)
    assert rates["run-in (default)"] > rates["pointer pass"]
    import ctypes as C
    st = (C.c_int * 5)()
    monkeypatch.delenv("MI355LZ4_LINKED_RUNIN", raising=False)
    engine.decompress_batch_device(buf, len(fr), off, nb, torch.zeros(nb * bl, dtype=torch.uint8, device=dev), ooff, res, linked=True)
    engine.synchronize()
    slz4.lib.mi355lz4_debug_runin_state(engine.ctx, st, None)
    assert list(st)[:3] == [0, 0, 0] and st[4] == 2, list(st)       # the default run-in, chosen from the sample (share st[3] / 1e6)
    # The same stream with payload bytes of three blocks corrupted: whatever the run-in decode does with it (a block that fails
    # with its dictionary sends the span to the pointer pass), results and bytes must be those of the
    # pointer pass alone -- which tests/test_parity_gpu.py holds against the oracle's codes on short streams.
    bad = buf.clone()
    for blk in (5000, 5001, nb - 3):
        p0 = int(offs[blk]) + 8
        n = int(offs[blk + 1]) - p0
        bad[p0 + n // 2:p0 + n // 2 + 48] = 0xff           # (tokens of 0xff: length fields that run past the block)
    outs = {}
    for label, env in (("runin", None), ("pointer", "0")):
        if env is None:
            monkeypatch.delenv("MI355LZ4_LINKED_RUNIN", raising=False)
        else:
            monkeypatch.setenv("MI355LZ4_LINKED_RUNIN", env)
        out = torch.zeros(nb * bl, dtype=torch.uint8, device=dev)
        r = torch.zeros(nb, dtype=torch.int32, device=dev)
        engine.decompress_batch_device(bad, len(fr), off, nb, out, ooff, r, linked=True)
        engine.synchronize()
        outs[label] = (r.cpu().numpy().copy(), out)
    r_t, o_t = outs["runin"]
    r_p, o_p = outs["pointer"]
    assert (r_t == r_p).all(), np.nonzero(r_t != r_p)[0][:8]
    assert (r_p <= 0).any()                                  # (the corruption was felt)
    good = torch.from_numpy((r_p == bl)).to(dev)
    same = (o_t.view(nb, bl) == o_p.view(nb, bl)).all(dim=1)
    assert bool((same | ~good).all().item())


def _copying_stream(nb, bl=65536):
    """(bytes, framed): a linked stream written by hand in which every block but the first is ONE match that copies the block from
    65535 bytes back (the data is noise of period 65535) and five literals: legal LZ4, and every byte derives from the first
    block -- a run-in from anywhere else never arrives at the true bytes.  (The reference's own compressor does not write such
    streams: on periodic noise it finds its matches in every other block only -- the blocks in between are literals and stand
    alone -- and on blocks that repeat the block before them with changes its 4096-entry table has lost most of the positions
    65 000 bytes back: the sampled share stays at 0.12.)"""
    import random
    pat = random.Random(11).randbytes(65535)
    data = (pat * (nb * bl // 65535 + 2))[: nb * bl]
    ml = bl - 5 - 4 - 15
    first = b"\xf0" + b"\xff" * ((bl - 15) // 255) + bytes([(bl - 15) % 255]) + data[:bl]
    out = [len(first).to_bytes(4, "little") + bl.to_bytes(4, "little") + first]
    head = b"\x0f\xff\xff" + b"\xff" * (ml // 255) + bytes([ml % 255]) + b"\x50"
    for k in range(1, nb):
        c = head + data[(k + 1) * bl - 5:(k + 1) * bl]
        out.append(len(c).to_bytes(4, "little") + bl.to_bytes(4, "little") + c)
    return data, b"".join(out)


def test_long_linked_stream_that_never_forgets(slz4, oracle, record):
    """A long stream whose every block IS the block before it (_copying_stream, written by hand): no run-in arrives at the true
    dictionary.  The engine reads that off a sample of the stream's blocks (all of their bytes come directly from the block
    before: api.cpp, k_dict_share) and takes the pointer pass from the first call on -- without the sample the run-in decode
    gives the first call up and the engine learns it that way.  Bytes and results exact every time (the oracle decodes a short
    stream of the same make); an engine of its own, so that the shared one keeps its defaults."""
    import torch
    dev = torch.device("cuda:0")
    eng = slz4.Engine(0)
    bl, nb = 65536, 9472
    d6, f6 = _copying_stream(6, bl)
    assert oracle.frame_decompress(f6, len(d6), 8, bl, True) == d6
    data, fr = _copying_stream(nb, bl)
    offs = np.zeros(nb + 1, dtype=np.int64)
    pos = 0
    for i in range(nb):
        offs[i] = pos
        pos += 8 + int.from_bytes(fr[pos:pos + 4], "little")
    offs[nb] = pos
    buf = torch.from_numpy(np.frombuffer(fr, dtype=np.uint8).copy()).to(dev)
    off = torch.from_numpy(offs).to(dev)
    ooff = torch.arange(nb + 1, dtype=torch.int64, device=dev) * bl
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    e0, e1 = slz4.Event(), slz4.Event()
    ms = []
    for _ in range(3):
        out = torch.zeros(nb * bl, dtype=torch.uint8, device=dev)
        res = torch.zeros(nb, dtype=torch.int32, device=dev)
        eng.record(e0)
        eng.decompress_batch_device(buf, len(fr), off, nb, out, ooff, res, linked=True)
        eng.record(e1)
        eng.synchronize()
        ms.append(round(eng.elapsed_ms(e0, e1), 3))
        assert bool((res == bl).all().item()) and torch.equal(out, src)
        del out
    # (straight to the pointer pass from the first call on: the sample of the stream's blocks says that it never forgets its
    # dictionary; the engine's state stays as it was: no call was given up)
    import ctypes as C
    st = (C.c_int * 5)()
    slz4.lib.mi355lz4_debug_runin_state(eng.ctx, st, None)
    assert list(st)[:3] == [0, 0, 0] and st[3] >= 600000 and st[4] == 5, list(st)
    rec = {"streams": 1, "blocks": nb, "block_len": bl, "data": "every block one match that copies the block before it, hand-written, one stream",
           "sampled_dictionary_share": st[3] / 1e6, "ms_first_call": ms[0], "ms_next_calls": ms[1:]}
    record("linked_rate", rec)
    print(rec)


def test_long_engine_written_linked_stream_takes_the_long_run_in(slz4, monkeypatch, record):
    """The engine's own linked compressor takes half of a text block from the block before it (the reference's: a third), and
    its streams forget a missing dictionary after 9 to 15 blocks instead of 5 to 12: the default run-in would give
    a call up (round 5: the first call of an engine, 43 ms, then 22); the engine reads the stream's kind off a sample of its blocks and
    takes the long run-in from the first call on.  Bytes and results exact every time; the rates are
    recorded.  An engine of its own.  Its scratch is reserved before the timed calls by one call that forces the same
    run-in (MI355LZ4_LINKED_RUNIN: such a call neither samples nor touches what the engine has learnt), so that the first
    timed call is still the engine's first choice of path but not its first allocation: a fresh 640 MiB of device memory
    takes anywhere from 0.04 ms to a second, depending on what the device's memory went through before."""
    import torch
    dev = torch.device("cuda:0")
    eng = slz4.Engine(0)
    eng.set_linked_compress(True)
    bl, nb = 65536, 20480
    src = torch.empty(nb * bl, dtype=torch.uint8, device=dev)
    eng.generate("text", src, bl, nb)
    stride = slz4.slot_stride(bl, 8)
    slots = torch.empty(nb * stride, dtype=torch.uint8, device=dev)
    flen = torch.empty(nb, dtype=torch.int32, device=dev)
    dense = torch.empty(nb * stride, dtype=torch.uint8, device=dev)
    doff = torch.empty(nb + 1, dtype=torch.int64, device=dev)
    eng.compress_batch_device(src, nb, bl, slots, stride, flen)
    eng.compact_device(slots, stride, flen, nb, dense, nb * stride, doff)
    eng.synchronize()
    del slots
    clen = int(doff[-1].item())
    ooff = torch.arange(nb + 1, dtype=torch.int64, device=dev) * bl
    res = torch.zeros(nb, dtype=torch.int32, device=dev)
    out = torch.zeros(nb * bl, dtype=torch.uint8, device=dev)
    eng.decompress_batch_device(dense, clen, doff, nb, out, ooff, res, linked=False)
    eng.synchronize()
    assert int((res < 0).sum().item()) >= nb - 8              # (the stream really is linked)
    import ctypes as C
    st = (C.c_int * 5)()
    monkeypatch.setenv("MI355LZ4_LINKED_RUNIN", "1")
    monkeypatch.setenv("MI355LZ4_LINKED_RUNIN_BLOCKS", "17")     # (RUNIN_LONG_64K: the run-in the timed calls take)
    eng.decompress_batch_device(dense, clen, doff, nb, out, ooff, res, linked=True)
    eng.synchronize()
    monkeypatch.delenv("MI355LZ4_LINKED_RUNIN")
    monkeypatch.delenv("MI355LZ4_LINKED_RUNIN_BLOCKS")
    assert bool((res == bl).all().item()) and torch.equal(out, src)
    slz4.lib.mi355lz4_debug_runin_state(eng.ctx, st, None)
    assert list(st) == [0, 0, 0, -1, 2], list(st)                 # run-in, no sample taken, nothing learnt
    e0, e1 = slz4.Event(), slz4.Event()
    ms = []
    for _ in range(3):
        out.zero_()
        res.zero_()
        eng.record(e0)
        eng.decompress_batch_device(dense, clen, doff, nb, out, ooff, res, linked=True)
        eng.record(e1)
        eng.synchronize()
        ms.append(round(eng.elapsed_ms(e0, e1), 3))
        assert bool((res == bl).all().item()) and torch.equal(out, src)
    rec = {"streams": 1, "blocks": nb, "block_len": bl, "data": "text, linked stream written by this engine, one stream",
           "ratio": round(nb * bl / clen, 3), "ms_first_call": ms[0], "ms_next_calls": ms[1:],
           "GBps_uncompressed_next_calls": round(nb * bl / min(ms[1:]) / 1e6, 2)}
    record("linked_rate", rec)
    print(rec)
    # the long run-in is taken from the FIRST call on: how long the stream remembers a dictionary is read off a sample of its
    # blocks (api.cpp, k_dict_share), no longer learnt from a call given up (round 5: 43 ms, then 22)
    slz4.lib.mi355lz4_debug_runin_state(eng.ctx, st, None)
    assert list(st)[:3] == [0, 0, 0] and st[4] == 3, list(st)       # nothing was given up, nothing learnt; the long run-in
    assert ms[0] < 1.5 * min(ms[1:]), ms
