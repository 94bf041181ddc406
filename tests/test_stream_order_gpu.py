"""Every device call's stream contract on a NON-BLOCKING stream (include/mi355lz4.h, "Streams").

The header says that every *_device call only enqueues work on the engine's stream, and the product's default configuration is
the engine's own non-blocking stream.  The rest of the suite runs the engine on the legacy null stream, where a kernel, memset or
copy issued to the wrong stream, a scratch buffer reused too early and a missing event wait are still ordered.  Here every call
runs on torch.cuda.Stream() with LATE input (tests/stream_order.py): the inputs hold a valid decoy and the outputs a fill pattern;
then, with no synchronisation in between, a delay, an event `gate`, copies of the real input over the decoy, the call, copies of
the outputs into `kept`, and the decoy back.  `kept` must equal what the same call gave on the default stream, byte for byte.
A call that read too early gives the decoy's outputs, one that wrote too late leaves the fill pattern.

"Only enqueues" is a condition: right after the call returns, gate.query() is False -- the delay (10 x the call's own warm host
time, calibrated, recorded in measurements/stream_order.jsonl) has not ended, so the call did not wait for its stream.  It is
asserted on warm calls of every call whose header comment says it only enqueues.  Exempt, because the header lets them wait (they
are still held to the ordering verdict):
  mi355lz4_decompress_batch_device with linked != 0 and no mi355lz4_set_linked_async  (waits for its first pass)
  mi355lz4_decompress_streams_device                                                 (always waits)
  mi355lz4_compress_batch_device in reference-exact mode                             (reads the lengths, verifies its pieces)
  the fifth and later of five stream-table calls in flight (dstreams, cstreams, fstreams: the table ring has four entries)
  the first use of a scratch (allocation), a scratch that grows, a fifth stream that takes over a scratch (hipStreamSynchronize)
No late-input case (tests/stream_order.py, EXEMPT): mi355lz4_generate_device, mi355lz4_interleave_device,
mi355lz4_decompress_linked_begin / _end.

Known blind spot: a process has a few hardware queues (four by default), so two streams may share one and be ordered by accident.
That can only hide a bug; it never raises a false alarm.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import stream_order as SO  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def h(record):
    import torch
    hh = SO.Harness(torch, record)
    yield hh
    hh.close()


@pytest.fixture(autouse=True)
def stop_after_a_device_error(h):
    """a device that reports an error after a test ends the whole pytest session: nothing further runs on it"""
    yield
    try:
        h.torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        pytest.exit("the device reports an error after a stream-order test: %s" % e, returncode=3)


# ---- the harness can fail --------------------------------------------------------------------------------------------------------
def copy_case(name, stream_of):
    """a stand-in call, no library code: out = a device-to-device copy of the input, issued on stream_of() (None: the current one)"""
    import torch
    n = 1 << 20
    inputs = {v: {"x": np.random.RandomState(SO.SEED[v]).randint(0, 256, size=n).astype(np.uint8)} for v in SO.VARIANTS}

    def call(ctx, i, o):
        st = stream_of()
        if st is None:
            o["y"].copy_(i["x"], non_blocking=True)
        else:
            with torch.cuda.stream(st):
                o["y"].copy_(i["x"], non_blocking=True)

    return SO.Built(name, [], inputs, {"y": (n, np.uint8)}, call, lambda o: {"y": o["y"].copy()})


def test_harness_sees_a_misordered_copy(h):
    good = h.slot(copy_case("copy on the stream", lambda: None))
    h.reference([good])
    for warm in (False, True):
        kept = h.late([good], no_wait=(0,) if warm else ())
        h.judge(good, kept[0])
    # the same copy on a second non-blocking stream runs while the delay still holds the first: it reads the decoy.  (Two streams
    # may share a hardware queue and be ordered by accident, so up to four second streams are tried; one must show it.)
    seen = []
    for _ in range(4):
        other = h.new_stream()
        bad = h.slot(copy_case("copy on another stream", lambda: other))
        h.reference([bad])
        canon, raw = h.late([bad])[0]
        msg = SO.verdict(bad.b.name, canon, bad.ref["real"], bad.ref["decoy"], raw)
        seen.append(msg)
        h.torch.cuda.synchronize()
        if msg is not None:
            break
    assert seen[-1] is not None, "a copy issued on another stream passed the late-input check on four streams"
    assert "equals the decoy's output" in seen[-1] and "y differs" in seen[-1], seen[-1]


# ---- one late-input case per device call and mode -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SO.CASE_NAMES)
def test_late_input(h, name):
    h.run_case(SO.build(name))


# ---- cross-call protocols ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fstreams", "cstreams", "dstreams"])
def test_stream_table_ring(h, kind):
    """nine calls with nine stream tables behind one delay: every call sees its own table (StreamTableRing: four pinned entries,
    an event each).  The first four do not wait; the fifth may, by design."""
    slots = [h.slot(b) for b in SO.ring_cases(kind)]
    h.reference(slots)
    for warm in (False, True):
        kept = h.late(slots, no_wait=(0, 1, 2, 3) if warm else (), what="ring/" + kind)
        for s, k in zip(slots, kept):
            h.judge(s, k)


@pytest.mark.parametrize("kind", ["fstreams", "cstreams", "dstreams"])
def test_slots_continue_across_queued_calls(h, kind):
    """a stream cut into three calls behind one delay, without a wait: the bytes of the one-call result"""
    whole, parts = SO.cut_cases(kind)
    w = h.slot(whole)
    h.reference([w])
    ps = [h.slot(p) for p in parts]
    h.reference(ps)
    per, streams = 2, 3
    keys = ("result", "out") if kind == "dstreams" else ("framedLen", "slots")
    for warm in (False, True):
        kept = h.late(ps, no_wait=(0, 1, 2) if warm else (), what="cut/" + kind)
        for p, (s, k) in enumerate(zip(ps, kept)):
            h.judge(s, k)
            canon = k[0]
            for st in range(streams):
                for j in range(per):
                    at, of = st * per + j, st * per * len(parts) + p * per + j
                    for key in keys:
                        assert canon[key][at] == w.ref["real"][key][of], \
                            "%s: call %d, stream %d, block %d: %s is not the one-call result's" % (kind, p, st, j, key)


@pytest.mark.parametrize("kind", ["segments", "hcdict", "checksum", "exact"])
def test_scratch_grows_behind_a_queued_call(h, kind):
    """a small call, then one that needs a larger scratch, both behind one delay on an engine whose scratch has not grown yet
    (dev_reserve frees the old buffer while the small call is still queued)"""
    slots = [h.slot(b) for b in SO.growth_cases(kind)]
    h.reference(slots)
    ctx = h.new_engine()
    kept = h.late(slots, ctx=ctx, what="growth/" + kind)
    for s, k in zip(slots, kept):
        h.judge(s, k)


@pytest.mark.parametrize("kind", ["segments", "hcdict"])
def test_per_stream_scratch_changes_hands(h, kind):
    """five live streams in turn, each behind its own delay with its own inputs: the engine keeps a scratch for four, the fifth
    takes over the one used longest ago; then the first stream goes again, behind a delay of its own (the take-over has
    synchronised that stream, so without one its input would be on time).  Two rounds: in the first, on the fresh engine, a
    scratch's first use allocates, and the dictionary staging synchronises its stream before it grows, so those calls launch
    with their input in place -- that round checks the results; only the second round is late for every call."""
    slots = [h.slot(b) for b in SO.scratch_cases(kind)]
    for s in slots:
        h.reference([s])
    ctx = h.new_engine()
    streams = [h.new_stream() for _ in range(5)]
    plan = [(s, streams[k % 5]) for k, s in enumerate(slots)]
    for _ in range(2):
        kept = h.late_streams(plan, ctx=ctx, what="scratch/" + kind)
        for s, k in zip(slots, kept):
            h.judge(s, k)


def test_checksum_verdicts_across_streams(h):
    """checksummed decodes for two streams in turn share the engine's verdict buffer (ckBuf, ckEvent): each call reports its own
    MI355LZ4_BLK_E_CHECKSUM position"""
    cases = SO.checksum_verdict_cases()
    slots = [h.slot(b) for b in cases]
    for s in slots:
        h.reference([s])
    a, b = h.new_stream(), h.new_stream()
    plan = [(s, (a, b)[k % 2]) for k, s in enumerate(slots)]
    for _ in range(2):
        kept = h.late_streams(plan, what="verdicts")
        for s, (canon, raw) in zip(slots, kept):
            h.judge(s, (canon, raw))
            bad = [i for i, r in enumerate(canon["result"]) if r == SO.BLK_E_CHECKSUM]
            assert bad == [s.b.bad["real"]], (s.b.name, bad)
            assert all(r >= 0 for i, r in enumerate(canon["result"]) if i != s.b.bad["real"]), s.b.name


def test_two_engines(h):
    """one engine on its stream behind a delay, another on torch's default stream meanwhile: each gets its own result"""
    torch = h.torch
    a, b = h.slot(SO.build("compress_batch_device/level0")), h.slot(SO.build("decompress_batch_device/decoder0"))
    other = h.new_engine()
    h.reference([a])
    h.reference([b], ctx=other)
    a.load("decoy")
    a.fill()
    b.load("real")
    b.fill()
    SO.configure(h.eng, a.b.cfg)
    SO.configure(other.eng, b.b.cfg)
    torch.cuda.synchronize()
    ms = h.delay_ms([a, b])
    gate = torch.cuda.Event()
    with torch.cuda.stream(h.s):
        h.delay(ms)
        gate.record()
        a.enqueue(h.ctx)
    b.b.call(other, b.inp, b.out)                       # the default stream: not ordered with h.s, which is non-blocking
    torch.cuda.default_stream().synchronize()
    got_b = b.fetch(b.out)
    meanwhile = not gate.query()
    h.s.synchronize()
    h.record(what="two engines", delay_ms=ms, second_engine_done_before_the_gate=meanwhile)
    h.judge(a, h.kept_of(a))
    msg = SO.verdict(b.b.name + " (second engine)", b.b.canon(got_b), b.ref["real"], b.ref["decoy"], got_b)
    assert msg is None, msg


# ---- host-buffer forms with the engine's stream a non-blocking one -------------------------------------------------------------------
def test_host_buffer_forms_on_a_stream(h):
    """The host-buffer calls are synchronous and use the engine's stream as one of their own; the suite only ever runs them with
    the null stream in that role.  One round trip of each with the engine on torch.cuda.Stream(): the results of the default
    stream, and the oracle's where it applies."""
    torch, S, eng, O = h.torch, SO.S(), h.eng, SO.orc()
    SO.configure(eng, {})
    torch.cuda.synchronize()
    _u8p = C.POINTER(C.c_uint8)
    blocks = SO.blocks_of(SO.ragged(12, 65536, 31), "real", salt=7000)
    raw = b"".join(blocks)
    dic = SO.dict_input("real", 70)
    dic_dev = torch.from_numpy(np.frombuffer(dic, dtype=np.uint8).copy()).to("cuda:0")
    stream_blocks = [SO.blocks_of(ln, "real", salt=7100 + s, kinds=SO.LINKED_KINDS) for s, ln in enumerate(([4096, 65536, 13], [70000, 5], [1, 20000, 30000]))]
    flat = [b for st in stream_blocks for b in st]
    sf = np.cumsum([0] + [len(st) for st in stream_blocks]).tolist()
    linked = b"".join(SO.M.frame(c, len(b), 8) for st in stream_blocks for c, b in zip(SO.M.linked_stream(O, st, ragged=True), st))
    pinned_in = [torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).pin_memory() for b in blocks]
    ctx = h.ctx

    def pinned_decompress(framed):
        src = torch.from_numpy(np.frombuffer(framed, dtype=np.uint8).copy()).pin_memory()
        out = torch.empty(len(raw) + 16, dtype=torch.uint8).pin_memory()
        blen = np.zeros(len(blocks), dtype=np.int32)
        out_len, got = C.c_size_t(), C.c_int()
        rc = S.lib.mi355lz4_decompress_batch(eng.ctx, C.cast(src.data_ptr(), _u8p), src.numel(), 8, 0, 0, None, 0,
                                             C.cast(out.data_ptr(), _u8p), out.numel(), C.byref(out_len),
                                             blen.ctypes.data_as(C.POINTER(C.c_int32)), len(blocks), C.byref(got))
        assert rc == 0, rc
        return out.numpy()[:out_len.value].tobytes(), blen[:got.value].tolist()

    def forms():
        r = {}
        r["compress_batch"] = eng.compress_batch(blocks)
        r["decompress_batch"] = eng.decompress_batch(r["compress_batch"][0])
        r["compress_batch pinned"] = eng.compress_batch([t.numpy() for t in pinned_in])
        r["decompress_batch pinned"] = pinned_decompress(r["compress_batch"][0])
        r["decompress_streams"] = eng.decompress_streams(linked, sf)
        ctx.cs.load_dict(14, dic_dev)
        r["compress_dict"] = eng.compress_dict(blocks, ctx.cs, dict_slot=14)
        r["decompress_dict"] = eng.decompress_dict(r["compress_dict"][0], dic)
        r["compress_pages_fast"] = eng.compress_pages_fast(blocks[:4], 1024, 6)
        ctx.fs.reset()
        r["compress_streams_fast"] = eng.compress_streams_fast(stream_blocks, ctx.fs, slots=[3, 8, 1])
        ctx.ds.reset()
        r["decompress_dstreams"] = eng.decompress_dstreams(r["compress_streams_fast"][0], sf, ctx.ds, slots=[3, 8, 1])
        return r

    want = forms()                                       # the engine follows torch's current stream: the default one
    torch.cuda.synchronize()
    with torch.cuda.stream(h.s):
        eng._follow_torch()                              # (the host-buffer forms take the engine's stream as it is)
        assert eng._cur_stream == h.s.cuda_stream
        got = forms()
    h.s.synchronize()
    with torch.cuda.stream(torch.cuda.default_stream()):
        eng._follow_torch()
    for key in want:
        assert got[key] == want[key], key + ": differs from the default stream's result"
    lens = [len(b) for b in blocks]
    for key in ("decompress_batch", "decompress_batch pinned", "decompress_dict"):
        assert got[key] == (raw, lens), key
    assert got["compress_batch pinned"] == got["compress_batch"]
    assert O.frame_decompress(got["compress_batch"][0], len(raw), 8, 0, False) == raw
    assert got["decompress_streams"] == (b"".join(flat), [len(b) for b in flat])
    assert got["decompress_dstreams"] == (b"".join(flat), [len(b) for b in flat])
    loaded = SO.dict_model.model_load(dic)
    model = b"".join(SO.dict_model.framed_block(*SO.dict_model.model_compress(loaded, b, 1), len(b), 8) for b in blocks)
    assert got["compress_dict"][0] == model, "compress_dict: not the reference's bytes"
    for (pages, consumed), data in zip(got["compress_pages_fast"], blocks[:4]):
        pos = 0
        for page, used in pages:
            assert O.decompress_block(page[8:], used) == (used, data[pos:pos + used])
            pos += used
        assert pos == consumed
