"""The legacy face (include/lz4.h, csrc/legacy.cpp) call by call against the reference's recorded results
(tests/golden/legacy_sessions.json, sessions of tests/legacy_cases.py): return codes exactly, negative ones included, and bytes.
The decoder behind it has a launch shape of its own (one block, two device buffers that swap and regrow, the other buffer as
dictionary), so everything goes through slz4.lib.LZ4_* as bound in streamly_lz4_amd.  Every destination is a numpy buffer with 64
guard bytes of a position-dependent pattern behind dstCapacity; a decode that returns r > 0 leaves dst[r:] as it was."""
import ctypes as C
import threading

import numpy as np
import pytest

import guarded as G
import legacy_cases as LC
from test_parity_gpu import split_blocks

pytestmark = pytest.mark.gpu

GUARD = 64
_u8p = C.POINTER(C.c_uint8)


def _ptr(a):
    return a.ctypes.data_as(_u8p)


def _src(data):
    return np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)


class Decoder:
    """one LZ4_streamDecode_t; step() is one LZ4_decompress_safe_continue into a guarded buffer of its own"""

    def __init__(self, L):
        self.L, self.ctx, self.calls = L, L.LZ4_createStreamDecode(), 0
        assert self.ctx

    def step(self, block, cap, what=""):
        src = _src(block)
        dst = G.new_numpy(max(cap, 0) + GUARD, seed=self.calls + 1)
        before = dst.copy()
        self.calls += 1
        r = self.L.LZ4_decompress_safe_continue(self.ctx, _ptr(src), _ptr(dst), len(block), cap)
        assert r <= max(cap, 0), (what, r, cap)
        keep = r if r > 0 else max(cap, 0)              # the guard always; behind the r bytes of a decoded block too
        assert np.array_equal(dst[keep:], before[keep:]), "%s: bytes behind %d changed (capacity %d, returned %d)" % (what, keep, cap, r)
        return r, dst[:max(r, 0)].tobytes()

    def close(self):
        self.L.LZ4_freeStreamDecode(self.ctx)


class Compressor:
    """one LZ4_stream_t; step() is one LZ4_compress_fast_continue into a guarded buffer of its own"""

    def __init__(self, L):
        self.L, self.ctx, self.calls = L, L.LZ4_createStream(), 0
        assert self.ctx

    def step(self, data, cap, accel=1, src_size=None, what=""):
        src = _src(data)
        dst = G.new_numpy(max(cap, 0) + GUARD, seed=self.calls + 50)
        before = dst.copy()
        self.calls += 1
        r = self.L.LZ4_compress_fast_continue(self.ctx, _ptr(src), _ptr(dst), len(data) if src_size is None else src_size, cap, accel)
        assert 0 <= r <= max(cap, 0), (what, r, cap)
        assert np.array_equal(dst[max(cap, 0):], before[max(cap, 0):]), "%s: guard behind capacity %d changed (returned %d)" % (what, cap, r)
        return r, dst[:r].tobytes()

    def close(self):
        self.L.LZ4_freeStream(self.ctx)


@pytest.fixture(scope="module")
def gold():
    return LC.load_golden()


@pytest.fixture(scope="module")
def sessions():
    return LC.decode_sessions()


def _run_decode(L, name, steps):
    d = Decoder(L)
    try:
        return [d.step(blk, cap, "%s, step %d (%s)" % (name, k, step)) for k, (step, blk, cap) in enumerate(steps)]
    finally:
        d.close()


def _check_decode(name, steps, rec, results):
    got = LC.record(results)
    assert len(rec["codes"]) == len(steps) == len(results), name
    bad = ["%s, step %d (%s, capacity %d): returned %d, the reference %d%s"
           % (name, k, step, cap, got["codes"][k], rec["codes"][k], "" if got["codes"][k] != rec["codes"][k] else ", bytes differ")
           for k, (step, _, cap) in enumerate(steps) if (got["codes"][k], got["sha256"][k]) != (rec["codes"][k], rec["sha256"][k])]
    assert not bad, "%d of %d steps differ: %s" % (len(bad), len(steps), "; ".join(bad[:8]))


# ---- decode -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", ["D1", "D2", "D3", "D4", "D5", "D6"])
def test_decode_sessions(slz4, gold, sessions, group):
    """D1 first-call branch, D2 the same blocks behind a dictionary of 70 000 and of 100 bytes, D3 dictionary streams, D4 the
    context after results <= 0, D5 outputs swinging between 5 bytes and 1 MiB, D6 capacities down to 0 and srcSize 0"""
    recs = gold["decode"][group]
    assert [name for name, _ in sessions[group]] == [r["session"] for r in recs]
    for (name, steps), rec in zip(sessions[group], recs):
        _check_decode(name, steps, rec, _run_decode(slz4.lib, name, steps))


def _decode_stream(L, blocks_caps, what):
    d = Decoder(L)
    try:
        out, codes = [], []
        for k, (blk, cap) in enumerate(blocks_caps):
            r, dec = d.step(blk, cap, "%s, block %d" % (what, k))
            codes.append(r)
            out.append(dec)
        return codes, b"".join(out)
    finally:
        d.close()


@pytest.mark.parametrize("kind,block_len,n_blocks", [("text", 1000, 300), ("lzsynth", 1000, 300), ("text", 65536, 32),
                                                     ("lzsynth", 65536, 32), ("text", 262144, 8), ("lzsynth", 262144, 8)])
def test_streams_written_by_the_reference_compressor(slz4, oracle, kind, block_len, n_blocks):
    """linked streams as the reference's compressor writes them (oracle.frame_compress is its byte-pinned restatement), block by
    block through one context"""
    data = oracle.gen(kind, n_blocks, block_len, first_block=77).tobytes()
    fr = oracle.frame_compress(data, block_len, 1, 8, True)
    blocks = [(b[8:], int.from_bytes(b[4:8], "little")) for b in split_blocks(fr)]
    assert len(blocks) == n_blocks
    if kind == "text":                                  # the stream really is linked (lzsynth's blocks share nothing with each other)
        assert sum(oracle.decompress_block(b, cap)[0] < 0 for b, cap in blocks[1:]) > len(blocks) // 2
    codes, out = _decode_stream(slz4.lib, blocks, "%s in blocks of %d" % (kind, block_len))
    assert codes == [cap for _, cap in blocks]
    assert out == data


RAGGED = [65536, 1000, 65536, 0, 13, 12, 40000, 65536, 65536, 5, 65536, 30000]    # test_engine_written_linked_stream_all_linked_paths'


def test_stream_written_by_the_engines_linked_compressor(slz4, engine, oracle):
    """the engine's linked compressor reaches deeper into the predecessor than the reference's; ragged blocks, among them one of
    0 bytes (decoded into a capacity of 0), 12 and 13 bytes"""
    data = oracle.gen("text", 9, 65536, first_block=6).tobytes()
    blocks, pos = [], 0
    for sz in RAGGED:
        blocks.append(data[pos:pos + sz])
        pos += sz
    engine.set_linked_compress(True)
    try:
        fr, _ = engine.compress_batch(blocks)
    finally:
        engine.set_linked_compress(False)
    comp = [(b[8:], int.from_bytes(b[4:8], "little")) for b in split_blocks(fr)]
    assert [cap for _, cap in comp] == RAGGED
    codes, out = _decode_stream(slz4.lib, comp, "engine-written linked stream")
    assert codes == RAGGED
    assert out == data[:pos]


def test_two_contexts_alternately(slz4, gold, sessions):
    """D3's first two streams through contexts A and B, calls interleaved: each comes out as in its own session"""
    (na, sa), (nb, sb) = sessions["D3"][:2]
    A, B = Decoder(slz4.lib), Decoder(slz4.lib)
    ra, rb = [], []
    try:
        for k in range(max(len(sa), len(sb))):
            if k < len(sa):
                ra.append(A.step(sa[k][1], sa[k][2], "A step %d" % k))
            if k < len(sb):
                rb.append(B.step(sb[k][1], sb[k][2], "B step %d" % k))
    finally:
        A.close()
        B.close()
    _check_decode(na + " (context A)", sa, gold["decode"]["D3"][0], ra)
    _check_decode(nb + " (context B)", sb, gold["decode"]["D3"][1], rb)


# ---- compress -----------------------------------------------------------------------------------------------------------------

def test_compress_forced_outcomes(slz4, oracle, gold):
    """C1: what the reference is forced to return, the legacy face returns -- 1 and a zero byte for an empty input, 0 without room,
    0 for incompressible input in a buffer of its own size, 0 for a negative size and for one past LZ4_MAX_INPUT_SIZE (refused
    before src is read: the size is only named); more than 0 at LZ4_compressBound"""
    cases = LC.c1_sessions(oracle)
    assert [name for name, _, _ in cases] == [r["session"] for r in gold["compress"]["C1"]]
    for (name, steps, forced), rec in zip(cases, gold["compress"]["C1"]):
        c = Compressor(slz4.lib)
        try:
            res = [c.step(data, cap, accel, src_size=n, what="%s, %s" % (name, step)) for step, data, n, cap, accel in steps]
        finally:
            c.close()
        if forced:
            got = LC.record(res)
            assert (got["codes"], got["sha256"]) == (rec["codes"], rec["sha256"]), (name, got["codes"], rec["codes"])
        else:
            for (step, data, n, cap, _), (r, comp), pos in zip(steps, res, rec["positive"]):
                assert pos and 0 < r <= cap, (name, step, r)
                assert oracle.decompress_block(comp, n) == (n, data), (name, step)


@pytest.mark.parametrize("kind", LC.C2_KINDS)
def test_compress_lengths_and_accelerations(slz4, oracle, kind):
    """C2: lengths around the match rules' 12 / 13 and around 64 KiB, up to 1 MiB; accelerations far outside [1, 65537] on both
    sides.  At LZ4_compressBound the result is within the bound, decodes WITHOUT a dictionary to the input (blocks are emitted
    independent although the context is one), and a second call writes the same bytes."""
    c = Compressor(slz4.lib)
    try:
        for n in LC.C2_LENGTHS:
            data = LC.gen_input(oracle, kind, n, seed=n % 251)
            bound = slz4.lib.LZ4_compressBound(n)
            assert bound == LC.bound(n)
            for accel in LC.C2_ACCELS:
                what = "%s, %d bytes, acceleration %d" % (kind, n, accel)
                r, comp = c.step(data, bound, accel, what=what)
                assert 0 < r <= bound, (what, r)
                assert oracle.decompress_block(comp, n) == (n, data), what
                r2, comp2 = c.step(data, bound, accel, what=what + " (again)")
                assert (r2, comp2) == (r, comp), what
    finally:
        c.close()


def test_compressed_blocks_are_independent(slz4, oracle):
    """the same block twice in a row, then a block that starts with its predecessor's last 3000 bytes: a linked compressor would
    reach back for them; every block here decodes without a dictionary (include/lz4.h)"""
    a = LC.gen_input(oracle, "text", 40000, seed=3)
    b = a[-3000:] + LC.gen_input(oracle, "text", 20000, seed=4)
    c = Compressor(slz4.lib)
    try:
        for k, data in enumerate((a, a, b)):
            r, comp = c.step(data, LC.bound(len(data)), 1, what="block %d" % k)
            assert r > 0 and oracle.decompress_block(comp, len(data)) == (len(data), data), k
    finally:
        c.close()


@pytest.mark.parametrize("kind", ["text", "random"])
def test_compress_limited_output(slz4, oracle, kind):
    """C3: one byte less than the block needs returns 0; exactly enough and one more return the block"""
    data = LC.gen_input(oracle, kind, 20000, seed=9)
    c = Compressor(slz4.lib)
    try:
        n, comp = c.step(data, LC.bound(len(data)), 1, what="at bound")
        assert n > 0 and oracle.decompress_block(comp, len(data)) == (len(data), data)
        assert c.step(data, n - 1, 1, what="capacity c - 1") == (0, b"")
        assert c.step(data, n, 1, what="capacity c") == (n, comp)
        assert c.step(data, n + 1, 1, what="capacity c + 1") == (n, comp)
    finally:
        c.close()


def test_compress_source_sizes_swing(slz4, oracle):
    """C4: sources of 100 bytes, 300 000, 5, 1 MiB, 64 through one context: its device and page-locked buffers regrow"""
    c = Compressor(slz4.lib)
    try:
        for k, n in enumerate(LC.SRC_SWING):
            data = LC.gen_input(oracle, "text", n, seed=20 + k)
            r, comp = c.step(data, LC.bound(n), 1, what="%d bytes" % n)
            assert r > 0 and oracle.decompress_block(comp, n) == (n, data), n
    finally:
        c.close()


# ---- several threads over the one engine ----------------------------------------------------------------------------------------

def _thread_work(L, d5, inputs):
    dec = _run_decode(L, d5[0], d5[1])
    c = Compressor(L)
    try:
        comp = [c.step(data, LC.bound(len(data)), accel, what="threads: %d bytes, acceleration %d" % (len(data), accel))
                for data, accel in inputs]
    finally:
        c.close()
    return dec, comp


def test_four_threads(slz4, oracle, gold, sessions):
    """four threads, each with a decode and a compress context of its own, run D5 and a part of C2 at once (ctypes releases the
    GIL: the calls contend for the engine's mutex): every thread gets what one thread alone gets"""
    L = slz4.lib
    d5 = sessions["D5"][0]
    inputs = [(LC.gen_input(oracle, kind, n, seed=n % 251), accel) for kind in ("text", "random") for n in (13, 65537, 1048576)
              for accel in (1, 9)]
    alone = _thread_work(L, d5, inputs)
    _check_decode(d5[0], d5[1], gold["decode"]["D5"][0], alone[0])
    results, errors = [None] * 4, []

    def run(i):
        try:
            results[i] = _thread_work(L, d5, inputs)
        except BaseException as e:                       # (an assertion of a guard, say: reported by the test, not lost with the thread)
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=run, args=(i,), daemon=True) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a thread is still running after 120 s"
    assert not errors, errors
    for i in range(4):
        assert results[i] == alone, "thread %d differs from the single-threaded run" % i
