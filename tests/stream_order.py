"""Stream-order harness and cases for tests/test_stream_order_gpu.py and tests/test_stream_order_host.py (test infrastructure
only; not a conftest).

include/mi355lz4.h: every *_device call only ENQUEUES on the engine's stream, which in the product is a non-blocking stream.  The
rest of the suite runs on the legacy null stream, where a kernel, memset or copy issued to the wrong stream, a scratch buffer
reused too early and a missing event wait are all still ordered.  Here every call runs on a non-blocking stream with LATE input:

  a case is a pair of inputs, `real` and `decoy`: both valid, the same shapes (block count, offsets, capacities, strides, buffer
  sizes, dictionary lengths, stream tables), different bytes.  The inputs hold `decoy` and the outputs a fill pattern; then, on
  the stream and with no synchronisation in between: a delay, an event `gate`, device-to-device copies of `real` over the
  inputs, the call, copies of every output into `kept`, copies of `decoy` back over the inputs.  `kept` must equal what the
  same call gave for `real` on the default stream, byte for byte.  A call that read too early gives the decoy's outputs, one
  that wrote too late leaves the fill pattern; a misordered call reads valid data and gives a wrong answer, never garbage.

  "only enqueues" is the condition gate.query() == False right after the call returns: the delay has not ended, so the call
  did not wait for its stream.

The data is the oracle generator's kinds ("text", "lzsynth") and the dictionary tests' word text, each at two seeds.

Known blind spot: a process has a few hardware queues (four here by default), so two streams may share one and be ordered by
accident.  That can only hide a bug; it never raises a false alarm.
"""
import collections
import ctypes as C
import os
import re
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dict_cases  # noqa: E402
import dict_model  # noqa: E402
import dstreams_model as M  # noqa: E402
import lz4_check  # noqa: E402
import pages_model  # noqa: E402

FILL = 0xA5
BLK_E_CHECKSUM = -0x7F000004
SEED = {"real": 11, "decoy": 47}
VARIANTS = ("real", "decoy")
_u8p = C.POINTER(C.c_uint8)

# the engine switches a case may set; every run starts from these
DEFAULT_CFG = dict(level=0, checksum=False, linked=False, exact=False, segments=-1, decoder=0, linked_async=0)

# device calls of the header that have no late-input case, and why
EXEMPT = {
    "mi355lz4_generate_device": "reads no device memory: its inputs are scalars, so there is nothing to bring late",
    "mi355lz4_interleave_device": "multi-GPU gather support, driven over torch.distributed (tests/test_distributed.py)",
    "mi355lz4_decompress_linked_begin": "one linked decode in two halves over several engines; the halves wait on the host",
    "mi355lz4_decompress_linked_end": "see mi355lz4_decompress_linked_begin",
}


def S():
    import streamly_lz4_amd
    return streamly_lz4_amd


_ORC = None


def orc():
    global _ORC
    if _ORC is None:
        from oracle.oracle import Oracle
        _ORC = Oracle()
    return _ORC


def xxh32(b, seed=0):
    a = np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(1, dtype=np.uint8)
    return int(S().lib.slz4_xxh32(a.ctypes.data_as(_u8p), len(b), int(seed))) & 0xFFFFFFFF


# ---- data ---------------------------------------------------------------------------------------------------------------------
_GEN = {}


def gen(kind, n, seed):
    key = (kind, n, seed)
    if key not in _GEN:
        _GEN[key] = dict_cases.text(seed, n) if kind == "words" else orc().gen(kind, 1, n, first_block=seed).tobytes()
    return _GEN[key]


def blocks_of(lens, var, salt=0, kinds=("text", "lzsynth")):
    """block i: lens[i] bytes of kinds[i % len(kinds)] at the variant's seed"""
    total = sum(lens) + 16
    bufs = [gen(k, total, SEED[var] + salt) for k in kinds]
    out, p = [], 0
    for i, n in enumerate(lens):
        out.append(bufs[i % len(kinds)][p:p + n])
        p += n
    return out


def ragged(n, top, seed, edges=True):
    lens = np.random.RandomState(seed).randint(1, top + 1, size=n).tolist()
    if edges:
        lens[:6] = [1, 12, 13, 4095, top, top - 1][:n]
    return lens


def ragged_pair(n, top):
    """two length lists that differ at every block (decode cases: the results then differ too)"""
    a, b = ragged(n, top, 1, edges=False), ragged(n, top, 2, edges=False)
    b = [y if y != x else (y % top) + 1 for x, y in zip(a, b)]
    return {"real": a, "decoy": b}


def arr(v, dtype):
    return np.ascontiguousarray(np.asarray(v, dtype=dtype))


# ---- a built case -------------------------------------------------------------------------------------------------------------
class Built:
    """name; symbols: the C calls it runs; waits: the header lets the call wait on the host (no no-wait assertion); cfg: engine
    switches; inputs[variant][name] = numpy array; outs[name] = (elements, numpy dtype); call(ctx, inp, out): the GPU call on
    device tensors; canon(outs as numpy) -> {array name: numpy array or list per block}: what the verdict compares;
    model(variant) -> the same from a CPU model, or None; valid(variant): raises when an input is not valid; check(variant,
    canon): holds an engine's own parse to lz4_check and the oracle's decode."""

    def __init__(self, name, symbols, inputs, outs, call, canon, waits=False, cfg=None, model=None, valid=None, check=None):
        self.name, self.symbols, self.inputs, self.outs, self.call, self.canon = name, tuple(symbols), inputs, outs, call, canon
        self.waits, self.cfg, self.model, self.valid, self.check = waits, dict(cfg or {}), model, valid, check


def place(blocks_by_var, gap, lead=3):
    """one layout for both variants (their lengths may differ): offsets by the longer block, `gap` bytes apart; the buffers"""
    n = len(blocks_by_var["real"])
    off, pos = [], lead
    for i in range(n):
        off.append(pos)
        pos += max(len(blocks_by_var[v][i]) for v in VARIANTS) + gap
    bufs = {}
    for v in VARIANTS:
        buf = np.full(pos + 64, 0xEE, dtype=np.uint8)
        for o, b in zip(off, blocks_by_var[v]):
            buf[o:o + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
        bufs[v] = buf
    return off, bufs


def clip(v, hi):
    return max(0, min(int(v), int(hi)))


# ---- compress calls: src, srcOff, srcLen -> slots, framedLen --------------------------------------------------------------------
def compress_built(name, symbols, blocks, call, max_len, cfg=None, kind=8, gap=7, extra=None, dict_for=None, model=None,
                   waits=False):
    """blocks[variant] = the blocks (equal lengths in both variants); call(ctx, inp, out, L) with L the layout (n, max_len, kind,
    stride); extra[variant] = further inputs (dictionary bytes, dictIdx); dict_for(variant, i) = block i's dictionary for the
    check of an engine's own parse (None: the byte model is the check); model(variant) = [framed bytes per block]."""
    checksum = bool((cfg or {}).get("checksum"))
    n = len(blocks["real"])
    assert [len(b) for b in blocks["real"]] == [len(b) for b in blocks["decoy"]]
    off, bufs = place(blocks, gap)
    stride = int(S().slot_stride_ex(max_len, kind, checksum))
    L = collections.namedtuple("L", "n max_len kind stride")(n, max_len, kind, stride)
    inputs = {}
    for v in VARIANTS:
        inputs[v] = {"src": bufs[v], "srcOff": arr(off + [0], np.int64), "srcLen": arr([len(b) for b in blocks[v]] + [0], np.int32)}
        if extra:
            inputs[v].update(extra[v])
    outs = {"slots": (n * stride, np.uint8), "framedLen": (n, np.int32)}

    def canon(o):
        fl = o["framedLen"]
        return {"framedLen": fl.copy(),
                "slots": [o["slots"][i * stride:i * stride + clip(fl[i], stride)].tobytes() for i in range(n)]}

    def want(v):
        if model is None:
            return None
        frames = model(v)
        return {"framedLen": arr([len(f) for f in frames], np.int32), "slots": list(frames)}

    def check(v, c):
        if dict_for is None:
            return
        for i, (frame, data) in enumerate(zip(c["slots"], blocks[v])):
            what = "%s/%s block %d" % (name, v, i)
            assert len(frame) == c["framedLen"][i] and len(frame) > kind, what
            comp_len = int.from_bytes(frame[:4], "little")
            assert len(frame) == kind + comp_len + (4 if checksum else 0), what
            if kind == 8:
                assert int.from_bytes(frame[4:8], "little") == len(data), what
            payload = frame[kind:kind + comp_len]
            if checksum:
                assert int.from_bytes(frame[kind + comp_len:], "little") == xxh32(payload), what + ": trailer"
            d = dict_for(v, i) or b""
            lz4_check.check_block(payload, len(data), len(d[-65536:]))
            r, got = orc().decompress_block(payload, len(data), dict_bytes=d[-65536:] or None)
            assert r == len(data) and got == data, what + ": the oracle does not decode it to the input"

    def valid(v):
        assert all(0 <= len(b) <= max_len for b in blocks[v])

    return Built(name, symbols, inputs, outs, lambda ctx, i, o: call(ctx, i, o, L), canon, waits=waits, cfg=cfg,
                 model=want if model else None, valid=valid, check=check)


def enc_kw(i, L):
    return dict(header_kind=L.kind, src_off=i["srcOff"], src_len=i["srcLen"], block_stride=0)


def frame_of(comp, n, kind, checksum=False):
    return M.frame(comp, n, kind, checksum)


def b_compress_batch(mode):
    sym = ["mi355lz4_compress_batch_device"]
    name = "compress_batch_device/" + mode
    cfg, gap, model, waits = {}, 7, None, False
    lens, max_len = ragged(6 if mode == "exact" else 48, 65536, 5), 65536        # (exact: one serial chain per call; 48 blocks would need a delay above one second)
    dict_for = lambda v, i: None  # noqa: E731
    if mode == "big":
        lens, max_len = [262144] * 6 + [262143, 100000], 262144
    elif mode == "segments4":
        lens, cfg = [65536] * 8, {"segments": 4}
    elif mode == "linked":
        cfg, gap = {"linked": True}, 0
    elif mode in ("level3", "level9"):
        cfg = {"level": int(mode[5:])}
    elif mode == "checksum":
        cfg = {"checksum": True}
    elif mode == "exact":
        cfg, waits, dict_for = {"exact": True}, True, None
    blocks = {v: blocks_of(lens, v, kinds=LINKED_KINDS if mode in ("linked", "exact") else ("text", "lzsynth")) for v in VARIANTS}
    if mode == "linked":
        dict_for = lambda v, i: blocks[v][i - 1] if i else None  # noqa: E731
    if mode == "exact":
        model = lambda v: [frame_of(c, len(b), 8) for c, b in zip(M.linked_stream(orc(), blocks[v], ragged=True), blocks[v])]  # noqa: E731

    def call(ctx, i, o, L):
        if mode == "exact":
            ctx.eng.reset_compress_stream()
        ctx.eng.compress_batch_device(i["src"], L.n, L.max_len, o["slots"], L.stride, o["framedLen"], accel=1, **enc_kw(i, L))

    return compress_built(name, sym, blocks, call, max_len, cfg=cfg, gap=gap, dict_for=dict_for, model=model, waits=waits)


def streams_table(streams):
    return np.cumsum([0] + [len(st) for st in streams]).astype(np.int32)


def b_compress_streams(name="compress_streams_device", streams=None, slots=(5, 0, 7), reset=True, held=None, max_len=None):
    """mi355lz4_compress_streams_device: streams[variant] = lists of blocks, stream s continuing slot slots[s] of the set; held[s]
    (model only) = an OracleStream-like list of the arrays the slot has seen before"""
    if streams is None:
        lens = [[4096, 65536, 13, 20000], [1, 70000, 4095], [30000, 30000, 5, 12, 65537]]
        streams = {v: [blocks_of(ln, v, salt=100 + s, kinds=LINKED_KINDS) for s, ln in enumerate(lens)] for v in VARIANTS}
    flat = {v: [b for st in streams[v] for b in st] for v in VARIANTS}
    sf, sl = streams_table(streams["real"]), list(slots)
    max_len = max_len or max(len(b) for b in flat["real"])

    def model(v):
        out = []
        for s, st in enumerate(streams[v]):
            before = list(held[v][s]) if held else []
            comps = M.linked_stream(orc(), before + list(st), ragged=True)[len(before):]
            out += [frame_of(c, len(b), 8) for c, b in zip(comps, st)]
        return out

    def call(ctx, i, o, L):
        if reset:
            ctx.cs.reset(sl)
        ctx.eng.compress_streams_device(ctx.cs, i["src"], L.n, L.max_len, sf, sl, o["slots"], L.stride, o["framedLen"], accel=1,
                                        **enc_kw(i, L))

    b = compress_built(name, ["mi355lz4_compress_streams_device", "mi355lz4_cstreams_reset"], flat, call, max_len, model=model)
    b.table = ([int(x) for x in sf], sl)
    return b


def b_compress_streams_fast(name="compress_streams_fast_device", streams=None, slots=(5, 0, 7), reset=True, with_dict=True,
                            checked=True, max_len=None):
    """mi355lz4_compress_streams_fast_device behind fstreams_reset and fstreams_set_dict (stream 0's slot, dictionary late)"""
    if streams is None:
        lens = [[4096, 65536, 13, 20000], [1, 65536, 4095], [30000, 30000, 5, 12, 60000]]
        streams = {v: [blocks_of(ln, v, salt=200 + s, kinds=LINKED_KINDS) for s, ln in enumerate(lens)] for v in VARIANTS}
    flat = {v: [b for st in streams[v] for b in st] for v in VARIANTS}
    sf, sl = streams_table(streams["real"]), list(slots)
    max_len = max_len or max(len(b) for b in flat["real"])
    dicts = {v: gen("text", 30000, SEED[v] + 250) for v in VARIANTS}
    extra = {v: {"dict": arr(np.frombuffer(dicts[v], dtype=np.uint8), np.uint8)} for v in VARIANTS} if with_dict else None
    prev = {}
    for v in VARIANTS:
        k = 0
        for s, st in enumerate(streams[v]):
            for j, _ in enumerate(st):
                prev[(v, k)] = st[j - 1] if j else (dicts[v] if with_dict and s == 0 else None)
                k += 1

    def call(ctx, i, o, L):
        if reset:
            ctx.fs.reset()
        if with_dict:
            ctx.fs.set_dict(sl[0], i["dict"])
        ctx.eng.compress_streams_fast_device(ctx.fs, i["src"], L.n, L.max_len, sf, sl, o["slots"], L.stride, o["framedLen"],
                                             accel=1, **enc_kw(i, L))

    b = compress_built(name, ["mi355lz4_compress_streams_fast_device", "mi355lz4_fstreams_reset", "mi355lz4_fstreams_set_dict"],
                       flat, call, max_len, extra=extra, dict_for=(lambda v, i: prev[(v, i)]) if checked else None)
    b.table = ([int(x) for x in sf], sl)
    return b


DICT_LEN = 20000
SET_DICT_LENS = (20000, 65536, 100)          # the members of the dictionary set


def set_dicts():
    return [gen("words", n, 7000 + k) for k, n in enumerate(SET_DICT_LENS)]


def word_blocks(lens, var, salt):
    return [gen("words", n, 100 * SEED[var] + salt + i) for i, n in enumerate(lens)]


def dict_input(var, salt=0):
    return gen("words", DICT_LEN, 9000 + SEED[var] + salt)


def b_compress_dict():
    """mi355lz4_compress_dict_device behind cstreams_load_dict, the dictionary bytes late; the reference's bytes (dict_model)"""
    lens = ragged(24, 65536, 7)
    blocks = {v: word_blocks(lens, v, 300) for v in VARIANTS}
    dicts = {v: dict_input(v) for v in VARIANTS}
    extra = {v: {"dict": arr(np.frombuffer(dicts[v], dtype=np.uint8), np.uint8)} for v in VARIANTS}

    def model(v):
        loaded = dict_model.model_load(dicts[v])
        return [dict_model.framed_block(*dict_model.model_compress(loaded, b, 1), len(b), 8) for b in blocks[v]]

    def call(ctx, i, o, L):
        ctx.cs.load_dict(15, i["dict"])
        ctx.eng.compress_dict_device(ctx.cs, 15, i["src"], L.n, L.max_len, o["slots"], L.stride, o["framedLen"], accel=1,
                                     **enc_kw(i, L))

    return compress_built("compress_dict_device", ["mi355lz4_compress_dict_device", "mi355lz4_cstreams_load_dict"], blocks, call,
                          65536, extra=extra, model=model)


def b_compress_hcdict(fast):
    """mi355lz4_compress_hcdict_device (level 3) / mi355lz4_compress_fastdict_device (level 0) behind hcdict_load, dictionary late"""
    lens = ragged(24, 65536, 8)
    blocks = {v: word_blocks(lens, v, 400 + fast) for v in VARIANTS}
    dicts = {v: dict_input(v, 1 + fast) for v in VARIANTS}
    extra = {v: {"dict": arr(np.frombuffer(dicts[v], dtype=np.uint8), np.uint8)} for v in VARIANTS}

    def call(ctx, i, o, L):
        ctx.hd.load(i["dict"])
        if fast:
            ctx.eng.compress_fastdict_device(ctx.hd, i["src"], L.n, L.max_len, o["slots"], L.stride, o["framedLen"], accel=1,
                                             **enc_kw(i, L))
        else:
            ctx.eng.compress_hcdict_device(ctx.hd, i["src"], L.n, L.max_len, o["slots"], L.stride, o["framedLen"], **enc_kw(i, L))

    name = "compress_fastdict_device" if fast else "compress_hcdict_device"
    return compress_built(name, ["mi355lz4_" + name, "mi355lz4_hcdict_load"], blocks, call, 65536, cfg={} if fast else {"level": 3},
                          extra=extra, dict_for=lambda v, i: dicts[v])


def dict_indices(n):
    """dictIdx of both variants: members -1..2, different at every block"""
    real = [(i % 4) - 1 for i in range(n)]
    return {"real": real, "decoy": [((i + 1 + i // 4) % 4) - 1 if ((i + 1 + i // 4) % 4) - 1 != real[i] else ((i + 2) % 4) - 1
                                    for i in range(n)]}


def b_compress_fastdict_multi():
    lens = ragged(24, 65536, 9)
    blocks = {v: word_blocks(lens, v, 500) for v in VARIANTS}
    idx = dict_indices(len(lens))
    extra = {v: {"dictIdx": arr(idx[v] + [0], np.int32)} for v in VARIANTS}
    members = set_dicts()

    def call(ctx, i, o, L):
        ctx.eng.compress_fastdict_multi_device(ctx.dset, i["dictIdx"], i["src"], L.n, L.max_len, o["slots"], L.stride,
                                               o["framedLen"], accel=1, **enc_kw(i, L))

    return compress_built("compress_fastdict_multi_device", ["mi355lz4_compress_fastdict_multi_device"], blocks, call, 65536,
                          extra=extra, dict_for=lambda v, i: members[idx[v][i]] if idx[v][i] >= 0 else None)


# ---- decode calls: framed, blockOff, outOff -> out, result -----------------------------------------------------------------------
CAP = 16384


def decode_built(name, symbols, frames, expect, call, kind=8, cfg=None, extra=None, waits=False, data=None):
    """frames[variant] = the framed blocks; expect[variant] = [(result, bytes) per block] by the oracle's decode; data[variant] =
    what a good block must decode to (valid())"""
    n = len(frames["real"])
    off, bufs = place(frames, 3, lead=5)
    out_off = [9 + i * (CAP + 5) for i in range(n)]
    out_bytes = 9 + n * (CAP + 5) + 64
    L = collections.namedtuple("L", "n kind framed_len")(n, kind, int(bufs["real"].size))
    inputs = {}
    for v in VARIANTS:
        inputs[v] = {"framed": bufs[v], "blockOff": arr(off + [0], np.int64), "outOff": arr(out_off + [0], np.int64)}
        if extra:
            inputs[v].update(extra[v])
    outs = {"out": (out_bytes, np.uint8), "result": (n, np.int32)}

    def canon(o):
        res = o["result"]
        return {"result": res.copy(), "out": [o["out"][out_off[i]:out_off[i] + clip(res[i], CAP)].tobytes() for i in range(n)]}

    def model(v):
        return {"result": arr([r for r, _ in expect[v]], np.int32), "out": [b for _, b in expect[v]]}

    def valid(v):
        if data is not None:
            for i, ((r, got), d) in enumerate(zip(expect[v], data[v])):
                if d is not None:
                    assert r == len(d) and got == d, "%s/%s block %d: the oracle decodes it to %d" % (name, v, i, r)

    return Built(name, symbols, inputs, outs, lambda ctx, i, o: call(ctx, i, o, L), canon, waits=waits, cfg=cfg, model=model,
                 valid=valid)


def independent_comps(blocks):
    return [orc().compress_block(b) for b in blocks]


N_DEC = 12


def dec_blocks(salt=0, kinds=("text", "lzsynth")):
    lens = ragged_pair(N_DEC, CAP)
    return {v: blocks_of(lens[v], v, salt=600 + salt, kinds=kinds) for v in VARIANTS}


LINKED_KINDS = ("text",)       # one kind, so that a block finds its matches in the block before it


def b_decompress_batch(mode):
    """mi355lz4_decompress_batch_device: decoders 1, 2, 4, 0; header kinds 8 and 4; checksums; linked with and without the wait"""
    cfg, kind, waits, linked = {}, 8, False, False
    if mode.startswith("decoder"):
        cfg = {"decoder": int(mode[7:])}
    elif mode == "kind4":
        kind = 4
    elif mode == "checksum":
        cfg = {"checksum": True}
    elif mode == "linked":
        linked, waits = True, True
    elif mode == "linked_async":
        linked, cfg = True, {"linked_async": 65536}
    blocks = dec_blocks(1, LINKED_KINDS) if linked else dec_blocks(0)
    comps = {v: M.linked_stream(orc(), blocks[v], ragged=True) if linked else independent_comps(blocks[v]) for v in VARIANTS}
    frames = {v: [M.frame(c, len(b), kind, bool(cfg.get("checksum"))) for c, b in zip(comps[v], blocks[v])] for v in VARIANTS}
    expect = {}
    for v in VARIANTS:
        caps = [len(b) if kind == 8 else CAP for b in blocks[v]]
        if linked:
            codes, outs, _ = M.model(orc(), [M.Block(f, c, cap, 0) for f, c, cap in zip(frames[v], comps[v], caps)])
            expect[v] = list(zip(codes, outs))
        else:
            expect[v] = [orc().decompress_block(c, cap) for c, cap in zip(comps[v], caps)]

    def call(ctx, i, o, L):
        ctx.eng.decompress_batch_device(i["framed"], L.framed_len, i["blockOff"], L.n, o["out"], i["outOff"], o["result"],
                                        header_kind=kind, fixed_uncomp=CAP if kind == 4 else 0, linked=linked)

    return decode_built("decompress_batch_device/" + mode, ["mi355lz4_decompress_batch_device"], frames, expect, call, kind=kind,
                        cfg=cfg, waits=waits, data=blocks)


STREAM_CUT = (0, 4, 8, 12)


def linked_streams(blocks, first_dict=None, cut=STREAM_CUT):
    """the compressed blocks of the streams blocks[cut[s]:cut[s + 1]], and what each decodes to in its stream; first_dict:
    stream 0 continues a stream whose last array was this dictionary"""
    comps, expect = [], []
    for s in range(len(cut) - 1):
        st = blocks[cut[s]:cut[s + 1]]
        if s == 0 and first_dict:
            cs = [c for _, c in dict_model.model_stream(first_dict, st, 1)]
        else:
            cs = M.linked_stream(orc(), st, ragged=True)
        codes, outs, _ = M.model(orc(), [M.Block(b"", c, len(b), 0) for c, b in zip(cs, st)], prev=first_dict[-65536:] if s == 0 and first_dict else None)
        comps += cs
        expect += list(zip(codes, outs))
    return comps, expect


def b_decompress_streams():
    blocks = dec_blocks(2, LINKED_KINDS)
    made = {v: linked_streams(blocks[v]) for v in VARIANTS}
    frames = {v: [M.frame(c, len(b), 8) for c, b in zip(made[v][0], blocks[v])] for v in VARIANTS}
    extra = {v: {"streamFirst": arr(STREAM_CUT, np.int32)} for v in VARIANTS}

    def call(ctx, i, o, L):
        ctx.eng.decompress_streams_device(i["framed"], L.framed_len, i["blockOff"], L.n, i["streamFirst"], len(STREAM_CUT) - 1,
                                          o["out"], i["outOff"], o["result"])

    return decode_built("decompress_streams_device", ["mi355lz4_decompress_streams_device"], frames, {v: made[v][1] for v in VARIANTS},
                        call, extra=extra, waits=True, data=blocks)


def b_decompress_dstreams(name="decompress_dstreams_device", blocks=None, slots=(5, 0, 7), reset=True, with_dict=True, cfg=None,
                          bad=None, cut=STREAM_CUT):
    """mi355lz4_decompress_dstreams_device behind dstreams_reset and dstreams_set_dict (stream 0's slot, dictionary late); bad[variant]
    = blocks whose trailer is corrupted (checksums on); cut = the stream table (streamFirst) over the blocks"""
    blocks = blocks or dec_blocks(3, LINKED_KINDS)
    dicts = {v: dict_input(v, 5) for v in VARIANTS}
    made = {v: linked_streams(blocks[v], dicts[v] if with_dict else None, cut) for v in VARIANTS}
    checksum = bool((cfg or {}).get("checksum"))
    frames = {v: [M.frame(c, len(b), 8, checksum, bad_checksum=bool(bad and i in bad[v]))
                  for i, (c, b) in enumerate(zip(made[v][0], blocks[v]))] for v in VARIANTS}
    extra = {v: {"dict": arr(np.frombuffer(dicts[v], dtype=np.uint8), np.uint8)} for v in VARIANTS} if with_dict else None
    sf, sl = list(cut), list(slots)

    def call(ctx, i, o, L):
        if reset:
            ctx.ds.reset()
        if with_dict:
            ctx.ds.set_dict(sl[0], i["dict"])
        ctx.eng.decompress_dstreams_device(ctx.ds, i["framed"], L.framed_len, i["blockOff"], L.n, sf, sl, o["out"], i["outOff"],
                                           o["result"])

    b = decode_built(name, ["mi355lz4_decompress_dstreams_device", "mi355lz4_dstreams_reset", "mi355lz4_dstreams_set_dict"], frames,
                     {v: made[v][1] for v in VARIANTS}, call, extra=extra, cfg=cfg, data=None if bad else blocks)
    b.table = (sf, sl)
    return b


def b_decompress_partial():
    blocks = dec_blocks(4)
    comps = {v: independent_comps(blocks[v]) for v in VARIANTS}
    frames = {v: [M.frame(c, len(b), 8) for c, b in zip(comps[v], blocks[v])] for v in VARIANTS}
    target = {v: np.random.RandomState(SEED[v]).randint(0, CAP + 1, size=N_DEC).tolist() for v in VARIANTS}
    target["real"][0], target["decoy"][0], target["real"][1], target["decoy"][1] = 0, 1, CAP, CAP - 1
    extra = {v: {"target": arr(target[v] + [0], np.int32)} for v in VARIANTS}
    # well-formed blocks: LZ4_decompress_safe_partial gives min(target, n) and the prefix (include/mi355lz4.h)
    expect = {v: [(min(t, len(b)), b[:min(t, len(b))]) for t, b in zip(target[v], blocks[v])] for v in VARIANTS}

    def call(ctx, i, o, L):
        ctx.eng.decompress_partial_device(i["framed"], L.framed_len, i["blockOff"], L.n, o["out"], i["outOff"], i["target"],
                                          o["result"])

    b = decode_built("decompress_partial_device", ["mi355lz4_decompress_partial_device"], frames, expect, call, extra=extra)

    def valid(v):
        for c, d in zip(comps[v], blocks[v]):
            assert orc().decompress_block(c, len(d)) == (len(d), d)
    b.valid = valid
    return b


def dict_compressed(dict_bytes, block):
    code, comp = dict_model.model_compress(dict_bytes or b"", block, 1)
    assert code > 0
    return comp


def b_decompress_dict():
    """mi355lz4_decompress_dict_device, the dictionary bytes late"""
    lens = ragged_pair(N_DEC, CAP)
    blocks = {v: word_blocks(lens[v], v, 700) for v in VARIANTS}
    dicts = {v: dict_input(v, 7) for v in VARIANTS}
    comps = {v: [dict_compressed(dicts[v], b) for b in blocks[v]] for v in VARIANTS}
    frames = {v: [M.frame(c, len(b), 8) for c, b in zip(comps[v], blocks[v])] for v in VARIANTS}
    expect = {v: [orc().decompress_block(c, len(b), dict_bytes=dicts[v]) for c, b in zip(comps[v], blocks[v])] for v in VARIANTS}
    extra = {v: {"dict": arr(np.frombuffer(dicts[v], dtype=np.uint8), np.uint8)} for v in VARIANTS}

    def call(ctx, i, o, L):
        ctx.eng.decompress_dict_device(i["framed"], L.framed_len, i["blockOff"], L.n, i["dict"], DICT_LEN, o["out"], i["outOff"],
                                       o["result"])

    return decode_built("decompress_dict_device", ["mi355lz4_decompress_dict_device"], frames, expect, call, extra=extra, data=blocks)


def b_decompress_dict_multi():
    lens = ragged_pair(N_DEC, CAP)
    blocks = {v: word_blocks(lens[v], v, 800) for v in VARIANTS}
    idx, members = dict_indices(N_DEC), set_dicts()
    member = lambda v, i: members[idx[v][i]][-65536:] if idx[v][i] >= 0 else None  # noqa: E731
    comps = {v: [dict_compressed(member(v, i), b) for i, b in enumerate(blocks[v])] for v in VARIANTS}
    frames = {v: [M.frame(c, len(b), 8) for c, b in zip(comps[v], blocks[v])] for v in VARIANTS}
    expect = {v: [orc().decompress_block(c, len(b), dict_bytes=member(v, i)) for i, (c, b) in enumerate(zip(comps[v], blocks[v]))]
              for v in VARIANTS}
    extra = {v: {"dictIdx": arr(idx[v] + [0], np.int32)} for v in VARIANTS}

    def call(ctx, i, o, L):
        ctx.eng.decompress_dict_multi_device(i["framed"], L.framed_len, i["blockOff"], L.n, ctx.dset, i["dictIdx"], o["out"],
                                             i["outOff"], o["result"])

    return decode_built("decompress_dict_multi_device", ["mi355lz4_decompress_dict_multi_device"], frames, expect, call, extra=extra,
                        data=blocks)


# ---- the small calls ----------------------------------------------------------------------------------------------------------------
def framed_inputs(kind, salt):
    blocks = dec_blocks(salt)
    comps = {v: independent_comps(blocks[v]) for v in VARIANTS}
    frames = {v: [M.frame(c, len(b), kind) for c, b in zip(comps[v], blocks[v])] for v in VARIANTS}
    off, bufs = place(frames, 3, lead=5)
    inputs = {v: {"framed": bufs[v], "blockOff": arr(off + [0], np.int64)} for v in VARIANTS}
    return blocks, comps, inputs, int(bufs["real"].size)


def scan(lens):
    return arr(np.concatenate([[0], np.cumsum(lens)]), np.int64)


def b_index():
    blocks, comps, inputs, flen = framed_inputs(8, 10)
    n = N_DEC

    def call(ctx, i, o):
        ctx.eng.index_device(i["framed"], flen, i["blockOff"], n, o["outOff"])

    def valid(v):
        for c, d in zip(comps[v], blocks[v]):
            assert orc().decompress_block(c, len(d)) == (len(d), d)

    return Built("index_device", ["mi355lz4_index_device"], inputs, {"outOff": (n + 1, np.int64)}, call,
                 lambda o: {"outOff": o["outOff"].copy()}, model=lambda v: {"outOff": scan([len(b) for b in blocks[v]])}, valid=valid)


def b_decoded_size():
    import size_model
    blocks, comps, inputs, flen = framed_inputs(4, 11)
    n = N_DEC

    def call(ctx, i, o):
        ctx.eng.decoded_size_device(i["framed"], flen, i["blockOff"], n, o["size"], o["outOff"], header_kind=4, max_uncomp=CAP)

    def model(v):
        sizes = [size_model.model_size(c, CAP) for c in comps[v]]
        return {"size": arr(sizes, np.int32), "outOff": scan([max(s, 0) for s in sizes])}

    def valid(v):
        for c, d in zip(comps[v], blocks[v]):
            assert orc().decompress_block(c, len(d)) == (len(d), d) and size_model.model_size(c, CAP) == len(d)

    return Built("decoded_size_device", ["mi355lz4_decoded_size_device"], inputs, {"size": (n, np.int32), "outOff": (n + 1, np.int64)},
                 call, lambda o: {"size": o["size"].copy(), "outOff": o["outOff"].copy()}, model=model, valid=valid)


def b_xxh32():
    lens = ragged(32, 20000, 12)
    lens[6] = 0
    blocks = {v: blocks_of(lens, v, salt=12) for v in VARIANTS}
    off, bufs = place(blocks, 5)
    n, seed = len(lens), 0x9E3779B1
    inputs = {v: {"base": bufs[v], "off": arr(off + [0], np.int64), "len": arr(lens + [0], np.int32)} for v in VARIANTS}

    def call(ctx, i, o):
        ctx.eng.xxh32_device(i["base"], i["off"], i["len"], n, seed, o["out"])

    return Built("xxh32_device", ["mi355lz4_xxh32_device"], inputs, {"out": (n, np.int32)}, call, lambda o: {"out": o["out"].copy()},
                 model=lambda v: {"out": arr([xxh32(b, seed) for b in blocks[v]], np.uint32).view(np.int32)},
                 valid=lambda v: None)


def b_compact():
    blocks = dec_blocks(13)
    frames = {v: [M.frame(c, len(b), 8) for c, b in zip(independent_comps(blocks[v]), blocks[v])] for v in VARIANTS}
    n = N_DEC
    stride = int(S().slot_stride_ex(CAP, 8, False))
    inputs = {}
    for v in VARIANTS:
        slots = np.full(n * stride, 0xEE, dtype=np.uint8)
        for i, f in enumerate(frames[v]):
            slots[i * stride:i * stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
        inputs[v] = {"slots": slots, "framedLen": arr([len(f) for f in frames[v]] + [0], np.int32)}
    cap = n * stride

    def call(ctx, i, o):
        ctx.eng.compact_device(i["slots"], stride, i["framedLen"], n, o["dense"], cap, o["denseOff"])

    def canon(o):
        do = o["denseOff"]
        return {"denseOff": do.copy(), "dense": [o["dense"][clip(do[i], cap):clip(do[i + 1], cap)].tobytes() for i in range(n)]}

    return Built("compact_device", ["mi355lz4_compact_device"], inputs, {"dense": (cap, np.uint8), "denseOff": (n + 1, np.int64)}, call,
                 canon, model=lambda v: {"denseOff": scan([len(f) for f in frames[v]]), "dense": list(frames[v])},
                 valid=lambda v: None)


# ---- pages ----------------------------------------------------------------------------------------------------------------------------
PAGE, MAX_PAGES, N_PAGE_INPUTS, PAGE_INPUT = 1024, 12, 16, 16384


def b_pages(flavour):
    """the three page calls: 16 inputs of 16 KiB, 1 KiB pages, chains of at most 12 pages (text and word text run
    out of pages, so `consumed` depends on the bytes; lzsynth ends after 9 or 10, so nPages does)"""
    hk = 8
    name = {"exact": "compress_pages_device", "fast": "compress_pages_fast_device", "fastdict": "compress_pages_fastdict_device"}[flavour]
    lens = [PAGE_INPUT] * N_PAGE_INPUTS
    if flavour == "fastdict":
        # word text that the dictionary serves, lzsynth that ends after 9 or 10 pages, and text that runs out of pages
        blocks = {v: [x[i % 3] for i, x in enumerate(zip(word_blocks(lens, v, 900), blocks_of(lens, v, salt=901, kinds=("lzsynth",)),
                                                         blocks_of(lens, v, salt=902, kinds=("text",))))] for v in VARIANTS}
        dicts = {v: dict_input(v, 9) for v in VARIANTS}
    else:
        blocks = {v: blocks_of(lens, v, salt=900) for v in VARIANTS}
        dicts = None
    off, bufs = place(blocks, 7)
    n, stride = N_PAGE_INPUTS, hk + PAGE
    inputs = {v: {"src": bufs[v], "srcOff": arr(off + [0], np.int64), "srcLen": arr(lens + [0], np.int32),
                  "pageSize": arr([PAGE] * n + [0], np.int32)} for v in VARIANTS}
    if dicts:
        for v in VARIANTS:
            inputs[v]["dict"] = arr(np.frombuffer(dicts[v], dtype=np.uint8), np.uint8)
    outs = {"pages": (n * MAX_PAGES * stride, np.uint8), "pageSrcLen": (n * MAX_PAGES, np.int32),
            "pageCompLen": (n * MAX_PAGES, np.int32), "nPages": (n, np.int32), "consumed": (n, np.int32)}

    def call(ctx, i, o):
        a = (i["src"], i["srcOff"], i["srcLen"], n, i["pageSize"], MAX_PAGES, o["pages"], stride, o["pageSrcLen"], o["pageCompLen"],
             o["nPages"], o["consumed"])
        if flavour == "exact":
            ctx.eng.compress_pages_device(*a, header_kind=hk)
        elif flavour == "fast":
            ctx.eng.compress_pages_fast_device(*a, header_kind=hk, accel=1)
        else:
            ctx.hd.load(i["dict"])
            ctx.eng.compress_pages_fastdict_device(ctx.hd, *a, header_kind=hk, accel=1)

    def canon(o):
        cnt = [clip(c, MAX_PAGES) for c in o["nPages"]]
        at = lambda i: range(i * MAX_PAGES, i * MAX_PAGES + cnt[i])  # noqa: E731
        return {"nPages": o["nPages"].copy(), "consumed": o["consumed"].copy(),
                "pageSrcLen": [tuple(int(o["pageSrcLen"][e]) for e in at(i)) for i in range(n)],
                "pageCompLen": [tuple(int(o["pageCompLen"][e]) for e in at(i)) for i in range(n)],
                "pages": [tuple(o["pages"][e * stride:e * stride + hk + clip(o["pageCompLen"][e], PAGE)].tobytes() for e in at(i))
                          for i in range(n)]}

    def model(v):
        if not pages_model.available():           # the model is C, built with gcc; without it the decode check below is all
            warnings.warn("compress_pages_device: no gcc, the byte model of LZ4_compress_destSize was not applied")
            return None
        chains = [pages_model.chain(b, PAGE, MAX_PAGES, hk) for b in blocks[v]]
        return {"nPages": arr([len(c) for c, _ in chains], np.int32), "consumed": arr([u for _, u in chains], np.int32),
                "pageSrcLen": [tuple(p[2] for p in c) for c, _ in chains], "pageCompLen": [tuple(p[1] for p in c) for c, _ in chains],
                "pages": [tuple(p[0] for p in c) for c, _ in chains]}

    def check(v, c):
        """every page decodes, on its own or against the dictionary, to the next pageSrcLen bytes of its input"""
        for i, data in enumerate(blocks[v]):
            pos = 0
            for page, sl, cl in zip(c["pages"][i], c["pageSrcLen"][i], c["pageCompLen"][i]):
                what = "%s/%s input %d at %d" % (name, v, i, pos)
                assert len(page) == hk + cl and 0 < cl <= PAGE and sl > 0, what
                r, got = orc().decompress_block(page[hk:], sl, dict_bytes=dicts[v] if dicts else None)
                assert r == sl and got == data[pos:pos + sl], what
                pos += sl
            assert pos == c["consumed"][i] and len(c["pages"][i]) == c["nPages"][i], "%s/%s input %d" % (name, v, i)

    syms = ["mi355lz4_" + name] + (["mi355lz4_hcdict_load"] if dicts else [])
    return Built(name, syms, inputs, outs, call, canon, model=model if flavour == "exact" else None, valid=lambda v: None, check=check)


# ---- the case list --------------------------------------------------------------------------------------------------------------------
COMPRESS_MODES = ("level0", "big", "segments4", "linked", "level3", "level9", "checksum", "exact")
DECODE_MODES = ("decoder1", "decoder2", "decoder4", "decoder0", "kind4", "checksum", "linked", "linked_async")


def _registry():
    r = collections.OrderedDict()
    for m in COMPRESS_MODES:
        r["compress_batch_device/" + m] = (lambda m=m: b_compress_batch(m))
    r["compact_device"] = b_compact
    for m in DECODE_MODES:
        r["decompress_batch_device/" + m] = (lambda m=m: b_decompress_batch(m))
    r["decompress_streams_device"] = b_decompress_streams
    r["decompress_partial_device"] = b_decompress_partial
    r["index_device"] = b_index
    r["decoded_size_device"] = b_decoded_size
    r["xxh32_device"] = b_xxh32
    r["compress_streams_device"] = b_compress_streams
    r["compress_dict_device"] = b_compress_dict
    r["decompress_dict_device"] = b_decompress_dict
    r["compress_hcdict_device"] = lambda: b_compress_hcdict(0)
    r["compress_fastdict_device"] = lambda: b_compress_hcdict(1)
    r["compress_fastdict_multi_device"] = b_compress_fastdict_multi
    r["decompress_dict_multi_device"] = b_decompress_dict_multi
    r["compress_pages_device"] = lambda: b_pages("exact")
    r["compress_pages_fast_device"] = lambda: b_pages("fast")
    r["compress_pages_fastdict_device"] = lambda: b_pages("fastdict")
    r["decompress_dstreams_device"] = b_decompress_dstreams
    r["compress_streams_fast_device"] = b_compress_streams_fast
    return r


REGISTRY = _registry()
CASE_NAMES = tuple(REGISTRY)
_BUILT = {}


def build(name):
    if name not in _BUILT:
        _BUILT[name] = REGISTRY[name]()
    return _BUILT[name]


def header_device_symbols():
    text = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    return sorted(set(re.findall(r"^int\s+(mi355lz4_\w+_device)\s*\(", text, flags=re.M)))


# ---- cross-call protocols: the cases -----------------------------------------------------------------------------------------------------
RING_CALLS = 9


def ring_cases(kind):
    """nine calls on ONE set with nine different stream tables and inputs; every call resets the set first (enqueued like the
    call), so its streams begin anew and the per-call models hold.  The tables differ in their block ranges (streamFirst and the
    block count), between call k and k + 1 and between k and k + 4 -- the call whose ring entry k takes over -- so a call that read
    another call's table would decode other ranges of its blocks, as other streams, and give other bytes."""
    out = []
    for k in range(RING_CALLS):
        slots = [(3 * k + j) % 11 for j in (0, 4, 7)]
        cut = [1 + (k % 3), 2 + (k % 2), 1 + ((k + 1) % 3)]
        if kind == "dstreams":
            first = tuple(int(x) for x in np.cumsum([0] + cut))
            lens = ragged_pair(first[-1], CAP)
            blocks = {v: blocks_of(lens[v], v, salt=2000 + k, kinds=LINKED_KINDS) for v in VARIANTS}
            out.append(b_decompress_dstreams("ring/dstreams/%d" % k, blocks=blocks, slots=slots, reset=True, with_dict=False, cut=first))
            continue
        streams = {v: [blocks_of(ragged(c, 8000, 50 + 3 * k + s, edges=False), v, salt=2100 + 10 * k + s, kinds=LINKED_KINDS) for s, c in enumerate(cut)]
                   for v in VARIANTS}
        if kind == "fstreams":
            out.append(b_compress_streams_fast("ring/fstreams/%d" % k, streams=streams, slots=slots, reset=True, with_dict=False))
        else:
            out.append(b_compress_streams("ring/cstreams/%d" % k, streams=streams, slots=slots, reset=True))
    return out


CUT_LENS = [[4096, 20000, 13, 65536, 1, 30000], [70000, 5, 4095, 12, 65536, 100], [1000, 1000, 65537, 20000, 64, 9000]]


def cut_cases(kind):
    """(the whole: three streams of six blocks in one call, [three calls of two blocks per stream, only the first resets])"""
    slots = (2, 9, 4)
    if kind == "dstreams":
        lens = {"real": [[min(n, CAP) for n in ln] for ln in CUT_LENS]}
        lens["decoy"] = [[n - 1 if n > 1 else 2 for n in ln] for ln in lens["real"]]       # (the results differ too)
        arrays = {v: [blocks_of(ln, v, salt=3000 + s, kinds=LINKED_KINDS) for s, ln in enumerate(lens[v])] for v in VARIANTS}
        comps = {v: [M.linked_stream(orc(), st, ragged=True) for st in arrays[v]] for v in VARIANTS}

        def part(name, lo, hi, reset):
            take = lambda x: {v: [b for st in x[v] for b in st[lo:hi]] for v in VARIANTS}  # noqa: E731
            blocks, cs = take(arrays), take(comps)
            frames = {v: [M.frame(c, len(b), 8) for c, b in zip(cs[v], blocks[v])] for v in VARIANTS}
            expect = {v: [(len(b), b) for b in blocks[v]] for v in VARIANTS}
            k = hi - lo
            sf = [0, k, 2 * k, 3 * k]

            def call(ctx, i, o, L):
                if reset:
                    ctx.ds.reset()
                ctx.eng.decompress_dstreams_device(ctx.ds, i["framed"], L.framed_len, i["blockOff"], L.n, sf, list(slots), o["out"],
                                                   i["outOff"], o["result"])
            b = decode_built(name, ["mi355lz4_decompress_dstreams_device"], frames, expect, call)
            b.table = (sf, list(slots))
            return b
        return part("cut/dstreams/whole", 0, 6, True), [part("cut/dstreams/%d" % p, 2 * p, 2 * p + 2, p == 0) for p in range(3)]
    streams = {v: [blocks_of(ln, v, salt=3100 + s, kinds=LINKED_KINDS) for s, ln in enumerate(CUT_LENS)] for v in VARIANTS}
    make = b_compress_streams_fast if kind == "fstreams" else b_compress_streams

    def part(name, lo, hi, reset):
        sub = {v: [st[lo:hi] for st in streams[v]] for v in VARIANTS}
        kw = dict(with_dict=False, checked=False) if kind == "fstreams" else dict(held={v: [st[:lo] for st in streams[v]] for v in VARIANTS})
        return make(name, streams=sub, slots=slots, reset=reset, max_len=70000, **kw)     # (one maxBlockLen: it picks the table)
    return part("cut/%s/whole" % kind, 0, 6, True), [part("cut/%s/%d" % (kind, p), 2 * p, 2 * p + 2, p == 0) for p in range(3)]


def seg_case(name, n, ln, salt):
    """n blocks of ln bytes through the segment path (mi355lz4_set_segments(4))"""
    blocks = {v: blocks_of([ln] * n, v, salt=salt) for v in VARIANTS}
    return compress_built(name, ["mi355lz4_compress_batch_device"], blocks,
                          lambda ctx, i, o, L: ctx.eng.compress_batch_device(i["src"], L.n, L.max_len, o["slots"], L.stride,
                                                                             o["framedLen"], accel=1, **enc_kw(i, L)),
                          ln, cfg={"segments": 4}, dict_for=lambda v, i: None)


def hcdict_case(name, n, top, salt):
    """n ragged blocks at level 3 against the first member of the dictionary set (loaded when the engine's objects are made)"""
    blocks = {v: word_blocks(ragged(n, top, 21), v, salt) for v in VARIANTS}
    members = set_dicts()
    return compress_built(name, ["mi355lz4_compress_hcdict_device"], blocks,
                          lambda ctx, i, o, L: ctx.eng.compress_hcdict_device(ctx.hd_fixed, i["src"], L.n, L.max_len, o["slots"],
                                                                              L.stride, o["framedLen"], **enc_kw(i, L)),
                          top, cfg={"level": 3}, dict_for=lambda v, i: members[0])


def scratch_cases(kind):
    """six calls of one shape on different data: five streams in turn, then the first stream again"""
    if kind == "segments":
        return [seg_case("scratch/segments/%d" % k, 8, 65536, 6000 + k) for k in range(6)]
    return [hcdict_case("scratch/hcdict/%d" % k, 24, 65536, 6100 + 40 * k) for k in range(6)]


def growth_cases(kind):
    """(a small call, one that needs a larger scratch) of the same kind"""
    if kind == "segments":
        return seg_case("growth/segments/small", 2, 8192, 4002), seg_case("growth/segments/large", 8, 65536, 4008)
    if kind == "hcdict":
        return hcdict_case("growth/hcdict/small", 6, 4096, 4106), hcdict_case("growth/hcdict/large", 24, 65536, 4124)
    if kind == "checksum":
        def one(name, n, bad):
            lens = ragged_pair(n, CAP)
            blocks = {v: blocks_of(lens[v], v, salt=4200 + n) for v in VARIANTS}
            comps = {v: independent_comps(blocks[v]) for v in VARIANTS}
            frames = {v: [M.frame(c, len(b), 8, True, bad_checksum=(i == bad[v])) for i, (c, b) in enumerate(zip(comps[v], blocks[v]))]
                      for v in VARIANTS}
            expect = {v: [(BLK_E_CHECKSUM, b"") if i == bad[v] else (len(b), b) for i, b in enumerate(blocks[v])] for v in VARIANTS}
            return decode_built(name, ["mi355lz4_decompress_batch_device"], frames, expect,
                                lambda ctx, i, o, L: ctx.eng.decompress_batch_device(i["framed"], L.framed_len, i["blockOff"], L.n,
                                                                                     o["out"], i["outOff"], o["result"]),
                                cfg={"checksum": True})
        # (dev_reserve keeps a quarter and 256 bytes over: 3 blocks leave room for 67)
        return one("growth/checksum/small", 3, {"real": 1, "decoy": 2}), one("growth/checksum/large", 100, {"real": 83, "decoy": 7})
    assert kind == "exact"

    def one(name, n, before):
        """before: the blocks the engine's stream has seen (None: the call starts the stream anew)"""
        blocks = {v: blocks_of(ragged(n, 32768, 23, edges=False), v, salt=4300 + n, kinds=LINKED_KINDS) for v in VARIANTS}

        def call(ctx, i, o, L):
            if before is None:
                ctx.eng.reset_compress_stream()
            ctx.eng.compress_batch_device(i["src"], L.n, L.max_len, o["slots"], L.stride, o["framedLen"], accel=1, **enc_kw(i, L))

        def model(v):
            seen = list(before[v]) if before else []
            comps = M.linked_stream(orc(), seen + blocks[v], ragged=True)[len(seen):]
            return [frame_of(c, len(b), 8) for c, b in zip(comps, blocks[v])]
        b = compress_built(name, ["mi355lz4_compress_batch_device"], blocks, call, 65536, cfg={"exact": True}, model=model, waits=True)
        b.blocks = blocks
        return b
    small = one("growth/exact/small", 2, None)
    return small, one("growth/exact/large", 8, small.blocks)


def checksum_verdict_cases():
    """four checksummed decodes for two streams in turn, a corrupted trailer in a different block of each call and variant"""
    out = []
    for k in range(4):
        lens = ragged_pair(N_DEC, CAP)
        blocks = {v: blocks_of(lens[v], v, salt=5000 + k) for v in VARIANTS}
        comps = {v: independent_comps(blocks[v]) for v in VARIANTS}
        bad = {"real": (2 * k + 1) % N_DEC, "decoy": (2 * k + 6) % N_DEC}
        frames = {v: [M.frame(c, len(b), 8, True, bad_checksum=(i == bad[v])) for i, (c, b) in enumerate(zip(comps[v], blocks[v]))]
                  for v in VARIANTS}
        expect = {v: [(BLK_E_CHECKSUM, b"") if i == bad[v] else (len(b), b) for i, b in enumerate(blocks[v])] for v in VARIANTS}
        b = decode_built("verdicts/%d" % k, ["mi355lz4_decompress_batch_device"], frames, expect,
                         lambda ctx, i, o, L: ctx.eng.decompress_batch_device(i["framed"], L.framed_len, i["blockOff"], L.n, o["out"],
                                                                              i["outOff"], o["result"]), cfg={"checksum": True})
        b.bad = bad
        out.append(b)
    return out


# ---- the verdict -----------------------------------------------------------------------------------------------------------------------
def same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return list(a) == list(b)


def first_difference(a, b):
    a, b = list(a), list(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i
    return min(len(a), len(b))


def verdict(name, kept, want, decoy, kept_raw):
    """None when kept equals want; else the message: the array, the first differing block and which form kept has"""
    for key in want:
        if same(kept[key], want[key]):
            continue
        raw = kept_raw.get(key)
        if decoy is not None and same(kept[key], decoy[key]):
            form = "equals the decoy's output (the call read its input too early)"
        elif raw is not None and bool((raw.view(np.uint8) == FILL).all()):
            form = "is still the fill pattern (the call wrote too late)"
        else:
            form = "equals neither the decoy's output nor the fill pattern"
        return "%s: %s differs from the reference run at block %d and %s" % (name, key, first_difference(kept[key], want[key]), form)
    return None


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------------
def configure(eng, cfg):
    c = dict(DEFAULT_CFG, **cfg)
    eng.set_compress_exact(c["exact"])
    eng.set_compression_level(c["level"])
    eng.set_block_checksum(c["checksum"])
    eng.set_linked_compress(c["linked"])
    eng.set_segments(c["segments"])
    eng.set_decoder(c["decoder"])
    eng.set_linked_async(c["linked_async"])


class Ctx:
    """an engine and the objects the cases' calls use, created on the default stream"""

    def __init__(self, torch, eng):
        lib = S()
        self.eng = eng
        self.cs = lib.CompressStreams(eng, 16)
        self.fs = lib.FastCompressStreams(eng, 16)
        self.ds = lib.DecompressStreams(eng, 16)
        self.hd = lib.HcDict(eng)
        self._dicts = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).to("cuda:0") for d in set_dicts()]
        self._members = [lib.HcDict(eng) for _ in self._dicts]
        for m, d in zip(self._members, self._dicts):
            m.load(d)
        self.hd_fixed = self._members[0]
        self.dset = lib.DictSet(eng, self._members)
        torch.cuda.synchronize()

    def close(self):
        for o in [self.dset, self.hd, self.ds, self.fs, self.cs] + self._members:
            o.close()


_TORCH_DTYPE = {"uint8": "uint8", "int32": "int32", "int64": "int64"}


class Slot:
    """the device side of one built case: the inputs the call reads, both variants beside them, the outputs and their copies"""

    def __init__(self, h, built):
        torch = h.torch
        self.h, self.b = h, built
        dev = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")  # noqa: E731  (a copy: some inputs are views of bytes)
        self.var = {v: {k: dev(a) for k, a in built.inputs[v].items()} for v in VARIANTS}
        self.inp = {k: t.clone() for k, t in self.var["decoy"].items()}
        mk = lambda: {k: torch.empty(max(n, 1), dtype=getattr(torch, _TORCH_DTYPE[np.dtype(dt).name]), device="cuda:0")  # noqa: E731
                      for k, (n, dt) in built.outs.items()}
        self.out, self.kept = mk(), mk()
        self.ref = None

    def load(self, v):
        for k, t in self.inp.items():
            t.copy_(self.var[v][k], non_blocking=True)

    def fill(self):
        for d in (self.out, self.kept):
            for t in d.values():
                t.view(self.h.torch.uint8).fill_(FILL)

    def keep(self):
        for k, t in self.kept.items():
            t.copy_(self.out[k], non_blocking=True)

    def fetch(self, d):
        return {k: t.cpu().numpy()[:self.b.outs[k][0]] for k, t in d.items()}

    def enqueue(self, ctx):
        """on the current stream, no synchronisation: real over the inputs, the call, the outputs kept, decoy back"""
        self.load("real")
        self.b.call(ctx, self.inp, self.out)
        self.keep_and_restore()

    def keep_and_restore(self):
        self.keep()
        self.load("decoy")


class Harness:
    def __init__(self, torch, record):
        self.torch, self._record = torch, record
        self.eng = S().Engine(0)
        self.ctx = Ctx(torch, self.eng)
        self.s = torch.cuda.Stream()
        self.streams = [self.s]                      # every stream stays alive: the engine's scratch slots remember their handles
        self.others = []                             # further engines
        self.calibrate()

    def close(self):
        self.torch.cuda.synchronize()
        for ctx in self.others:
            ctx.close()
            ctx.eng.close()
        self.ctx.close()
        self.eng.close()

    def new_stream(self):
        self.streams.append(self.torch.cuda.Stream())
        return self.streams[-1]

    def new_engine(self):
        eng = S().Engine(0)
        self.others.append(Ctx(self.torch, eng))
        return self.others[-1]

    def record(self, **rec):
        self._record("stream_order", rec)

    # -- the delay --
    def calibrate(self):
        torch = self.torch
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.pad = None
        if self.sleep is None:
            self.pad = (torch.empty(64 << 20, dtype=torch.uint8, device="cuda:0"), torch.empty(64 << 20, dtype=torch.uint8, device="cuda:0"))

        def timed(units):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(self.s):
                a.record()
                self._spin(units)
                b.record()
            self.s.synchronize()
            return a.elapsed_time(b)

        units = 1000000 if self.sleep else 4
        timed(units)                                  # (first use)
        ms = timed(units)
        if self.sleep and ms < 5.0:                   # aim at 20 ms for the figure that is kept
            units = int(units * 20.0 / max(ms, 1e-3))
            ms = timed(units)
        self.units_per_ms = units / ms
        self.record(what="calibration", delay="torch.cuda._sleep" if self.sleep else "64 MiB device-to-device copies",
                    units=units, ms=ms, units_per_ms=self.units_per_ms)

    def _spin(self, units):
        if self.sleep:
            self.sleep(int(units))
        else:
            for _ in range(max(1, int(units))):
                self.pad[0].copy_(self.pad[1], non_blocking=True)

    def delay(self, ms):
        self._spin(max(1, int(ms * self.units_per_ms + 1)))

    # -- runs --
    def slot(self, built):
        return Slot(self, built)

    def on_default(self, slot, var, ctx=None, timed=False):
        """the call on torch's default stream with `var` loaded: (the outputs, host seconds from the call to the end of the
        synchronise, host seconds to enqueue the input copies)"""
        torch, ctx = self.torch, ctx or self.ctx
        slot.fill()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        slot.load(var)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        slot.b.call(ctx, slot.inp, slot.out)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return slot.fetch(slot.out), t3 - t2, t1 - t0

    def reference(self, slots, ctx=None, model=True):
        """The reference run of one call, or of a sequence of calls that continue each other's state: on the default stream, a
        synchronise after every call -- real, decoy, and real again (warm, timed).  The kept outputs are held to the CPU model
        and the checks (model=False: a call that continues state its model does not know)."""
        slots = slots if isinstance(slots, (list, tuple)) else [slots]
        ctx = ctx or self.ctx
        configure(ctx.eng, slots[0].b.cfg)
        self.torch.cuda.synchronize()
        real = [self.on_default(s, "real", ctx)[0] for s in slots]
        decoy = [self.on_default(s, "decoy", ctx)[0] for s in slots]
        again = [self.on_default(s, "real", ctx) for s in slots]
        for slot, r, d, (a, t_ref, t_load) in zip(slots, real, decoy, again):
            b = slot.b
            slot.ref = {"real": b.canon(r), "decoy": b.canon(d)}
            slot.t_ref, slot.t_load = t_ref, t_load
            msg = verdict(b.name + " (default stream, run twice)", b.canon(a), slot.ref["real"], None, {})
            assert msg is None, msg
            for v in VARIANTS if model else ():
                want = b.model(v) if b.model else None
                if want is not None:
                    msg = verdict(b.name + "/" + v + " against the CPU model", slot.ref[v], want, None, {})
                    assert msg is None, msg
                elif b.model:
                    self.record(what=b.name, variant=v, cpu_model="not applied: the model could not be built here")
                if b.check:
                    b.check(v, slot.ref[v])
            for key in slot.ref["real"]:
                assert not same(slot.ref["real"][key], slot.ref["decoy"][key]), \
                    "%s: real and decoy give the same %s: a misordered call would pass" % (b.name, key)
        return [s.ref for s in slots]

    def delay_ms(self, slots):
        """10 x the slowest t_ref (plus the host time to enqueue the input copies, which run between the gate and the call)"""
        ms = 10.0 * 1000.0 * sum(s.t_ref + s.t_load for s in slots)
        assert ms <= 1000.0, "the case is too big: its delay would be %.0f ms" % ms
        return ms

    def late(self, slots, stream=None, ctx=None, no_wait=(), what=None):
        """the late run of one or more calls behind ONE delay on one stream; no_wait: indices of the calls whose return must find
        the gate unsignalled.  Returns the kept outputs in canonical form, per slot."""
        torch, ctx, stream = self.torch, ctx or self.ctx, stream or self.s
        for s in slots:
            s.load("decoy")
            s.fill()
        configure(ctx.eng, slots[0].b.cfg)
        torch.cuda.synchronize()
        ms = self.delay_ms(slots)
        gate = torch.cuda.Event()
        waited = []
        with torch.cuda.stream(stream):
            self.delay(ms)
            gate.record()
            for s in slots:
                s.enqueue(ctx)
                waited.append(gate.query())
        still = not gate.query()
        stream.synchronize()
        assert gate.query()
        self.record(what=what or slots[0].b.name, calls=len(slots), t_ref_ms=[1000.0 * s.t_ref for s in slots],
                    t_load_ms=[1000.0 * s.t_load for s in slots], delay_ms=ms, delay_outlasted_enqueue=still,
                    gate_signalled_at_return=waited)
        for k in no_wait:
            assert not waited[k], ("%s: the call returned after the gate behind the %.1f ms delay was signalled: it waited for its "
                                   "stream, and the header says it only enqueues" % (slots[k].b.name, ms))
        return [self.kept_of(s) for s in slots]

    def late_streams(self, plan, ctx=None, what=None):
        """the late runs of several calls for several streams in turn, nothing synchronised in between: plan = [(slot, stream)].
        Every call has a delay of its own in front of it on its stream (10 x its own warm time), so a call on a stream that has
        been synchronised meanwhile -- a scratch that changes hands waits for the stream that held it -- is late as well.
        Returns the kept outputs like late()."""
        torch, ctx = self.torch, ctx or self.ctx
        slots = [s for s, _ in plan]
        for s in slots:
            s.load("decoy")
            s.fill()
        configure(ctx.eng, slots[0].b.cfg)
        torch.cuda.synchronize()
        ms = [self.delay_ms([s]) for s in slots]
        seen = []
        for (slot, st), d in zip(plan, ms):
            if not any(st is x for x in seen):
                seen.append(st)
            with torch.cuda.stream(st):
                self.delay(d)
                slot.enqueue(ctx)
        for st in seen:
            st.synchronize()
        self.record(what=what or slots[0].b.name, calls=len(slots), streams=len(seen), t_ref_ms=[1000.0 * s.t_ref for s in slots],
                    t_load_ms=[1000.0 * s.t_load for s in slots], delay_ms=ms)
        return [self.kept_of(s) for s in slots]

    def kept_of(self, slot):
        raw = slot.fetch(slot.kept)
        return slot.b.canon(raw), raw

    def judge(self, slot, kept, want=None):
        canon, raw = kept
        msg = verdict(slot.b.name, canon, want or slot.ref["real"], slot.ref["decoy"] if slot.ref else None, raw)
        assert msg is None, msg

    def run_case(self, built):
        """reference run, a first late run (first use of the stream allocates), then the late run that is held to "no wait" """
        slot = self.slot(built)
        self.reference([slot])
        for warm in (False, True):
            kept = self.late([slot], no_wait=(0,) if warm and not built.waits else ())
            self.judge(slot, kept[0])
        return slot
