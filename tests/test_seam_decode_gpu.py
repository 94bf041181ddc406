"""The dictionary form of the lane-parallel decoder (decode_par.hpp, decode_block_par<false, true>) on hand-built blocks: every
call that runs it -- mi355lz4_decompress_dict_device, mi355lz4_decompress_dstreams_device with the dictionary in the slot and
in the previous block's output, and the second pass of the linked calls -- on the blocks of tests/lz4_synth.py cut at a
sequence boundary (seam_cuts: the structural corpus with its first k bytes turned into a dictionary) and on one probe match
placed on the dictionary's edges (seam_family), and on corrupted cuts.  Every result code is the oracle's
(oracle.decompress_block(block, cap, dict), lz4_synth.linked_expect for the linked forms), every byte where that code is not
negative, and nothing outside the blocks' capacities is written: the outputs lie in tests/guarded.py buffers.

What this found when it was written: no wrong code and no wrong byte.  All forms gave the oracle's results on all 1212 cuts,
all 3022 probe blocks and all 480 corrupted blocks (323 of them with a negative code), and wrote nothing outside the
capacities.  Every test of the file took under 1.1 s on an MI355X, the linked variants 0.04 .. 0.6 s each, so every variant
runs the full sets: none was given seam_cuts_small() (which equals seam_cuts() as long as no case decodes to more than
256 KiB).  It also found that two conditions of the `ok` expression cannot be observed from outside in the build as shipped:
PAR_FAR_WIDE is 0, so `spos + 16 <= 0` is compiled out, and a 16-bit offset never puts spos below -65535, so
dictLo = -min(dictLen, 65535) and -min(dictLen, 65536) accept the same matches.  The probes stay on both sides of both for
the day PAR_FAR_WIDE is switched on.

Later (with tests/test_frames_corpus_gpu.py): lz4_synth.seam_dictionary had made every dictionary of the seam family ONE
repeated byte, which a match read from the wrong place of the dictionary yields as well.  With dictionaries of all byte values
every test of this file gave the oracle's results again, unchanged.
"""
import random

import numpy as np
import pytest

import guarded as G
import lz4_synth as S
import test_parity_gpu as P
from test_parity_gpu import LINKED_VARIANTS, _decode_streams

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SYNC_EVERY = 128
STALE = 0xEE


# ---- the cases and what the oracle makes of them, once a module -----------------------------------------------------------------

@pytest.fixture(scope="module")
def cut_cases(oracle):
    """[(name, dict, block, cap, (code, bytes))] of the cuts"""
    return [(name, d, blk, cap, oracle.decompress_block(blk, cap, d)) for name, d, blk, cap, _ in S.seam_cuts()]


@pytest.fixture(scope="module")
def seam_cases(oracle):
    """the same of the seam family"""
    return [(name, S.seam_dictionary(dl), blk, cap, oracle.decompress_block(blk, cap, S.seam_dictionary(dl)))
            for name, dl, blk, cap, _ in S.seam_family()]


@pytest.fixture(scope="module")
def all_cases(cut_cases, seam_cases):
    return cut_cases + seam_cases


@pytest.fixture(scope="module")
def fuzz_cases(oracle):
    """40 cuts of at most 16 KiB compressed, 12 mutations each (truncated, 1..3 bytes overwritten, 1..5 bytes appended, the
    capacity moved by up to 20 bytes): [(name, dict, block, cap, (code, bytes))], the 12 of a cut one after another"""
    rng = random.Random(2027)
    small = [c for c in S.seam_cuts() if len(c[2]) <= 16384 and len(c[1]) > 0]
    cases = []
    for name, d, blk, cap, _ in rng.sample(small, 40):
        for m in range(12):
            comp, c = bytearray(blk), cap
            mode = 1 + m % 4
            if mode == 1:
                comp = comp[: rng.randrange(1, len(comp) + 1)]
            elif mode == 2:
                for _ in range(rng.randrange(1, 4)):
                    comp[rng.randrange(len(comp))] = rng.randrange(256)
            elif mode == 3:
                comp += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 6)))
            else:
                c = max(0, cap + rng.randrange(-20, 20))
            comp = bytes(comp)
            cases.append(("%s mutation %d" % (name, m), d, comp, c, oracle.decompress_block(comp, c, d)))
    codes = [e[0] for *_, e in cases]
    assert any(c < 0 for c in codes) and any(c >= 0 for c in codes), "the sample is one-sided"
    assert any(oracle.decompress_block(blk, cap)[0] != e[0] for _, _, blk, cap, e in cases), "no block needs its dictionary"
    return cases


# ---- buffers ------------------------------------------------------------------------------------------------------------------------

def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bytes_t(b, pad=16):
    return _t(np.frombuffer(bytes(b) + bytes(pad), dtype=np.uint8).copy())


class Blocks:
    """Blocks framed back to back (headerKind 8: the capacity in the header; 4: the capacities in outCap), as
    test_parity_gpu.test_linked_streams_fuzz_codes lays them out, and their outputs in one guarded buffer with tests/guarded.py's
    pattern between and around them."""

    def __init__(self, blocks_caps, kind=8, seed=31):
        self.n, self.kind, self.seed = len(blocks_caps), kind, seed
        parts, boff, pos = [], [], 0
        for blk, cap in blocks_caps:
            boff.append(pos)
            h = len(blk).to_bytes(4, "little") + (int(cap).to_bytes(4, "little") if kind == 8 else b"")
            parts += [h, blk]
            pos += len(h) + len(blk)
        self.framed_len = pos
        self.framed = _bytes_t(b"".join(parts))
        self.caps = [c for _, c in blocks_caps]
        self.lay = G.layout(self.caps)
        self.boff = _t(np.array(boff + [0], dtype=np.int64))
        self.ooff = _t(np.array(self.lay.starts + [0], dtype=np.int64))
        self.out = G.new_torch(self.lay.total, seed, DEV)
        self.res = G.GuardedArray(self.n, __import__("torch").int32, seed + 1, device=DEV)
        self.kw = dict(header_kind=kind, fixed_uncomp=max(self.caps + [0]) if kind == 4 else 0,
                       out_cap=_t(np.array(self.caps + [0], dtype=np.int32)) if kind == 4 else None)

    def check(self, cases, what):
        """after the device is idle: codes and bytes are the cases' expectations, nothing else was written; returns the codes"""
        G.assert_confined(self.out, self.lay.ranges(), self.seed, "%s: out" % (what,))
        self.res.check(what="%s: result" % (what,))
        codes = self.res.view.cpu().tolist()
        got = self.out.cpu().numpy()
        for i, (name, _, _, _, (code, dec)) in enumerate(cases):
            assert codes[i] == code, (what, name, codes[i], code)
            if code >= 0:
                o = self.lay.starts[i]
                if got[o:o + code].tobytes() != dec:
                    bad = int(np.argmax(got[o:o + code] != np.frombuffer(dec, np.uint8)))
                    raise AssertionError((what, name, "bytes differ at", bad))
        return codes


class Dicts:
    """every case's dictionary in ONE device buffer, a guard of pattern bytes around each"""

    def __init__(self, cases, seed=47, last_64k=False):
        self.seed = seed
        self.datas = [d[-65536:] if last_64k else d for _, d, _, _, _ in cases]
        self.lay = G.layout([len(d) for d in self.datas])
        host = G.new_numpy(self.lay.total, seed)
        for s, d in zip(self.lay.starts, self.datas):
            host[s:s + len(d)] = np.frombuffer(d, dtype=np.uint8)
        self.host = host
        self.buf = _t(host)

    def view(self, i):
        s = self.lay.starts[i]
        return self.buf[s:s + len(self.datas[i])]

    def check(self, what):
        import torch
        assert bool(torch.equal(self.buf, torch.from_numpy(self.host).to(DEV))), "%s: a dictionary was written" % (what,)


def _by_dict(cases):
    """the cases grouped by dictionary (the same bytes object): [(dict, [case])]"""
    groups = {}
    for c in cases:
        groups.setdefault(id(c[1]), (c[1], []))[1].append(c)
    return list(groups.values())


# ---- a. mi355lz4_decompress_dict_device ---------------------------------------------------------------------------------------------

def _dict_calls(engine, groups, kind=8):
    """one call per (dictionary, its blocks); no synchronisation in between"""
    import torch
    done = []
    for d, cases in groups:
        b = Blocks([(blk, cap) for _, _, blk, cap, _ in cases], kind)
        dt = _bytes_t(d, pad=0) if d else None
        engine.decompress_dict_device(b.framed, b.framed_len, b.boff, b.n, dt, len(d), b.out, b.ooff, b.res.view, **b.kw)
        done.append((b, dt, d, cases))
    torch.cuda.synchronize()
    codes = []
    for b, dt, d, cases in done:
        codes += b.check(cases, ("decompress_dict_device", len(d), kind))
        assert dt is None or dt.cpu().numpy().tobytes() == d, "the dictionary was written"
    return codes


@pytest.mark.parametrize("kind", [8, 4])
def test_dict_call_seam_family(engine, seam_cases, kind):
    """One call per dictionary length with all its probe blocks; with the capacity in the header, and in outCap."""
    groups = _by_dict(seam_cases)
    assert len(groups) == len(S.SEAM_DICT_LENS)
    _dict_calls(engine, groups, kind)


def test_dict_call_ignores_set_decoder(engine, seam_cases):
    """mi355lz4_set_decoder is ignored by this call: the same (the oracle's) results under 1, 2 and 4"""
    groups = _by_dict(seam_cases)
    try:
        for decoder in (1, 2, 4):
            engine.set_decoder(decoder)
            _dict_calls(engine, groups)
    finally:
        engine.set_decoder(0)


def _dict_call_each(engine, cases, what):
    """one call per case: the dictionaries in one buffer, the outputs and results in one allocation each, no host
    synchronisation between the calls but one every SYNC_EVERY calls"""
    import torch
    b = Blocks([(blk, cap) for _, _, blk, cap, _ in cases])
    dicts = Dicts(cases)
    for i in range(b.n):
        d = dicts.view(i)
        engine.decompress_dict_device(b.framed, b.framed_len, b.boff[i:], 1, d if len(d) else None, len(d), b.out, b.ooff[i:],
                                      b.res.view[i:], **b.kw)
        if i % SYNC_EVERY == SYNC_EVERY - 1:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    dicts.check(what)
    return b.check(cases, what)


def test_dict_call_cuts(engine, cut_cases):
    """One call per cut, every cut with its own dictionary."""
    _dict_call_each(engine, cut_cases, "decompress_dict_device, one call a cut")


# ---- b. mi355lz4_decompress_dstreams_device, the dictionary in the slot ------------------------------------------------------------

@pytest.fixture(scope="module")
def slots(slz4, engine, all_cases, fuzz_cases):
    ds = slz4.DecompressStreams(engine, max(len(all_cases), len(fuzz_cases)))
    yield ds
    ds.close()


def _dstreams_call(engine, ds, b, first, n_streams):
    engine.decompress_dstreams_device(ds, b.framed, b.framed_len, b.boff, b.n, first, list(range(n_streams)), b.out, b.ooff,
                                      b.res.view, **b.kw)


def _set_dicts(ds, dicts, n):
    for i in range(n):
        d = dicts.view(i)
        ds.set_dict(i, d if len(d) else None, len(d))


def _check_slots(ds, cases, codes, what, seed=5):
    """a seeded sample of slots, and the eight that are to hold the most: each holds the tail of its block's output where the
    block decoded to a byte at least, else the (last 64 KiB of the) dictionary it was given"""
    import torch
    torch.cuda.synchronize()
    rng = random.Random(seed)

    def content(i):
        _, d, _, _, (code, dec) = cases[i]
        return dec[-65536:] if code > 0 else d[-65536:]

    longest = sorted(range(len(cases)), key=lambda i: -len(content(i)))[:8]
    for i in rng.sample(range(len(cases)), 16) + longest:
        name, want = cases[i][0], content(i)
        cnt, held = ds.state(i)
        assert cnt == len(want) and held[:cnt] == want, (what, name, cnt, len(want))


@pytest.mark.parametrize("mode", ["whole", "last_64k", "stale"])
def test_dstreams_dictionary_in_the_slot(engine, slots, all_cases, mode):
    """set_dict per case, then ONE call with every case as a stream of one block.  whole: the dictionary as it is (over 64 KiB
    the slot keeps its last 64 KiB); last_64k: cut to that on the host; stale: every slot held 65536 bytes of 0xEE before, and
    a match that reaches one byte in front of a short dictionary still is the oracle's error, not a copy of that byte."""
    import torch
    n = len(all_cases)
    slots.reset()
    if mode == "stale":
        ee = torch.full((65536,), STALE, dtype=torch.uint8, device=DEV)
        for i in range(n):
            slots.set_dict(i, ee)
        assert any(name.endswith("one in front") and e[0] < 0 for name, _, _, _, e in all_cases)
    dicts = Dicts(all_cases, last_64k=(mode == "last_64k"))
    _set_dicts(slots, dicts, n)
    b = Blocks([(blk, cap) for _, _, blk, cap, _ in all_cases])
    _dstreams_call(engine, slots, b, list(range(n + 1)), n)
    torch.cuda.synchronize()
    dicts.check(mode)
    codes = b.check(all_cases, ("decompress_dstreams_device, dictionary in the slot", mode))
    _check_slots(slots, all_cases, codes, mode)


# ---- c. mi355lz4_decompress_dstreams_device, the dictionary from the previous block ---------------------------------------------

def _pairs(cases):
    """every case as the stream [literal_block(dict), block]: (cases with the literal blocks' expectations in between, the
    (block, cap) list)"""
    both = []
    for name, d, blk, cap, e in cases:
        both.append((name + " (its dictionary as a literal block)", b"", S.literal_block(d), len(d), (len(d), d)))
        both.append((name, d, blk, cap, e))
    return both


def test_dstreams_dictionary_from_the_previous_block_one_call(engine, slots, all_cases):
    """[literal_block(dict), block] per case, both blocks in one call: the dictionary is the literal block's output in `out`, of
    any length"""
    import torch
    both = _pairs(all_cases)
    n = len(all_cases)
    slots.reset()
    b = Blocks([(blk, cap) for _, _, blk, cap, _ in both])
    _dstreams_call(engine, slots, b, list(range(0, 2 * n + 1, 2)), n)
    torch.cuda.synchronize()
    codes = b.check(both, "decompress_dstreams_device, both blocks in one call")
    _check_slots(slots, all_cases, codes[1::2], "both blocks in one call")


def test_dstreams_dictionary_from_the_previous_call(engine, slots, all_cases):
    """all literal blocks in one call, all suffixes in the next: the dictionary is the slot's saved tail; the first call's
    output and input are overwritten in between"""
    import torch
    both = _pairs(all_cases)
    n = len(all_cases)
    slots.reset()
    first = Blocks([(blk, cap) for _, _, blk, cap, _ in both[0::2]])
    _dstreams_call(engine, slots, first, list(range(n + 1)), n)
    torch.cuda.synchronize()
    first.check(both[0::2], "decompress_dstreams_device, the literal blocks' call")
    first.out.fill_(0xAA)
    first.framed.fill_(0xAA)
    b = Blocks([(blk, cap) for _, _, blk, cap, _ in all_cases])
    _dstreams_call(engine, slots, b, list(range(n + 1)), n)
    torch.cuda.synchronize()
    codes = b.check(all_cases, "decompress_dstreams_device, the suffixes' call")
    _check_slots(slots, all_cases, codes, "two calls")


def test_dstreams_slot_holds_the_last_block_only(engine, slots, seam_cases):
    """The probes on a 100-byte dictionary: a 70000-byte literal block, then the 100 bytes as a literal block, then the probe
    block in a later call.  The slot holds exactly the 100 bytes -- nothing of the 70000 in front of them can be reached."""
    import torch
    cases = [c for c in seam_cases if len(c[1]) == 100]
    assert len(cases) > 100 and any(name.endswith("one in front") and e[0] < 0 for name, _, _, _, e in cases)
    n = len(cases)
    big = S.seam_dictionary(70000)
    heads = []
    for name, d, _, _, _ in cases:
        heads.append((name + " (70000 literals)", b"", S.literal_block(big), len(big), (len(big), big)))
        heads.append((name + " (100 literals)", b"", S.literal_block(d), len(d), (len(d), d)))
    slots.reset()
    first = Blocks([(blk, cap) for _, _, blk, cap, _ in heads])
    _dstreams_call(engine, slots, first, list(range(0, 2 * n + 1, 2)), n)
    torch.cuda.synchronize()
    first.check(heads, "the literal blocks' call")
    for i in range(n):
        cnt, held = slots.state(i)
        assert cnt == 100 and held[:100] == cases[i][1], (cases[i][0], cnt)
    first.out.fill_(0xAA)
    first.framed.fill_(0xAA)
    b = Blocks([(blk, cap) for _, _, blk, cap, _ in cases])
    _dstreams_call(engine, slots, b, list(range(n + 1)), n)
    torch.cuda.synchronize()
    b.check(cases, "the probes' call")


# ---- d. the linked calls ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(params=list(LINKED_VARIANTS))
def linked_variant(request, monkeypatch):
    for k, v in LINKED_VARIANTS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def _stream_layout_joined(frs, meta=8):
    """test_parity_gpu._stream_layout with the streams joined once: its `blob += fr` copies the whole blob per stream, which
    thousands of streams with 64 KiB dictionaries cannot afford.  The same result."""
    boff, first, ulen, base = [], [0], [], 0
    for fr in frs:
        pos = 0
        while pos < len(fr):
            c = int.from_bytes(fr[pos:pos + 4], "little")
            boff.append(base + pos)
            ulen.append(int.from_bytes(fr[pos + 4:pos + 8], "little"))
            pos += meta + c
        base += len(fr)
        first.append(len(boff))
    return b"".join(frs), boff, first, ulen


@pytest.fixture(scope="module")
def linked_sets(oracle, cut_cases, seam_cases):
    """per set: (the pairs, one framed stream per pair, the oracle's linked decode of ALL pairs as one stream)"""
    sets = {}
    for key, cases in (("cuts", cut_cases), ("seam family", seam_cases)):
        both = _pairs(cases)
        frs = [S.framed([(both[i][2], both[i][3]), (both[i + 1][2], both[i + 1][3])]) for i in range(0, len(both), 2)]
        one = S.linked_expect(oracle, [(name, blk, cap, True) for name, _, blk, cap, _ in both])
        sets[key] = (both, frs, one)
    return sets


def _check_linked(both, expect, out, res, ulen, what):
    o = 0
    for j, ((name, _, _, _, _), (code, dec)) in enumerate(zip(both, expect)):
        assert res[j] == code, (what, name, res[j], code)
        if code >= 0 and dec is not None:
            assert out[o:o + code] == dec, (what, name)
        o += ulen[j]


@pytest.mark.parametrize("which", ["cuts", "seam family"])
def test_linked_calls(engine, monkeypatch, linked_sets, linked_variant, which):
    """The two-block streams through mi355lz4_decompress_streams_device (every pair a stream of its own) and through
    mi355lz4_decompress_batch_device(linked = 1) (all pairs one stream: a block's dictionary is the last block in front of it
    that decoded to a byte at least, which for a cut at k = 0 is the pair before), under every linked variant: the tolerant
    first pass, the pointer kernels, the run walker, the replay and the run-in decode.  Every variant runs the full sets;
    none was given seam_cuts_small()."""
    monkeypatch.setattr(P, "_stream_layout", _stream_layout_joined)
    both, frs, one = linked_sets[which]
    out, res, ulen, _ = _decode_streams(engine, frs, "streams")
    _check_linked(both, [e for *_, e in both], out, res, ulen, (linked_variant, which, "streams"))
    out, res, ulen, _ = _decode_streams(engine, [b"".join(frs)], "one")
    _check_linked(both, one, out, res, ulen, (linked_variant, which, "one stream"))


# ---- e. corrupted blocks with a dictionary ---------------------------------------------------------------------------------------------

def test_fuzz_dict_call(engine, fuzz_cases):
    """one call per dictionary with its 12 mutated blocks"""
    groups = _by_dict(fuzz_cases)
    assert len(groups) == 40 and all(len(g) == 12 for _, g in groups)
    _dict_calls(engine, groups)


def test_fuzz_dstreams(engine, slots, fuzz_cases):
    """set_dict per block, then one call"""
    import torch
    n = len(fuzz_cases)
    assert n == 480
    slots.reset()
    dicts = Dicts(fuzz_cases)
    _set_dicts(slots, dicts, n)
    b = Blocks([(blk, cap) for _, _, blk, cap, _ in fuzz_cases])
    _dstreams_call(engine, slots, b, list(range(n + 1)), n)
    torch.cuda.synchronize()
    dicts.check("fuzz")
    codes = b.check(fuzz_cases, "decompress_dstreams_device, corrupted blocks")
    _check_slots(slots, fuzz_cases, codes, "fuzz")
