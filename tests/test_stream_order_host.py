"""CPU checks of the stream-order cases (tests/stream_order.py): the late-input harness of tests/test_stream_order_gpu.py can only
tell a misordered call from a right one when `real` and `decoy` are both valid, have the same shapes and give different outputs in
every array the verdict compares.  And every *_device call that include/mi355lz4.h declares has a case, or is named exempt."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import stream_order as SO  # noqa: E402


def cross_call_cases():
    out = []
    for kind in ("fstreams", "cstreams", "dstreams"):
        out += SO.ring_cases(kind)
        whole, parts = SO.cut_cases(kind)
        out += [whole] + parts
    for kind in ("segments", "hcdict", "checksum", "exact"):
        out += list(SO.growth_cases(kind))
    for kind in ("segments", "hcdict"):
        out += SO.scratch_cases(kind)
    return out + SO.checksum_verdict_cases()


_CROSS = None


def all_cases():
    global _CROSS
    if _CROSS is None:
        _CROSS = cross_call_cases()
    return [SO.build(n) for n in SO.CASE_NAMES] + _CROSS


def test_every_device_call_of_the_header_has_a_case_or_is_exempt():
    declared = SO.header_device_symbols()
    assert len(declared) >= 22 and "mi355lz4_compress_batch_device" in declared, declared
    covered = set()
    for name in SO.CASE_NAMES:
        covered.update(SO.build(name).symbols)
    for sym in declared:
        assert (sym in covered) != (sym in SO.EXEMPT), "%s: %s" % (sym, "both a case and exempt" if sym in covered else
                                                                 "no stream-order case and not named exempt")
    for sym, why in SO.EXEMPT.items():
        assert why and (sym in declared or sym.startswith("mi355lz4_decompress_linked_")), sym
    # the calls that are enqueued in front of a case's call
    for sym in ("mi355lz4_cstreams_load_dict", "mi355lz4_hcdict_load", "mi355lz4_dstreams_reset", "mi355lz4_dstreams_set_dict",
                "mi355lz4_fstreams_reset", "mi355lz4_fstreams_set_dict", "mi355lz4_cstreams_reset"):
        assert sym in covered, sym


def test_the_waiting_calls_are_the_ones_the_header_names():
    waits = sorted(n for n in SO.CASE_NAMES if SO.build(n).waits)
    assert waits == ["compress_batch_device/exact", "decompress_batch_device/linked", "decompress_streams_device"]


def test_real_and_decoy_have_the_same_shapes():
    for b in all_cases():
        real, decoy = b.inputs["real"], b.inputs["decoy"]
        assert sorted(real) == sorted(decoy), b.name
        differ = 0
        for k in real:
            assert real[k].shape == decoy[k].shape and real[k].dtype == decoy[k].dtype, (b.name, k)
            differ += not np.array_equal(real[k], decoy[k])
        assert differ, b.name + ": real and decoy are the same input"
        # offsets, lengths of a compress call and stream tables are the same in both; only bytes, targets and indices differ
        for k in ("srcOff", "srcLen", "blockOff", "outOff", "off", "len", "pageSize", "streamFirst"):
            if k in real:
                assert np.array_equal(real[k], decoy[k]), (b.name, k)
        for k in ("src", "framed", "base", "slots", "dict", "dictIdx", "target"):
            if k in real:
                assert not np.array_equal(real[k], decoy[k]), (b.name, k)


def test_the_models_tell_real_from_decoy_in_every_array():
    seen = 0
    for b in all_cases():
        if b.model is None:
            continue
        real, decoy = b.model("real"), b.model("decoy")
        if real is None:
            continue
        seen += 1
        assert list(real) == list(decoy), b.name
        for key in real:
            assert not SO.same(real[key], decoy[key]), "%s: %s is the same for real and decoy: a misordered call would pass" % (b.name, key)
            if not isinstance(real[key], np.ndarray):
                # block by block: no block whose output the two variants share
                same = [i for i, (x, y) in enumerate(zip(real[key], decoy[key])) if x == y and len(x)]
                assert len(same) <= len(real[key]) // 4, (b.name, key, same)
    assert seen >= 30, seen


def test_both_inputs_are_valid():
    for b in all_cases():
        assert b.valid is not None, b.name
        for v in SO.VARIANTS:
            b.valid(v)


def test_dictionary_indices_differ_at_every_block_and_name_members():
    for n in (SO.N_DEC, 24):
        idx = SO.dict_indices(n)
        assert all(-1 <= i < len(SO.SET_DICT_LENS) for v in SO.VARIANTS for i in idx[v])
        assert all(a != b for a, b in zip(idx["real"], idx["decoy"]))
        assert set(idx["real"]) == {-1, 0, 1, 2}


def test_linked_decode_cases_depend_on_their_dictionaries():
    """a linked case whose blocks all decode on their own would pass on a decoder without dictionaries"""
    O = SO.orc()
    for name in ("decompress_batch_device/linked", "decompress_batch_device/linked_async", "decompress_streams_device",
                 "decompress_dstreams_device", "decompress_dict_device", "decompress_dict_multi_device"):
        b = SO.build(name)
        for v in SO.VARIANTS:
            framed, off = b.inputs[v]["framed"], b.inputs[v]["blockOff"]
            alone = 0
            want = b.model(v)
            for i in range(len(want["out"])):
                o = int(off[i])
                c = int.from_bytes(framed[o:o + 4].tobytes(), "little")
                r, got = O.decompress_block(framed[o + 8:o + 8 + c].tobytes(), len(want["out"][i]))
                alone += (r == len(want["out"][i]) and got == want["out"][i])
            assert alone < len(want["out"]) - 2, "%s/%s: %d of %d blocks decode without a dictionary" % (name, v, alone, len(want["out"]))


def test_corrupted_trailers_are_corrupt_exactly_where_they_claim():
    cases = SO.checksum_verdict_cases() + list(SO.growth_cases("checksum"))
    for b in cases:
        for v in SO.VARIANTS:
            framed, off = b.inputs[v]["framed"], b.inputs[v]["blockOff"]
            want = b.model(v)["result"]
            bad = []
            for i in range(len(want)):
                o = int(off[i])
                c = int.from_bytes(framed[o:o + 4].tobytes(), "little")
                data = framed[o + 8:o + 8 + c].tobytes()
                trailer = int.from_bytes(framed[o + 8 + c:o + 12 + c].tobytes(), "little")
                if trailer != SO.xxh32(data):
                    bad.append(i)
                    assert want[i] == SO.BLK_E_CHECKSUM, (b.name, v, i)
                else:
                    assert want[i] >= 0, (b.name, v, i)
            assert len(bad) == 1, (b.name, v, bad)
            if hasattr(b, "bad"):
                assert bad == [b.bad[v]], (b.name, v)
    positions = [(b.bad["real"], b.bad["decoy"]) for b in SO.checksum_verdict_cases()]
    assert len({p for pair in positions for p in pair}) == 2 * len(positions), positions


def test_the_verdict_names_the_form():
    fill = np.full(8, SO.FILL, dtype=np.uint8).view(np.int32)
    want, decoy = {"result": np.array([1, 2], np.int32)}, {"result": np.array([1, 3], np.int32)}
    assert SO.verdict("x", dict(want), want, decoy, {"result": want["result"]}) is None
    m = SO.verdict("x", dict(decoy), want, decoy, {"result": decoy["result"]})
    assert "result" in m and "block 1" in m and "decoy" in m and "too early" in m, m
    m = SO.verdict("x", {"result": fill}, want, decoy, {"result": fill})
    assert "fill pattern" in m and "too late" in m and "block 0" in m, m
    m = SO.verdict("x", {"result": np.array([7, 2], np.int32)}, want, decoy, {"result": np.array([7, 2], np.int32)})
    assert "neither" in m and "block 0" in m, m
    lists = {"out": [b"ab", b"cd"]}
    m = SO.verdict("x", {"out": [b"ab", b"cX"]}, lists, {"out": [b"zz", b"yy"]}, {})
    assert "out" in m and "block 1" in m, m


def blocks_in(b, v):
    """the blocks a case brings, in call order: the framed blocks of a decode case, the source blocks of a compress case"""
    i = b.inputs[v]
    if "framed" in i:
        out = []
        for o in i["blockOff"][:-1]:
            o = int(o)
            c = int.from_bytes(i["framed"][o:o + 4].tobytes(), "little")
            out.append(i["framed"][o:o + 8 + c].tobytes())
        return out
    return [i["src"][int(o):int(o) + int(n)].tobytes() for o, n in zip(i["srcOff"][:-1], i["srcLen"][:-1])]


@pytest.mark.parametrize("kind", ["fstreams", "cstreams", "dstreams"])
def test_cut_cases_hold_the_whole(kind):
    """the three calls of a cut bring, stream by stream, exactly the blocks of the one-call case, with the same slots"""
    whole, parts = SO.cut_cases(kind)
    assert len(parts) == 3
    streams, per = 3, 2
    assert whole.table[0] == [0, 6, 12, 18]
    for v in SO.VARIANTS:
        all_blocks = blocks_in(whole, v)
        assert len(all_blocks) == streams * per * len(parts) and len(set(all_blocks)) > len(all_blocks) // 2
        for p, part in enumerate(parts):
            assert part.table == ([0, per, 2 * per, 3 * per], whole.table[1]), (kind, p)
            got = blocks_in(part, v)
            want = [all_blocks[st * per * len(parts) + p * per + j] for st in range(streams) for j in range(per)]
            assert got == want, (kind, v, p)


@pytest.mark.parametrize("kind", ["fstreams", "cstreams", "dstreams"])
def test_ring_tables_differ(kind):
    """a ring entry is reused four calls later: call k's stream table differs from call k + 1's and from call k + 4's in its
    block ranges, so a call that read another call's entry would give other bytes"""
    tables = [b.table for b in SO.ring_cases(kind)]
    assert len(tables) == SO.RING_CALLS == 9
    for k, (first, slots) in enumerate(tables):
        for d in (1, 4):
            if k + d < len(tables):
                assert first != tables[k + d][0], (kind, k, d)
                assert slots != tables[k + d][1], (kind, k, d)
    if kind == "dstreams":
        # the decode model is per stream: the same blocks under a neighbour's ranges are other streams, and where the block
        # counts differ, other blocks
        counts = [t[0][-1] for t in tables]
        assert all(counts[k] != counts[k + 4] for k in range(len(counts) - 4)), counts
