"""tests/guarded.py and tests/confinement_cases.py without a GPU: the layout really has the alignments and guard widths it
names, the checker sees one flipped byte wherever it lies and nothing on an untouched buffer, and the input sets that
tests/test_write_confinement_gpu.py decodes and compresses contain what that file claims to cover -- so the GPU test cannot
quietly leave cases out."""
import random

import numpy as np
import pytest

import confinement_cases as CC
import guarded as G
import lz4_synth as S


def test_layout_alignments_and_guards():
    for sizes in ([100] * 40, [65536] * 20, [0, 1, 12, 13, 5000, 65535, 65537] * 16,
                  [random.Random(1).randrange(5000) for _ in range(200)]):
        lay = G.layout(sizes)
        assert lay.start_residues() == set(range(16)), sizes[:3]
        assert lay.end_residues() == set(range(16)), sizes[:3]
        gaps = lay.gaps()
        assert len(gaps) == len(sizes) + 1
        assert gaps[0][0] == 0 and gaps[-1][1] == lay.total
        assert gaps[0][1] - gaps[0][0] >= 32768 and gaps[-1][1] - gaps[-1][0] >= 32768
        for a, b in gaps[1:-1]:
            assert b - a >= 1024 + 13 and b - a < 1024 + 13 + 16
        assert any((b - a) % 2 for a, b in gaps[1:-1])
        for (s, e), n in zip(lay.ranges(), sizes):
            assert e - s == n
    with pytest.raises(ValueError):
        G.layout([10], gap=512)
    with pytest.raises(ValueError):
        G.layout([10], end_guard=1024)


def test_layout_slots():
    lay = G.layout([100, 90, 100], stride=117, first_residue=3)
    assert lay.starts[0] % 16 == 3 and lay.starts[0] >= 32768
    assert [b - a for a, b in zip(lay.starts, lay.starts[1:])] == [117, 117]
    assert lay.total - (lay.starts[0] + 3 * 117) >= 32768
    with pytest.raises(ValueError):
        G.layout([200], stride=117)


def test_layout_typed_arrays():
    for dtype, item in ((np.int32, 4), (np.int64, 8), (np.uint32, 4)):
        a = G.GuardedArray(7, dtype, seed=3, lead=1)
        assert a.view.shape == (7,) and a.all.shape == (8,) and a.view.dtype == dtype
        assert a.view.ctypes.data % item == 0
        a.view[:] = 5
        a.check()
        a.all[0] = 1                                   # the item in front (result[-1] of a look-back call)
        with pytest.raises(AssertionError):
            a.check()


def test_pattern_depends_on_position_and_seed():
    p = G.pattern(0, 1 << 16, 1)
    assert len(set(p.tolist())) == 256
    assert abs(float(p.mean()) - 127.5) < 2
    for shift in (1, 2, 4, 8, 16, 64, 256, 1024, 4096, 32768):            # a stray COPY of nearby bytes is seen
        assert (p[shift:] == p[:-shift]).mean() < 0.02, shift
    assert (G.pattern(0, 4096, 1) == G.pattern(0, 4096, 2)).mean() < 0.02    # ... and one of another buffer's guard
    assert np.array_equal(G.pattern(1000, 50, 7), G.pattern(0, 1050, 7)[1000:])
    big = G.pattern((5 << 30) + 3, 64, 1)                                  # indices beyond 2^32 do not overflow
    assert big.dtype == np.uint8 and len(set(big.tolist())) > 30


def test_checker_flags_single_bytes():
    lay = G.layout([100, 0, 4097, 13])
    buf = G.new_numpy(lay.total, seed=9)
    assert G.violations(buf, lay.ranges(), 9) == (0, [])
    for s, e in lay.ranges():                                                # writes inside the allowed ranges
        buf[s:e] = 0xEE
    assert G.violations(buf, lay.ranges(), 9) == (0, [])
    s0, e0 = lay.ranges()[0]
    s2, e2 = lay.ranges()[2]
    gap_mid = (e0 + lay.starts[1]) // 2
    spots = {"before a region": (s2 - 1, 2, -1), "after a region": (e2, 2, 1), "middle of a guard": (gap_mid, None, None),
             "offset 0": (0, 0, -s0), "last byte": (lay.total - 1, 3, lay.total - lay.ranges()[3][1])}
    for name, (off, region, dist) in spots.items():
        b = buf.copy()
        b[off] ^= 0x01
        count, found = G.violations(b, lay.ranges(), 9)
        assert count == 1 and found[0][0] == off and found[0][3] == b[off], name
        if region is not None:
            assert found[0][1] == region and found[0][2] == dist, (name, found)
        with pytest.raises(AssertionError):
            G.assert_confined(b, lay.ranges(), 9, name)
    # the zero-length region's place is guard too
    b = buf.copy()
    b[lay.starts[1]] ^= 0x80
    assert G.violations(b, lay.ranges(), 9)[0] == 1
    # many violations: all counted, the first ones described
    b = buf.copy()
    b[:1000] = b[:1000] ^ 0xFF
    count, found = G.violations(b, lay.ranges(), 9)
    assert count == 1000 and len(found) == G._MAX_REPORT and found[0][0] == 0
    # a copy of the neighbouring guard bytes does not pass for the pattern
    b = buf.copy()
    b[e2:e2 + 16] = b[e2 + 16:e2 + 32]
    assert G.violations(b, lay.ranges(), 9)[0] >= 15


def test_checker_on_torch_cpu_tensors():
    torch = pytest.importorskip("torch")
    lay = G.layout([100, 3000])
    buf = G.new_torch(lay.total, seed=4, device="cpu")
    assert np.array_equal(buf.numpy(), G.new_numpy(lay.total, seed=4))
    assert G.violations(buf, lay.ranges(), 4) == (0, [])
    e = lay.ranges()[1][1]
    buf[e + 3] ^= 0xFF
    buf[lay.starts[0] + 5] = 1
    count, found = G.violations(buf, lay.ranges(), 4)
    assert count == 1 and found[0][:3] == (e + 3, 1, 4)
    a = G.GuardedArray(5, torch.int32, seed=6, device="cpu", lead=1)
    a.view[:] = 7
    a.check()
    a.all[0] = 7
    with pytest.raises(AssertionError):
        a.check()


def test_pair_differs_in_every_guard_byte():
    datas = [bytes([i]) * n for i, n in enumerate((100, 0, 5000))]
    lay = G.layout([len(d) for d in datas])
    a, b = G.pair(lay, datas)
    for (s, e), d in zip(lay.ranges(), datas):
        assert a[s:e].tobytes() == d and b[s:e].tobytes() == d
    for s, e in lay.gaps():
        assert not (a[s:e] == b[s:e]).any()


# ---- the input sets of the GPU tests -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases(oracle, golden):
    return CC.decode_cases(oracle, golden)


def test_decode_cases_families(cases, oracle, golden):
    fams = {c.family for c in cases}
    for fam in {c.family for c in S.independent_cases()}:
        assert "synth:" + fam in fams, fam
    assert sum(1 for c in cases if c.family.startswith("synth:")) == len(S.independent_cases())
    assert {"fuzz_small:%d" % m for m in range(5)} <= fams and {"fuzz_large:%d" % m for m in range(6)} <= fams
    assert {c.cap for c in cases if c.family == "oracle"} == set(CC.ORACLE_LENGTHS)
    assert {c.raw_len for c in cases if c.family.startswith("big:")} == {1 << 20, 4 << 20}
    assert len([c for c in cases if c.family == "huge"]) == 5
    classes = CC.capacity_classes(cases)
    assert len(classes["small"]) > 256 and classes["large"]             # (a small-class call is beyond variant 0's switch)
    # every layout the GPU test builds from these has all 16 start and end alignments
    # (the very sizes of the GPU test's calls: CC.region_sizes is what its plan is made from)
    for cls, cs in classes.items():
        for kind in (8, 4):
            for capmode in CC.CAPMODES:
                lay = G.layout([size for _, size in CC.region_sizes(cs, kind, capmode)[1]])
                assert lay.start_residues() == set(range(16)), (cls, kind, capmode)
                if cls == "small":                      # (the few big blocks of the large class cannot reach every end alignment)
                    assert lay.end_residues() == set(range(16)), (cls, kind, capmode, sorted(lay.end_residues()))


def test_decode_cases_fail_like_the_malformed_list(cases, oracle, golden):
    corrupted = [c for c in cases if c.corrupted and c.family != "malformed"]
    codes = [oracle.decompress_block(c.payload, c.cap)[0] for c in corrupted]
    assert sum(1 for r in codes if r < 0) * 4 >= len(corrupted), (sum(1 for r in codes if r < 0), len(corrupted))
    # the golden list's blocks are in the set with the codes recorded there, and every class of failure it names -- where in the
    # block the reference gave up -- also occurs among the corrupted blocks
    named = set()
    for m in golden["malformed"]:
        if m["payload_hex"]:
            p = bytes.fromhex(m["payload_hex"])
            assert oracle.decompress_block(p, m["cap"])[0] == m["code"], m["name"]
            named.add(CC.code_class(m["code"], len(p)))
    got = {CC.code_class(r, len(c.payload)) for c, r in zip(corrupted, codes)}
    assert named <= got, (named, got)
    assert {"first token", "inside", "tail", "end"} <= got


def test_decode_cases_capacities(cases, oracle):
    rel = set()
    for c in cases:
        if c.raw_len is not None:
            rel.add("smaller" if c.cap < c.raw_len else "equal" if c.cap == c.raw_len else "larger")
    assert rel == {"smaller", "equal", "larger"}
    # ... and decoded sizes short of the capacity occur among the blocks that decode
    assert any(0 <= oracle.decompress_block(c.payload, c.cap)[0] < c.cap for c in cases if c.family.startswith("fuzz"))


def test_encode_blocks(oracle):
    blocks = CC.encode_blocks(oracle)
    lens = {len(b) for b in blocks}
    assert {0, 1, 12, 13, 65535, 65536, 65537} <= lens
    for n in (65535, 65536, 65537):                   # the worst-case slot fill: an incompressible block of every edge length
        b = next(b for b in blocks if len(b) == n)
        assert len(oracle.compress_block(b, 1)) > n
    assert len(blocks) >= 50
    longest = blocks[-1]                              # the call's longest block does not compress: its slot is filled to the worst case
    assert len(longest) == max(len(b) for b in blocks) >= 65537 and len(oracle.compress_block(longest, 1)) > len(longest)
