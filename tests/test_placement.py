"""tests/placement.py pinned without a GPU, as tests/test_guarded.py pins guarded.py: the aliases, the four layouts for the
region lists tests/test_placement_gpu.py uses, and the window check on small numpy buffers with the marks scaled down (the same
code, placement.Space(24) in place of Space(32))."""
import numpy as np
import pytest

import guarded as G
import placement as P

SMALL = P.Space(24)


def test_aliases_either_side_of_the_marks():
    h, f = 1 << 31, 1 << 32
    assert P.FAR.total == h + f + (1 << 27) and P.FAR.front == h and P.FAR.view_len == f + (1 << 27)
    assert P.aliases(0) == [] and P.aliases(12345) == [] and P.aliases(h - 1) == []      # below 2^31 nothing is lost
    assert P.aliases(h) == [-h]                                   # int32: the lowest byte of the front pad
    assert P.aliases(h + 5) == [h + 5 - f]
    assert P.aliases(f - 1) == [-1]
    assert P.aliases(f) == [0]                                    # uint32
    assert P.aliases(f + 7) == [7]
    assert P.aliases(f + (1 << 27) - 1) == [(1 << 27) - 1]
    assert P.aliases(-5) == [f - 5]                               # (an offset inside the pad: not one a call is handed)
    # scaled: the same arithmetic
    assert SMALL.aliases(1 << 23) == [-(1 << 23)] and SMALL.aliases((1 << 24) + 7) == [7] and SMALL.aliases(100) == []
    # a shorter front pad keeps only the aliases that still lie inside the allocation
    wide = P.Space(32, front=1 << 30)
    assert wide.total == P.FAR.total and wide.view_len == P.FAR.total - (1 << 30)
    assert wide.aliases(h + 296) == [] and wide.aliases(3 * (1 << 30) + 444) == [-(1 << 30) + 444]
    assert wide.aliases(f + 592) == [592]


def test_a_straddling_region_has_the_aliases_of_its_last_byte():
    f = 1 << 32
    assert P.FAR.shifts(f - 100, 50) == [-f]
    assert P.FAR.shifts(f - 100, 200) == [-f]
    assert P.FAR.shifts((1 << 31) - 100, 200) == [-f]
    assert P.FAR.shifts((1 << 31) - 100, 50) == []
    assert P.FAR.shifts(f + 100, 50) == [-f]


def test_memory_order():
    assert P.memory_order(1) == [0] and P.memory_order(2) == [1, 0]
    assert P.memory_order(5) == [3, 1, 0, 2, 4] and P.memory_order(6) == [5, 3, 1, 0, 2, 4]
    for n in range(2, 40):
        o = P.memory_order(n)
        assert sorted(o) == list(range(n))
        assert o.index(1) < o.index(0)
        assert abs(o[0] - o[-1]) == 1                             # the lowest and the highest block follow one another


@pytest.fixture(scope="module")
def lists(oracle):
    import test_placement_gpu as TG
    return TG.region_lists(oracle)


def _props(sizes, mode, space=P.FAR, **kw):
    starts = P.place(sizes, mode, space, **kw)
    P.check_layout(starts, sizes, space, windows=mode.startswith("far"))
    return starts, P.describe(starts, sizes, space)


def test_layouts_of_the_gpu_tests(lists):
    assert len(lists) >= 20
    union = set()
    for name, sizes in lists.items():
        n = len(sizes)
        assert n >= 4 and max(sizes) >= 64, name
        for mode in P.MODES:
            for residue in (0, 1, 5, 9):
                starts, d = _props(sizes, mode, first_residue=residue)
                assert len(starts) == n and len(set(starts)) == n
                union |= d["residues"]
                if n >= 16:
                    assert d["residues"] == set(range(16)), (name, mode)
                else:                                             # consecutive residues: the lists of one test together have all
                    assert len(d["residues"]) == n, (name, mode)
                if mode == "dense":
                    assert starts == sorted(starts) and not d["below_predecessor"] and not d["above_full"], name
                    gaps = [b - (a + s) for a, b, s in zip(starts, starts[1:], sizes)]
                    assert all(G.GAP <= g < G.GAP + 16 for g in gaps), name
                if mode == "permuted":
                    assert d["below_predecessor"] and d["below_first"] and not d["above_full"], name
                    assert sorted(starts) == sorted(P.place([sizes[i] for i in P.memory_order(n)], "dense", first_residue=residue))
                if mode == "far":
                    assert starts == sorted(starts), name
                if mode in ("far", "far_permuted") and n >= 5:
                    assert d["near_zero"] and d["above_half"] and d["above_full"], (name, mode)
                if mode == "far_permuted":
                    assert d["below_predecessor"] and d["below_first"], name
                    assert d["max_predecessor_distance"] > (1 << 32), (name, d["max_predecessor_distance"])
    assert union == set(range(16))
    # the regions across the marks: every list has a long block where the far layouts put one across 2^31 and one across 2^32
    # (for the partial decode, whose targets 0 and 1 leave nothing to straddle with, under one of the four target shifts)
    partial = {}
    for name, sizes in lists.items():
        for mode in ("far", "far_permuted"):
            _, d = _props(sizes, mode)
            if name.startswith("partial out"):
                partial[mode] = partial.get(mode, False) or (d["straddles_half"] and d["straddles_full"])
            else:
                assert d["straddles_half"] and d["straddles_full"], (name, mode)
    assert partial == {"far": True, "far_permuted": True}


def test_single_regions_go_where_they_are_told():
    for size in (65536, 20 * 100500):
        s, d = _props([size], "far", zones=[4])
        assert d["above_full"] and not d["straddles_full"]
        s, d = _props([size], "far_permuted", zones=[3])
        assert d["straddles_full"]
        assert P.place([size], "dense") == P.place([size], "permuted")
        with pytest.raises(ValueError):
            P.place([size], "dense", zones=[4])                  # the dense layouts have no zones
    with pytest.raises(ValueError):
        P.place([10, 10], "far", zones=[3, 3])
    with pytest.raises(ValueError):
        P.place([10, 10], "far", zones=[4, 0])


def test_overlaps_are_refused():
    with pytest.raises(ValueError):
        P.check_layout([0, 100], [100, 10], P.FAR)                # adjacent
    with pytest.raises(ValueError):
        P.check_layout([1000, (1 << 32) + 1000], [10, 10], P.FAR)   # a region inside another one's alias window
    with pytest.raises(ValueError):
        P.check_layout([1000, 1000 + G.END_GUARD], [10, 10], P.FAR, windows=True)
    P.check_layout([1000, 1000 + G.END_GUARD], [10, 10], P.FAR, windows=False)
    with pytest.raises(ValueError):
        P.place([1 << 28] * 8, "far", SMALL)                      # does not fit


SIZES = [1, 13, 300, 4096, 70, 1000, 33, 2048]


@pytest.mark.parametrize("mode", P.MODES)
def test_window_check(mode):
    starts, d = _props(SIZES, mode, SMALL, first_residue=3)
    if mode.startswith("far"):
        assert d["straddles_half"] and d["straddles_full"] and d["above_full"] and d["near_zero"]
    buf = np.zeros(SMALL.total, dtype=np.uint8)
    win = P.Windows(starts, SIZES, SMALL, seed=5)
    win.fill(buf)
    assert win.violations(buf) == (0, [])                         # an untouched buffer
    for s, n in zip(starts, SIZES):                               # the regions themselves are the call's
        buf[s + SMALL.front:s + SMALL.front + n] ^= 0xFF
    assert win.violations(buf) == (0, [])
    win.check(buf, "regions written")
    k = 3
    for at, dist in ((starts[k] - 1, -1), (starts[k] + SIZES[k], 1), (starts[k] - G.END_GUARD, -G.END_GUARD),
                     (starts[k] + SIZES[k] + G.END_GUARD - 1, G.END_GUARD)):
        i = at + SMALL.front
        buf[i] ^= 0x40
        count, found = win.violations(buf)
        assert count == 1 and found[0][0] == at and found[0][3] == buf[i], (mode, at, found)
        if abs(dist) == 1:
            assert found[0][1:3] == (k, dist), (mode, found)
        with pytest.raises(AssertionError, match="1 bytes written outside the allowed ranges"):
            win.check(buf, "one flipped byte")
        buf[i] ^= 0x40
    assert win.violations(buf) == (0, [])


def test_window_check_sees_the_alias_windows():
    starts, _ = _props(SIZES, "far", SMALL)
    buf = np.zeros(SMALL.total, dtype=np.uint8)
    win = P.Windows(starts, SIZES, SMALL, seed=6)
    win.fill(buf)
    hit = 0
    for s, n in zip(starts, SIZES):
        for a in SMALL.aliases(s):                                # where a truncated offset would have written this region
            hit += 1
            for at in (a, a + n - 1, a - G.END_GUARD, a + n + G.END_GUARD - 1):
                if not SMALL.lo <= at < SMALL.hi:
                    continue
                i = at + SMALL.front
                buf[i] ^= 1
                assert win.violations(buf)[0] == 1, (s, a, at)
                buf[i] ^= 1
    assert hit >= 5                                               # every region from 2^31 on has one
    # the pattern of a window is its own: the bytes 2^bits further on are no copy of it
    s = starts[-1]
    a = SMALL.aliases(s)[0]
    w0 = buf[s - 64 + SMALL.front:s + SMALL.front].copy()
    w1 = buf[a - 64 + SMALL.front:a + SMALL.front]
    assert not np.array_equal(w0, w1)


def test_put_inputs_and_decoys():
    import test_placement_gpu as TG
    datas = [bytes([i + 1]) * n for i, n in enumerate(SIZES)]
    dec = TG.decoys(datas)
    assert all(len(a) != len(b) for a, b in zip(datas, dec))
    starts = P.place(SIZES, "far_permuted", SMALL)
    buf = np.zeros(SMALL.total, dtype=np.uint8)
    P.put_inputs(buf, starts, datas, dec, SMALL)
    n_alias = 0
    for s, d, c in zip(starts, datas, dec):
        assert P.read(buf, s, len(d), SMALL) == d
        for a in SMALL.aliases(s):
            n_alias += 1
            assert P.read(buf, a, len(c), SMALL) == c             # other valid input, of another length
    assert n_alias >= 5
    with pytest.raises(ValueError):
        P.put_inputs(buf, starts, datas, datas, SMALL)            # a decoy that equals its input proves nothing
