"""What mi355lz4_frames_load and mi355lz4_frames_decode may write (include/mi355lz4.h, "what a call may write"): with out,
result and buf in guarded layouts (tests/guarded.py: ragged regions, all 16 residues, position-dependent guard bytes), a batch
that mixes inputs that decode, inputs that fail at load and inputs that fail at decode time leaves every byte outside
[outOff[i], outOff[i] + sizes[i]) of the inputs with a size, and outside result[0, nInputs), as it was -- also when buf holds
OTHER valid frames of other sizes by the time the decode runs.  Results may then be errors; stray writes may not occur."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import frames_cases as FC  # noqa: E402
import frames_model as M  # noqa: E402
import guarded as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _batch(oracle, seed):
    named = [("golden/" + i, f) for i, f, _ in FC.golden() if "-b7-" not in i and ("65537" in i or "random" in i or "text13-" in i)]
    named += [("valid/" + n, f) for n, f, _ in FC.valid_cases(oracle)] + [("corrupt/" + n, f) for n, f, _ in FC.corrupt_cases(oracle)]
    random.Random(seed).shuffle(named)
    return named


@pytest.mark.parametrize("overwrite", [False, True], ids=["as-loaded", "buf-overwritten-before-decode"])
def test_frames_calls_are_confined(oracle, overwrite):
    import torch
    import streamly_lz4_amd as S
    eng = S.Engine(0)
    named = _batch(oracle, 21)
    other = _batch(oracle, 22)                                          # the same frames in another order: other sizes everywhere
    n = len(named)
    in_lay = G.layout([max(len(a[1]), len(b[1])) for a, b in zip(named, other)], first_residue=3)
    host = G.new_numpy(in_lay.total, 31)
    for s, (_, d) in zip(in_lay.starts, named):
        host[s:s + len(d)] = np.frombuffer(d, dtype=np.uint8)
    buf = _t(host)
    before = buf.clone()
    doff, dlen = _t(np.array(in_lay.starts, dtype=np.int64)), _t(np.array([len(d) for _, d in named], dtype=np.int64))
    fr = S.Frames(eng)
    sizes = fr.load(buf, doff, dlen)
    want = [M.model(d, oracle) for _, d in named]
    assert sizes == [w[0] for w in want]
    assert any(s < 0 for s in sizes) and any(w[0] >= 0 and w[1] < 0 for w in want) and any(w[1] >= 0 for w in want)
    assert torch.equal(buf, before), "mi355lz4_frames_load wrote to buf"
    if overwrite:
        host2 = G.new_numpy(in_lay.total, 32)
        for s, (_, d) in zip(in_lay.starts, other):
            host2[s:s + len(d)] = np.frombuffer(d, dtype=np.uint8)
        buf.copy_(_t(host2))
        before = buf.clone()
    out_lay = G.layout([max(s, 0) for s in sizes], first_residue=5)
    out = G.new_torch(out_lay.total, 41, DEV)
    res = G.GuardedArray(n, torch.int64, 43, DEV)
    off_before = np.array(out_lay.starts, dtype=np.int64)
    doutoff = _t(off_before)
    fr.decode(out, doutoff, res.view)
    torch.cuda.synchronize()
    allowed = [(s, s + z) for s, z in zip(out_lay.starts, sizes) if z > 0]
    G.assert_confined(out, allowed, 41, "mi355lz4_frames_decode, out")
    res.check(what="mi355lz4_frames_decode, result")
    assert torch.equal(buf, before) and np.array_equal(doutoff.cpu().numpy(), off_before)
    results = res.view.cpu().tolist()
    got = out.cpu().numpy()
    for (name, _), s, r, w, o in zip(named, sizes, results, want, out_lay.starts):
        if s < 0:
            assert r == s, name                                         # the load's code, whatever buf holds now
        elif not overwrite:
            assert r == w[1], name
            if r >= 0:
                assert got[o:o + s].tobytes() == w[2], name
        else:
            assert r == s or r in (M.E_BLOCK, M.E_CONTENT_CHECKSUM), name
    fr.close()
    eng.close()
