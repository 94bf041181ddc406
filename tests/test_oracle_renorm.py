"""LZ4_renormDictT (reference cbits/lz4.c:1545-1562, restated in oracle/lz4_oracle.c `renorm`): once more than 2 GiB
have gone through ONE compression context, the table's offsets are rebased.  The GPU path has no running offset
(positions are block-relative), so the restatement is exercised where it lives: the oracle's stream compressor and the
reference (its bytes recorded by tests/golden/make_golden.py) are fed the same 2 GiB + 64 MiB -- zeros, with text around
the point where the rebase happens, so that the table is full of live entries when it does -- and must write the same
bytes; the oracle's decoder must give the input back."""
import numpy as np

import reference_cases
from oracle.oracle import Oracle


def test_renorm_after_2gib_matches_reference(reference_vectors):
    orc = Oracle()
    BL = reference_cases.RENORM_BL
    data, t0 = reference_cases.renorm_input(orc)
    n_blocks = data.size // BL
    orc.lib.orc_debug_renorms.restype = __import__("ctypes").c_long
    before = orc.lib.orc_debug_renorms()
    a = orc.frame_compress(data, BL, 1, 8, True)
    assert orc.lib.orc_debug_renorms() == before + 1          # the rebase has really run, once
    expect = reference_vectors["renorm"]                       # the reference's bytes for the same input (make_golden.py)
    assert len(a) == expect["framed_len"] and reference_cases.sha(a) == expect["framed_sha256"]
    # and the tail decodes back (the blocks behind the rebase reference the blocks in front of it)
    back = orc.frame_decompress(a, n_blocks * BL, 8, BL, True)
    assert len(back) == n_blocks * BL
    tail = np.frombuffer(back, dtype=np.uint8)[t0 * BL:]
    assert np.array_equal(tail, data[t0 * BL:])
