"""The frame batch (mi355lz4_frames_load / mi355lz4_frames_decode) on the inputs of tests/frames_corpus.py: the structural and
the seam corpus of tests/lz4_synth.py inside frames, frames of up to 300 blocks, inputs of up to 200 frames, errors in
different 64-block chunks of a frame, the stored-block sweep, the block maxima, and 768 seeded mutations.  Every family goes
through Frames.load + Frames.decode in one call (the seam family in two), in an order shuffled with a fixed seed, at all 16
residues of inOff, the outputs between guard bytes: test_frames_gpu.run and check hold sizes[], result[] and every output byte
to tests/frames_model.py, and every byte outside the inputs' output ranges to the fill.

What this found when it was written (on fe38f21, MI355X):

Inputs, and what the model makes of them (accepted / refused at load / refused at decode), flags 0:
  A  independent frames  500 (264 blocks with code 5, 236 again with code 4)   474 / 20 / 6     6.3 MB of output
  A  third of a linked frame  500                                                480 / 20 / 0     7.1 MB
     (the six "offset to output start + 1" blocks find a byte in the blocks in front of them there)
  B  cuts  1212                                                                  1157 / 46 / 9    25.4 MB
  B  family  3022, two calls of 1511                                             2989 / 0 / 33    117.7 MB
  B  one in front of its frame, behind another frame  4                          0 / 0 / 4
  C  wide 115, one error 36, two errors 46, many frames 5, one call of 202       117 / 66 / 19    4 MB
  D  stored sweep  1120 (all four checksum/size combinations around 512 bytes)   1120 / 0 / 0     4.7 MB
  E  block maxima  30                                                            14 / 16 / 0      17.7 MB
  F  mutations  768: 46 still valid, 666 refused at load, 56 at decode; with both skip flags the checksum codes go

Disagreements met:
  1. Every frame with the one-byte compressed block 0x00 (the empty block: lz4_synth's "caps/empty" cases, the cut in front of
     a block's last, empty sequence, and every wide frame, which has such blocks on purpose) was refused with FRM_E_BLOCK at
     load.  The header and liblz4 take it as zero bytes; the library was wrong.  decoded_size_block's rule is right in the
     source, but in k_frames_sizes' instantiation the compiled exit for a size of 0 gave "no size" whatever the byte was (read
     in the kernel's disassembly; k_decoded_size's instantiation is right).  k_frames_sizes now sizes a one-byte block itself.
     220 inputs of A, B and C and 292 of F had differed; after the fix none does.
  2. lz4_synth.seam_dictionary made every dictionary one repeated byte (a generator per byte), so no test of the seam family,
     here or in test_seam_decode_gpu.py, could see a match read from the wrong place of the dictionary.  It makes real
     dictionaries now; both modules agree with the oracle on them.
  Nothing else: the stored sweep, the maxima, the 64-block chunks, the error order and the decoder variants gave the model's
  answers at the first run.  Where the system liblz4 loads, LZ4F_decompress gives the model's bytes for all 6397 inputs the
  model accepts (test_frames_corpus_host.py).

A deliberately wrong build (k_frames_layout placing a block without the sizes of the 64-block chunks in front of it) passes
test_frames_gpu.py and fails the wide-frame test and both mutation tests here.

Times on an MI355X: the inputs and the model's answers are computed in the module's fixtures, on the CPU -- 6.4 s for the seam
family, 4.2 s for the cuts, under 2 s for each other family (pure-Python xxh32; once a process, test_frames_corpus_host.py uses
the same).  The calls themselves: the independent corpus 0.01 .. 0.04 s a variant, a half of the seam family 0.08 s, the
mutations 0.12 s, the maxima's host forms 0.25 s, and with their family's preparation still inside the call the cuts 4.4 s, the
wide frames 1.9 s, the linked corpus 1.7 s, the maxima 1.4 s, the stored sweep 0.5 s.  In the whole suite no call of this
module took 2 s.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import frames_corpus as K  # noqa: E402
import frames_model as M  # noqa: E402
from conftest import DECODERS  # noqa: E402
from test_frames_gpu import check, expect, run  # noqa: E402

pytestmark = pytest.mark.gpu


def _family(name, flags=(0,), seed=2029, fixture_name=None):
    """a module-scoped fixture: [(name, input)] of a family in the order of its call, the model's answers computed (once a
    process: frames_corpus.family and test_frames_gpu.expect keep them), so that a test's own time is the GPU's"""
    @pytest.fixture(scope="module", name=fixture_name or name.lower().replace("-", "_"))
    def fixture(oracle):
        named = [(c[0], c[1]) for c in K.shuffled(K.family(name, oracle), seed)]
        for f in flags:
            for n, d in named:
                expect(oracle, n, d, f)
        return named
    return fixture


BOTH_SKIPS = M.SKIP_CONTENT_CHECKSUM | M.SKIP_BLOCK_CHECKSUM
a_independent, a_linked, b_cuts, b_family, b_behind = (_family(n) for n in ("A-independent", "A-linked", "B-cuts", "B-family", "B-behind"))
c_wide, c_one, c_pairs, c_many = (_family(n) for n in ("C-wide", "C-one", "C-pairs", "C-many"))
stored_sweep = _family("D", seed=K.STORED_SEED, fixture_name="stored_sweep")
maxima = _family("E", fixture_name="maxima")
mutations = _family("F", flags=(0, BOTH_SKIPS), fixture_name="mutations")


def _decode(engine, oracle, named, flags=0):
    got = run(engine, [d for _, d in named], flags=flags, residues=True)
    check(oracle, named, got, flags)
    return got


@pytest.mark.parametrize("decoder", DECODERS + [0])
def test_corpus_blocks_in_independent_frames(engine, oracle, a_independent, decoder):
    """A: every lz4_synth.independent_cases() block as the one block of an independent frame, which the planner decodes with a
    4-byte header and capacity = size, under every decoder variant"""
    engine.set_decoder(decoder)
    try:
        _decode(engine, oracle, a_independent)
    finally:
        engine.set_decoder(0)


def test_corpus_blocks_behind_two_blocks_of_a_linked_frame(engine, oracle, a_linked):
    """A: the same blocks as the third block of a linked frame: hist > 0, a shifted dst"""
    _decode(engine, oracle, a_linked)


def test_seam_cuts_as_linked_frames(engine, oracle, b_cuts):
    """B: all 1212 seam_cuts(), the dictionary as ragged stored and literal-only blocks in front of the case's block"""
    _decode(engine, oracle, b_cuts)


@pytest.mark.parametrize("part", [0, 1])
def test_seam_family_as_linked_frames(engine, oracle, b_family, part):
    """B: all 3022 seam_family() blocks the same way; about 118 MB of output, so every second case of the shuffled order a call"""
    _decode(engine, oracle, b_family[part::2])


def test_one_in_front_of_its_frame_behind_another_frame(engine, oracle, b_behind):
    """B: a match that reaches one byte in front of its own frame finds the frame before there; it is FRM_E_BLOCK all the same"""
    named = b_behind
    sizes, results, _ = _decode(engine, oracle, named)
    assert named and all(s > 0 for s in sizes) and results == [M.E_BLOCK] * len(named)


def test_wide_frames_many_frames_and_placed_errors(engine, oracle, c_wide, c_one, c_pairs, c_many):
    """C: frames of 63 .. 300 blocks in all 16 flag combinations, truly linked ones, one error at block 0, 63, 64, 65, 128 and
    the last, two errors in different 64-block chunks, inputs of 70 and 200 frames -- in one call"""
    _decode(engine, oracle, K.shuffled(c_wide + c_one + c_pairs + c_many, 2030))


def test_stored_block_sweep(engine, oracle, stored_sweep):
    """D: [stored P, stored N] for N on both sides of every form of wave_copy_bytes, P = 0 .. 15, independent and linked"""
    _decode(engine, oracle, stored_sweep)


def test_block_maxima(engine, oracle, maxima):
    """E: blocks that decode to exactly the maximum of codes 4 .. 7 and to one byte more, stored blocks of the maximum, block
    words of one more, three maximal blocks in a linked frame"""
    _decode(engine, oracle, maxima)


def test_block_maxima_host_forms(engine, oracle, maxima):
    """E through Engine.decompress_frames and through lz4FrameDecompress, the host-parsed reader of the same format"""
    import streamly_lz4_amd as S
    named = maxima
    parts, res = engine.decompress_frames([d for _, d in named], raise_on_error=False)
    for (name, data), p, r in zip(named, parts, res):
        _, wr, wp = expect(oracle, name, data)
        assert r == wr and p == (wp or b""), name
        if wr >= 0:
            assert S.lz4FrameDecompress(data, engine) == wp, name
        else:
            with pytest.raises(Exception):
                S.lz4FrameDecompress(data, engine)


@pytest.mark.parametrize("flags", [0, BOTH_SKIPS])
def test_seeded_mutations(engine, oracle, mutations, flags):
    """F: 768 mutations of 32 base frames in one call, and again with both skip flags"""
    _decode(engine, oracle, mutations, flags)
