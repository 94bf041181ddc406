"""Decoded sizes without decoding, the part that needs no GPU: the acceptance rule (tests/size_model.py, what
mi355lz4_decoded_size_device answers) against the oracle, the symbol, the argument checks.

The rule's reason for being: a block it accepts with size s decodes into exactly s bytes as it decodes into any larger capacity
-- same result, same bytes.  That is what lets a caller lay blocks out at their sizes instead of at fixedUncomp."""
import ctypes as C
import os

import pytest

import lz4_synth as Z
import size_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3
BIG = 4 << 20


def _equivalent(oracle, block, s, what):
    want = oracle.decompress_block(block, s)
    for F in (s + 1, 65536, BIG):
        if F < s:
            continue
        got = oracle.decompress_block(block, F)
        assert got == want, "%s: cap %d gives %r..., cap %d gives %r..." % (what, s, want[0], F, got[0])
    return want


@pytest.fixture(scope="module")
def fuzz(oracle):
    return M.fuzz_blocks(oracle)


def test_model_accepts_compressor_output(oracle, fuzz):
    """every block the oracle's compressor writes is accepted with its length (zeros too), levels 1 and 9"""
    for n, comp, _ in fuzz:
        assert M.model_size(comp, 65536) == n
        assert M.model_size(comp, n) == n and (n == 0 or M.model_size(comp, n - 1) == M.UNKNOWN)
    for n in (0, 1, 12):
        for kind in M.FUZZ_KINDS:
            assert M.model_size(oracle.compress_block(M.gen(oracle, kind, n)), 65536) == n


def test_equivalence_on_mutated_blocks(oracle, fuzz):
    """600 mutated blocks: whatever the model accepts decodes the same into s bytes and into s + 1, 64 KiB, 4 MiB"""
    accepted = 0
    for i, (n, comp, mut) in enumerate(fuzz):
        _equivalent(oracle, comp, n, "block %d unmutated" % i)
        s = M.model_size(mut, BIG)
        if s >= 0:
            accepted += 1
            _equivalent(oracle, mut, s, "block %d mutated" % i)
    assert 50 < accepted < 550, accepted              # both sides of the rule are exercised


def test_equivalence_on_hand_built_blocks(oracle):
    """lz4_synth's independent cases, end family and length family (end_family holds the end rules' both sides)"""
    cases = Z.independent_cases() + Z.end_family() + Z.length_family()
    accepted = rejected = 0
    for c in cases:
        s = M.model_size(c.block, BIG)
        if s < 0:
            rejected += 1
            continue
        accepted += 1
        code, _ = _equivalent(oracle, c.block, s, repr(c))
        if c.valid:
            assert code == s, (c, code, s)
    assert accepted > 100 and rejected >= 8, (accepted, rejected)
    # what the rule must refuse, by name: end rules broken, a block that ends with a match, offset 0
    for c in Z.end_family():
        if c.family == "ends" and (not c.valid or c.name.startswith("offset 0")):
            assert M.model_size(c.block, BIG) == M.UNKNOWN, c


def test_capacity_dependent_codes_are_refused(oracle):
    """The classes that made the rule tighter than "well formed + end rules": each decodes differently into s and into more."""
    # an empty block whose token carries a match nibble: 0 into a larger capacity, -1 into none
    assert oracle.decompress_block(b"\x05", 0)[0] != oracle.decompress_block(b"\x05", 64)[0]
    assert M.model_size(b"\x05", 64) == M.UNKNOWN and M.model_size(b"\x00", 64) == 0
    # a match with extension bytes near the end whose offset reaches in front of the block: the code's position moves
    blk = Z.write_block([(b"abcdefgh", 9, 40)], b"0123456789ab")
    s = 8 + 40 + 12
    assert oracle.decompress_block(blk, s)[0] != oracle.decompress_block(blk, BIG)[0]
    assert M.model_size(blk, BIG) == M.UNKNOWN
    # the same match far from the end: one code whatever the capacity, and the size is reported (offsets are not judged)
    blk = Z.write_block([(b"abcdefgh", 9, 40)], bytes(range(32, 132)))
    s = 8 + 40 + 100
    assert M.model_size(blk, BIG) == s
    code, _ = _equivalent(oracle, blk, s, "bad offset far from the end")
    assert code < 0


def test_symbol_declared():
    import streamly_lz4_amd as S
    assert "mi355lz4_decoded_size_device" in S.DECLARED_SYMBOLS
    assert getattr(S.lib, "mi355lz4_decoded_size_device")
    hdr = open(os.path.join(ROOT, "include", "mi355lz4.h")).read()
    assert "int mi355lz4_decoded_size_device(" in hdr
    # the host-memory form the C++ wrapper's Engine::decodedSizes is built on: declared like every other call
    assert "mi355lz4_decoded_sizes_host" in S.DECLARED_SYMBOLS and getattr(S.lib, "mi355lz4_decoded_sizes_host")
    assert "int mi355lz4_decoded_sizes_host(" in hdr
    hpp = open(os.path.join(ROOT, "include", "streamly_lz4.hpp")).read()
    assert "std::vector<int32_t> decodedSizes(const BlockConfig &cfg, const Array &framed, int maxUncomp);" in hpp
    assert "#define MI355LZ4_BLK_E_SIZE_UNKNOWN (-0x7F000005)" in hdr
    assert hex(-M.UNKNOWN) == "0x7f000005"


def test_bad_arguments_need_no_device():
    import streamly_lz4_amd as S
    f = S.lib.mi355lz4_decoded_size_device
    assert f(None, None, 0, None, 0, 4, 65536, None, None) == E_ARG
    assert f(None, None, 0, None, -1, 4, 65536, None, None) == E_ARG
    assert f(None, None, 0, None, 1, 5, 65536, None, None) == E_ARG
    assert b"decoded_size_device" in S.lib.mi355lz4_last_error()
    g = S.lib.mi355lz4_decoded_sizes_host
    assert g(None, None, 0, None, 0, 4, 65536, None) == E_ARG
    assert b"decoded_sizes_host" in S.lib.mi355lz4_last_error()
