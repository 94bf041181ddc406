"""CPU: the oracle restatement against the committed golden vectors, all of them generated from the real
reference by tests/golden/make_golden.py: known answers, and the reference's results on tests/reference_cases.py's
inputs."""
import hashlib

import pytest

import reference_cases


def sha(b):
    return hashlib.sha256(b).hexdigest()


def test_golden_version(golden):
    assert golden["lz4_version"] == 10903  # cbits/lz4.h:101-103


def test_kat_compressed_bytes(oracle, golden):
    for k in golden["kat"]:
        data = bytes.fromhex(k["input_hex"])
        comp = oracle.compress_block(data, k["accel"])
        assert comp.hex() == k["compressed_hex"], k["name"]
        code, out = oracle.decompress_block(comp, len(data))
        assert code == len(data) and out == data


def test_survey_kats(oracle):
    # SURVEY.md 8c (1)
    assert oracle.compress_block(b"").hex() == "00"
    assert oracle.compress_block(b"a" * 13).hex() == "13610100506161616161"
    assert oracle.compress_block(b"a" * 64).hex() == "1f61010027506161616161"
    assert len(oracle.compress_block(b"a" * 12)) == 13
    assert len(oracle.compress_block(bytes(65536))) == 267
    assert len(oracle.compress_block(bytes(262144))) == 1038


def test_kat_sizes_and_accel_clamp(oracle, golden):
    inputs = {"zeros64k": bytes(65536), "zeros256k": bytes(262144),
              "ramp64k": bytes(((i * 7 + (i >> 8)) & 255) for i in range(65536))}
    for k in golden["kat_sizes"]:
        c = oracle.compress_block(inputs[k["name"]], k["accel"])
        assert len(c) == k["size"] and sha(c) == k["sha256"], k
    by = {(k["name"], k["accel"]): k["size"] for k in golden["kat_sizes"]}
    assert by[("ramp64k", -1)] == by[("ramp64k", 0)] == by[("ramp64k", 1)] == 2249   # cbits/lz4.c:1577
    assert by[("ramp64k", 65537)] == by[("ramp64k", 1000000)] == 65794               # cbits/lz4.c:1578


def test_malformed_codes(oracle, golden):
    for m in golden["malformed"]:
        code, out = oracle.decompress_block(bytes.fromhex(m["payload_hex"]), m["cap"])
        assert code == m["code"], m["name"]
        if code >= 0:
            assert sha(out) == m["out_sha256"], m["name"]


def test_seeded_streams(oracle, golden):
    for s in golden["streams"]:
        data = oracle.gen(s["kind"], s["n_blocks"], s["block_len"]).tobytes()
        assert sha(data) == s["raw_sha256"], ("generator", s["kind"])
        fr = oracle.frame_compress(data, s["block_len"], s["accel"], 8, s["linked"])
        assert sha(fr) == s["framed_sha256"], s
        assert oracle.frame_decompress(fr, len(data), 8, 0, True) == data


def test_linked_stream_fixture(oracle, linked_golden):
    fr = bytes.fromhex(linked_golden["framed_hex"])
    bl = linked_golden["block_len"]
    blocks, pos = [], 0
    while pos < len(fr):
        c = int.from_bytes(fr[pos:pos + 4], "little")
        blocks.append(fr[pos + 8:pos + 8 + c])
        pos += 8 + c
    assert [oracle.decompress_block(b, bl)[0] for b in blocks] == linked_golden["standalone_codes"]
    out = oracle.frame_decompress(fr, 4 * bl, 8, 0, True)
    assert sha(out) == linked_golden["raw_sha256"]
    with pytest.raises(RuntimeError):
        oracle.frame_decompress(fr, 4 * bl, 8, 0, False)   # inter-block dependency is real


def test_compress_bound(oracle):
    assert oracle.compress_bound(65536) == 65809 and oracle.compress_bound(262144) == 263188
    assert oracle.compress_bound(0) == 16 and oracle.compress_bound(0x7E000001) == 0


# ---- against the reference itself: its results on tests/reference_cases.py's inputs, recorded by make_golden.py ----
def test_vs_reference_compress_bytes(oracle, reference_vectors):
    expect = reference_vectors["compress"]
    seen = set()
    for key, data, bl, accel, hdr, linked in reference_cases.compress_cases(oracle):
        assert sha(oracle.frame_compress(data, bl, accel, hdr, linked)) == expect[key], key
        seen.add(key)
    assert seen == set(expect)


def test_vs_reference_decode_fuzz(oracle, reference_vectors):
    expect = reference_vectors["decode_fuzz"]
    its = 0
    for it, probes in reference_cases.decode_fuzz_cases(oracle):
        got = reference_cases.results_record([oracle.decompress_block(p, cap, d) for p, cap, d in probes])
        assert got == expect[it], (it, got["codes"], expect[it]["codes"])
        its += 1
    assert its == len(expect)


def test_huge_length_fields_vs_reference(oracle, reference_vectors):
    expect = reference_vectors["huge_length"]
    names = []
    for name, probes in reference_cases.huge_length_cases():
        assert reference_cases.results_record([oracle.decompress_block(p, cap, d) for p, cap, d in probes]) == expect[name], name
        names.append(name)
    assert sorted(names) == sorted(expect)
