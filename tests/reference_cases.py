"""The inputs on which the oracle is compared with the real reference codec.

The reference itself is only compiled where its sources are (oracle/_ref), so tests/golden/make_golden.py runs it on
these inputs and records what it returned in tests/golden/reference_vectors.json; tests/test_oracle.py and
tests/test_oracle_renorm.py run the oracle on the same inputs and compare.  Both sides take the inputs from here, so
the records and the checks always describe the same cases."""
import hashlib
import random

import numpy as np

RENORM_BL = 65536


def sha(b):
    return hashlib.sha256(b).hexdigest()


def results_record(results):
    """What a list of decompress_block results (code, output) is compared by: the codes and one digest of the outputs."""
    return {"codes": [code for code, _ in results], "out_sha256": sha(b"".join(out for _, out in results))}


def compress_cases(oracle):
    """(key, data, block_len, accel, header, linked): frame_compress over kinds, odd block lengths, accelerations,
    linked and independent blocks, both header sizes."""
    for kind in ("lzsynth", "text", "random"):
        for bl in (1, 12, 13, 100, 4096, 65536, 70000):
            data = oracle.gen(kind, 3, bl, first_block=11).tobytes()
            for accel in (1, 7, 400):
                for linked in (True, False):
                    for hdr in (8, 4):
                        key = "%s bl=%d accel=%d linked=%d hdr=%d" % (kind, bl, accel, linked, hdr)
                        yield key, data, bl, accel, hdr, linked


def decode_fuzz_cases(oracle):
    """(iteration, probes): per iteration a block compressed by the oracle, decoded with exact, larger and smaller
    capacities, truncated, and with one byte corrupted; every probe with and without a dictionary."""
    rng = random.Random(99)
    for it in range(400):
        kind = rng.choice(["lzsynth", "text", "random"])
        n = rng.choice([0, 1, 12, 13, 20, 64, 65, 100, 300, 2000])
        data = oracle.gen(kind, 1, max(n, 1), first_block=it)[:n].tobytes()
        comp = oracle.compress_block(data, rng.choice([1, 1, 9]))
        probes = [(comp, n), (comp, n + 7), (comp, max(n - 1, 0)), (comp[: max(1, len(comp) // 2)], n)]
        m = bytearray(comp)
        m[rng.randrange(len(m))] = rng.randrange(256)
        probes += [(bytes(m), n), (bytes(m), n + 64)]
        d = oracle.gen("text", 1, rng.choice([3, 500, 65536, 70000]), first_block=it + 5).tobytes()
        yield it, [(payload, cap, dct) for payload, cap in probes for dct in (None, d)]


def huge_length_blocks():
    """(name, payload, capacity): blocks whose literal / match length fields are multi-megabyte runs of 0xFF: the
    lengths reach 2^31 and beyond (cbits/lz4.c:1811-1818, 1854-1858, 2064-2065 compare them as size_t)."""
    run = 8_600_000                                     # 255 * run > 2^31
    lit = b"\xf0" + b"\xff" * run + b"\x07" + b"abc"    # literal length overflowing int
    mat = b"\x1f" + b"x" + b"\x01\x00" + b"\xff" * run + b"\x03" + b"\x50hello"
    mat_dict = b"\x1f" + b"x" + b"\x05\x00" + b"\xff" * run + b"\x03" + b"\x50hello"
    return [("lit", lit, 4096), ("lit_bigcap", lit, 1 << 20), ("match", mat, 4096), ("match_cap64", mat, 40),
            ("match_far", mat_dict, 1 << 16)]


def huge_length_cases():
    """(name, probes): huge_length_blocks() without and with a dictionary."""
    d = bytes(range(256)) * 16
    for name, payload, cap in huge_length_blocks():
        yield name, [(payload, cap, None), (payload, cap, d)]


def renorm_input(oracle):
    """2 GiB + 64 MiB for ONE compression context: zeros, with text from 32 MiB in front of the 2 GiB mark to the end,
    so that the table is full of live entries when the offsets are rebased."""
    n_blocks = (2 << 30) // RENORM_BL + 1024
    data = np.zeros(n_blocks * RENORM_BL, dtype=np.uint8)
    t0 = (2 << 30) // RENORM_BL - 512
    text = oracle.gen("text", 256, RENORM_BL, first_block=11)
    for b in range(t0, n_blocks):
        k = (b - t0) % 256
        data[b * RENORM_BL:(b + 1) * RENORM_BL] = text[k * RENORM_BL:(k + 1) * RENORM_BL]
    return data, t0
