"""The inputs of the shared-dictionary tests, rebuilt from seeds: dictionaries, blocks, the three-block stream and the hand-built
decode cases.  tests/golden/make_dict_golden.py runs the reference over exactly these (tests/golden/dict_vectors.json holds
its return codes and sha256 sums, no input bytes); tests/dict_model.py is the model the GPU is compared with.

The grid.  Dictionary lengths sit on LZ4_loadDict's limits -- nothing, under HASH_UNIT (8), 8, 9 and 11 (one, one and two
positions entered), a short one, and around the 64 KiB that are kept; block lengths on the encoder's -- nothing, under
LZ4_minLength (13), 13, and past 64 KiB.  The text draws on a vocabulary of 300 words, so a dictionary overwrites its hash
buckets many times over: which writer a bucket keeps (the last) decides the bytes.

Test infrastructure only (imported by tests, like corpus.py).
"""
import random

import numpy as np

from lz4_synth import Builder, write_block

DICT_LENS = (0, 3, 7, 8, 9, 11, 100, 4095, 65535, 65536, 65537, 70000, 200000)
BLOCK_LENS = (0, 1, 4, 12, 13, 64, 1000, 4096, 65536, 100000)
ACCELS = (1, 7)
STREAM_LENS = (1000, 4096, 700)          # the three blocks continued after LZ4_loadDict, one stream per dictionary length
STREAM_ACCEL = 1

_LETTERS = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)


def _vocabulary():
    rs = np.random.RandomState(20261019)
    return [bytes(_LETTERS[rs.randint(0, 26, size=int(n))]) for n in rs.randint(2, 10, size=300)]


_VOCAB = _vocabulary()
_SEP = (b" ", b" ", b" ", b", ", b".\n")
_CACHE = {}


def text(seed, n):
    """n bytes of words of the vocabulary"""
    key = (seed, n)
    if key not in _CACHE:
        rs = np.random.RandomState(seed)
        out, size = [], 0
        while size < n:
            w = rs.randint(0, 300, size=4096)
            s = rs.randint(0, len(_SEP), size=4096)
            for a, b in zip(w, s):
                piece = _VOCAB[a] + _SEP[b]
                out.append(piece)
                size += len(piece)
                if size >= n:
                    break
        _CACHE[key] = b"".join(out)[:n]
    return _CACHE[key]


def dictionary(dict_len):
    return text(1000 + dict_len, dict_len)


def block(block_len):
    return text(500000 + block_len, block_len)


def stream_blocks():
    return [text(900000 + i, n) for i, n in enumerate(STREAM_LENS)]


def compress_key(dict_len, block_len, accel):
    return "d%d/b%d/a%d" % (dict_len, block_len, accel)


# ---- decode: hand-built blocks at the dictionary's edges -------------------------------------------------------------------------

DECODE_DICT_LENS = (100, 70000)


def decode_cases():
    """[(name, dictionary length, block, capacity)]: sequences placed on the external dictionary's edges (the first sequence of
    every block), followed by plain self-contained sequences so that the lane-parallel decoder's batches run too, and one more
    match deep in the block that lies wholly in the dictionary.  The codes and bytes come from the oracle and the golden."""
    rng = random.Random(11)
    cases = []

    def tail(b):
        b.fill(out_bytes=3000)
        b.add(2, b.op + 2 + 50, 8)                    # deep in the block: 8 bytes that end 42 bytes before the dictionary's end
        b.fill(out_bytes=500)
        return b.block(12)

    for D in DECODE_DICT_LENS:
        reach = min(D, 65535 - 3)
        cases.append(("offset onto the first reachable byte of the dictionary", D, *tail(Builder(rng, D).add(3, 3 + reach, 20))))
        if D < 65536:
            cases.append(("offset one byte in front of the dictionary", D, *tail(Builder(rng, D).add(3, 3 + D + 1, 20))))
        cases.append(("match from the dictionary into the block's own output", D, *tail(Builder(rng, D).add(1, 1 + 10, 24))))
        cases.append(("match inside the dictionary's last 4 bytes", D, *tail(Builder(rng, D).add(2, 2 + 4, 4))))
        cases.append(("offset 0", D, *tail(Builder(rng, D).add(3, 0, 8))))
        blk, n = tail(Builder(rng, D).add(3, 3 + 40, 20))
        cases.append(("capacity one byte short", D, blk, n - 1))
        cases.append(("truncated inside an offset field", D, blk[:1 + 3 + 1], n))
        b = Builder(rng, D).fill(out_bytes=1500)
        tok = len(write_block(b.seqs, final=False))
        b.add(4, b.op + 4 + 30, 12)
        blk, n = tail(b)
        cases.append(("truncated inside an offset field, deep", D, blk[:tok + 1 + 4 + 1], n))
    cases.append(("offset 65535", 70000, *tail(Builder(rng, 70000).add(3, 65535, 20))))
    cases.append(("offset 65535 deep in the block", 70000, *tail(Builder(rng, 70000).fill(out_bytes=2000).add(3, 65535, 300))))
    return cases
