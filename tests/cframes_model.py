"""The frame writer's contract in plain Python: the frame mi355lz4_cframes_compress must write for one input, given what the
encoder made of its blocks.

frame(data, block_size_id, flags, payloads) lays the frame out by the rules stated in include/mi355lz4.h ("writing batches of
standard LZ4 frames"): magic, FLG, BD, the content size, the header checksum byte, ceil(len / block size) blocks -- block k
stored when its compressed payload is no shorter than its bytes -- the end mark and the content checksum, with an xxh32 written
here from its published definition.  It shares no code with the library, and none with tests/frames_model.py, which the
host tests hold it against (a golden frame taken apart by frames_model.walk and rebuilt here is the same bytes).

Test infrastructure only (imported by tests, like lz4_synth.py).
"""
LINKED, BLOCK_CHECKSUM, CONTENT_SIZE, CONTENT_CHECKSUM = 1, 2, 4, 8
E_CAPACITY, E_INPUT = -0x7F000201, -0x7F000202

_M = 0xFFFFFFFF
_PRIMES = (2654435761, 2246822519, 3266489917, 668265263, 374761393)


def _rol(x, r):
    return ((x << r) & _M) | (x >> (32 - r))


def xxh32(data, seed=0):
    """xxHash32 by its specification: four lanes over 16-byte stripes, the tail in words and bytes, the avalanche"""
    p1, p2, p3, p4, p5 = _PRIMES
    data = bytes(data)
    n = len(data)
    at = 0
    if n >= 16:
        acc = [(seed + p1 + p2) & _M, (seed + p2) & _M, seed & _M, (seed - p1) & _M]
        while n - at >= 16:
            for lane in range(4):
                word = int.from_bytes(data[at + 4 * lane: at + 4 * lane + 4], "little")
                acc[lane] = (_rol((acc[lane] + word * p2) & _M, 13) * p1) & _M
            at += 16
        h = (_rol(acc[0], 1) + _rol(acc[1], 7) + _rol(acc[2], 12) + _rol(acc[3], 18)) & _M
    else:
        h = (seed + p5) & _M
    h = (h + n) & _M
    while n - at >= 4:
        h = (_rol((h + int.from_bytes(data[at: at + 4], "little") * p3) & _M, 17) * p4) & _M
        at += 4
    for b in data[at:]:
        h = (_rol((h + b * p5) & _M, 11) * p1) & _M
    h ^= h >> 15
    h = (h * p2) & _M
    h ^= h >> 13
    h = (h * p3) & _M
    h ^= h >> 16
    return h


def block_max(block_size_id):
    assert 4 <= block_size_id <= 7
    return 1 << (8 + 2 * block_size_id)


def cut(data, block_size_id):
    """the input's blocks: ceil(len / block size) of them, only the last may be short, none for an empty input"""
    bmax = block_max(block_size_id)
    return [bytes(data[at: at + bmax]) for at in range(0, len(data), bmax)]


def bound(n, block_size_id, flags):
    nb = -(-n // block_max(block_size_id))
    return (15 if flags & CONTENT_SIZE else 7) + nb * (8 if flags & BLOCK_CHECKSUM else 4) + n + 4 + (4 if flags & CONTENT_CHECKSUM else 0)


def header(block_size_id, flags, n):
    flg = 0x40 | (0 if flags & LINKED else 0x20) | (0x10 if flags & BLOCK_CHECKSUM else 0) | (0x08 if flags & CONTENT_SIZE else 0) | \
        (0x04 if flags & CONTENT_CHECKSUM else 0)
    desc = bytes([flg, block_size_id << 4]) + (n.to_bytes(8, "little") if flags & CONTENT_SIZE else b"")
    return (0x184D2204).to_bytes(4, "little") + desc + bytes([(xxh32(desc) >> 8) & 0xFF])


def stored(block, payload):
    """the writer's rule: a block whose compressed size is no smaller than the block is written as it is"""
    return payload is None or len(payload) >= len(block)


def frame(data, block_size_id, flags, payloads, blocks=None):
    """payloads[k]: the compressed bytes of block k (None: none were made).  blocks: the input's blocks where they are not the
    writer's cut (a liblz4 frame written with flushes has short blocks in its middle)"""
    data = bytes(data)
    blocks = cut(data, block_size_id) if blocks is None else [bytes(b) for b in blocks]
    assert len(payloads) == len(blocks) and b"".join(blocks) == data
    out = bytearray(header(block_size_id, flags, len(data)))
    for block, payload in zip(blocks, payloads):
        body = block if stored(block, payload) else bytes(payload)
        out += (len(body) | (0x80000000 if body is block else 0)).to_bytes(4, "little") + body
        if flags & BLOCK_CHECKSUM:
            out += xxh32(body).to_bytes(4, "little")
    out += bytes(4)
    if flags & CONTENT_CHECKSUM:
        out += xxh32(data).to_bytes(4, "little")
    return bytes(out)
