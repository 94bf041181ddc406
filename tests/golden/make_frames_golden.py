"""Writes tests/golden/frames_vectors.json: the frames the system liblz4 (LZ4F_compressFrame, and the streaming writer with a
flush behind every piece) makes of tests/frames_cases.py's contents.  Run once on a CPU machine that has liblz4:

    python tests/golden/make_frames_golden.py

Only frames and content hashes are stored; the tests regenerate the contents from their seeds.  A stored block is kept as a
reference into the content, everything else zlib'd, so that the file stays under the largest golden fixture's size.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import frames_cases as FC  # noqa: E402
import lz4f  # noqa: E402

LIMIT = 113162          # tests/golden/reference_vectors.json, the largest fixture when this one was added


def main():
    L = lz4f.load()
    if L is None:
        raise SystemExit("liblz4 with LZ4F_* not found")
    vectors = []
    for (ident, kind, n, seed, bid, linked, bsum, csum, csize, level, writer) in FC.golden_specs():
        data = FC.content(kind, n, seed)
        kw = dict(block_id=bid, linked=bool(linked), content_checksum=bool(csum), block_checksum=bool(bsum),
                  content_size=n if csize else 0, level=level)
        frame = lz4f.compress_frame(L, data, **kw) if writer == "frame" else lz4f.compress_pieces(L, FC.pieces_of(data), **kw)
        assert lz4f.decompress(L, frame, n + 16) == data, ident
        segs = FC.encode_segments(frame, data)
        assert FC.decode_segments(segs, data) == frame, ident
        vectors.append({"id": ident, "kind": kind, "n": n, "seed": seed, "sha": hashlib.sha256(data).hexdigest()[:16], "segs": segs})
    path = FC.GOLDEN
    with open(path, "w") as f:
        json.dump({"writer": "liblz4 LZ4F", "vectors": vectors}, f, separators=(",", ":"))
        f.write("\n")
    size = os.path.getsize(path)
    print("%d vectors, %d bytes" % (len(vectors), size))
    assert size <= LIMIT, "the fixture outgrew the largest golden file"


if __name__ == "__main__":
    main()
