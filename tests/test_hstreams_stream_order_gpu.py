"""mi355lz4_compress_streams_fast_device with the set at level 9 on a NON-BLOCKING stream with late input (tests/stream_order.py;
tests/test_stream_order_gpu.py says what that is): the plan, k_encode_hc_fstreams and the save are enqueued on the engine's stream
like the level-0 launches, so the kept outputs equal the default stream's, byte for byte, and the warm call returns before the
gate in front of it is signalled -- it does not wait for its stream.  The set's level is a host-side attribute: it is set around
the runs and nothing of it is enqueued."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streamly-lz4_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import stream_order as SO  # noqa: E402

pytestmark = pytest.mark.gpu
LEVEL = 9


@pytest.fixture(scope="module")
def h(record):
    import torch
    hh = SO.Harness(torch, record)
    yield hh
    hh.close()


@pytest.fixture(autouse=True)
def stop_after_a_device_error(h):
    """a device that reports an error after a test ends the whole pytest session: nothing further runs on it"""
    yield
    try:
        h.torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        pytest.exit("the device reports an error after a stream-order test: %s" % e, returncode=3)


def total(ref):
    return int(sum(int(x) for x in ref["real"]["framedLen"]))


def test_late_input_at_level_nine(h):
    """the level-0 case of tests/stream_order.py as it is, the set at level 9 around it: reference run (held to lz4_check and the
    oracle's dictionary decode), a cold late run, and the warm late run that must not wait"""
    built = SO.b_compress_streams_fast(name="compress_streams_fast_device/set level 9")
    assert not built.waits
    fast = h.slot(SO.b_compress_streams_fast())
    h.reference([fast])                                                  # level 0: the other encoder's bytes, to tell the two apart
    assert h.ctx.fs.level == 0
    h.ctx.fs.set_level(LEVEL)
    try:
        slot = h.run_case(built)
        assert h.ctx.fs.level == LEVEL
    finally:
        h.ctx.fs.set_level(0)
    assert total(slot.ref) < total(fast.ref), "the set's level did not reach the encoder"


def test_stream_table_ring_at_level_nine(h):
    """nine calls with nine stream tables behind one delay, the set at level 9: every call sees its own table; the first four do
    not wait"""
    slots = [h.slot(b) for b in SO.ring_cases("fstreams")]
    h.ctx.fs.set_level(LEVEL)
    try:
        h.reference(slots)
        for warm in (False, True):
            kept = h.late(slots, no_wait=(0, 1, 2, 3) if warm else (), what="ring/fstreams at set level 9")
            for s, k in zip(slots, kept):
                h.judge(s, k)
    finally:
        h.ctx.fs.set_level(0)
