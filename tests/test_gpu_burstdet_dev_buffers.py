"""BurstDetector.detect_block_devptr on tests/dev_arena.py arenas, as tests/test_gpu_autocorr_dev_buffers.py does for
Autocorr: input, events and the two status words sit at offsets inside guarded allocations filled with 0xFF; afterwards
the input is intact, exactly min(count, cap) events and both status words are written, the guards are untouched, and
events, status, pending and position equal tests/burstdet_ref.py byte for byte over two consecutive calls."""
import numpy as np
import pytest

import burstdet_ref as bdr
from dev_arena import GUARD_MIN, Arena

pytestmark = pytest.mark.gpu
T = bdr.TILE
GUARD = max(GUARD_MIN, 2 * T + 1024)
#        name     cap (None: room for all)
CASES = [("W16", None), ("W16", 2), ("W64", None), ("W1", None), ("W1", 100), ("W1", 0)]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("name,cap", CASES)
def test_detect_block_devptr_on_arenas(ya, name, cap, off):
    x, make, _, cuts = bdr.case("cccf", name)
    lens = cuts["T+1"]
    want = bdr.want("cccf", name, "T+1")
    _, W, d, _, thr, minlen, _ = next(s for s in bdr.SHAPES if s[0] == name)
    q = ya.BurstDetector("cccf", W, d, thr, 0.0, minlen)
    for i, part in enumerate(bdr.cut(x, lens)):                   # the second call reads the state the first left
        ev, over, pend, pos = want[i]
        room = ev.size + 3 if cap is None else cap
        ax = Arena(ya, np.complex64, part.size, off=off, guard=GUARD).load(part)
        ae = Arena(ya, bdr.EVENT, room, off=(off + 2) % 4, guard=GUARD)
        ast = Arena(ya, np.uint32, 2, off=(off + 1) % 4, guard=GUARD)
        q.detect_block_devptr(ax.ptr, part.size, ae.ptr if room else None, room, ast.ptr)
        status = ast.fetch_output()
        assert (int(status[0]), int(status[1])) == (ev.size, int(over)), (name, cap, off, i)
        got = ae.fetch_output(min(ev.size, room))
        ax.assert_input_intact(part)
        assert got.tobytes() == ev[:room].tobytes(), (name, cap, off, i)
        assert q.position == pos and (q.pending is None) == (pend is None)
        if pend is not None:
            assert q.pending.tobytes() == pend.tobytes()
        for a in (ax, ae, ast):
            a.free()


def test_an_empty_call_writes_the_status_only(ya):
    q = ya.BurstDetector("cccf", 8, 8, 0.5)
    ast = Arena(ya, np.uint32, 2, off=1)
    q.detect_block_devptr(None, 0, None, 0, ast.ptr)
    assert ast.fetch_output().tolist() == [0, 0] and q.position == 0
    ast.free()


def test_overlapping_buffers_and_null_pointers_are_config_errors(ya):
    n = 64
    q = ya.BurstDetector("cccf", 8, 8, 0.5)
    xd = ya.DeviceArray(2 * n, np.complex64)
    xd.zero()
    ed = ya.DeviceArray(4, bdr.EVENT)
    sd = ya.DeviceArray(2, np.uint32)
    with pytest.raises(ya.ConfigError):
        q.detect_block_devptr(xd.ptr, n, xd.ptr, 4, sd.ptr)                    # events on the input
    with pytest.raises(ya.ConfigError):
        q.detect_block_devptr(xd.ptr, n, ed.ptr, 4, xd.ptr + 8 * (n - 1))      # status on the last input sample
    with pytest.raises(ya.ConfigError):
        q.detect_block_devptr(xd.ptr, n, ed.ptr, 4, ed.ptr + 40)               # status inside the events
    with pytest.raises(ya.ConfigError):
        q.detect_block_devptr(xd.ptr, n, None, 4, sd.ptr)                      # no events buffer, but a capacity
    with pytest.raises(ya.ConfigError):
        q.detect_block_devptr(xd.ptr, n, ed.ptr, 4, None)
    q.detect_block_devptr(xd.ptr, n, xd.ptr + 8 * n, 1, sd.ptr)                # adjacent is fine
    ya.synchronize()
    assert q.position == n
