"""PreambleDetector.detect_block_devptr and correlate_block_devptr on tests/dev_arena.py arenas, as
tests/test_gpu_burstdet_dev_buffers.py does for BurstDetector: input, events, the two status words, rxy and energy sit at
offsets inside guarded allocations filled with 0xFF; afterwards the input is intact, exactly min(count, cap) events and
both status words (or K n sums and n energies) are written, the guards are untouched, and everything equals
tests/pdet_ref.py byte for byte over two consecutive calls."""
import numpy as np
import pytest

import pdet_ref as pr
from dev_arena import GUARD_MIN, Arena

pytestmark = pytest.mark.gpu
T = pr.TILE
GUARD = max(GUARD_MIN, 2 * T + 1024)
#        name     family     cap (None: room for all)
CASES = [("L16", "noise", None), ("L16", "noise", 2), ("L64", "noise", None), ("L5", "noise", None), ("L5", "noise", 100),
         ("L5", "noise", 0), ("L257", "plateau", None)]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def gpu(ya, name, family):
    p, dphi, *_ = pr.case(name, family, ya.preamble_templates)
    return ya.PreambleDetector(p, dphi, pr.THRESHOLD)


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("name,family,cap", CASES)
def test_detect_block_devptr_on_arenas(ya, name, family, cap, off):
    _, _, x, _, _, cuts = pr.case(name, family, ya.preamble_templates)
    lens = cuts["T+1"]
    want = pr.want(name, family, "T+1", ya.preamble_templates)
    q = gpu(ya, name, family)
    for i, part in enumerate(pr.cut(x, lens)):                     # the second call reads the state the first left
        ev, over, pend, pos = want[i]
        room = ev.size + 3 if cap is None else cap
        ax = Arena(ya, np.complex64, part.size, off=off, guard=GUARD).load(part)
        ae = Arena(ya, pr.EVENT, room, off=(off + 2) % 4, guard=GUARD)
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


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("name,family,energy", [("L5", "noise", True), ("L64", "noise", False), ("L257", "plateau", True)])
def test_correlate_block_devptr_on_arenas(ya, name, family, energy, off):
    _, dphi, x, make, _, cuts = pr.case(name, family, ya.preamble_templates)
    q, ref = gpu(ya, name, family), make().co.clone()
    ref.reset()
    K = dphi.size
    for part in pr.cut(x, cuts["T+1"]):
        rxy, en = ref.correlate_block(part)
        ax = Arena(ya, np.complex64, part.size, off=off, guard=GUARD).load(part)
        ay = Arena(ya, np.complex64, K * part.size, off=(off + 1) % 4, guard=GUARD)
        ae = Arena(ya, np.float32, part.size, off=(off + 2) % 4, guard=GUARD)
        q.correlate_block_devptr(ax.ptr, part.size, ay.ptr, ae.ptr if energy else None)
        got = ay.fetch_output()
        ax.assert_input_intact(part)
        assert got.tobytes() == rxy.tobytes(), (name, off)
        if energy:
            assert ae.fetch_output().tobytes() == en.tobytes()
        for a in (ax, ay, ae):
            a.free()
    assert q.position == x.size


def test_an_empty_call_writes_the_status_only(ya):
    q = gpu(ya, "L16", "noise")
    ast = Arena(ya, np.uint32, 2, off=1)
    q.detect_block_devptr(None, 0, None, 0, ast.ptr)
    assert ast.fetch_output().tolist() == [0, 0] and q.position == 0
    ast.free()
    q.correlate_block_devptr(None, 0, None, None)                  # a no-op
    assert q.position == 0


def test_overlapping_buffers_and_null_pointers_are_config_errors(ya):
    n = 64
    q = gpu(ya, "L16", "noise")                                    # K = 3
    xd = ya.DeviceArray(4 * n, np.complex64)
    xd.zero()
    ed = ya.DeviceArray(4, pr.EVENT)
    sd = ya.DeviceArray(2, np.uint32)
    yd = ya.DeviceArray(3 * n, np.complex64)
    fd = ya.DeviceArray(n, np.float32)
    with pytest.raises(ya.ConfigError):
        q.detect_block_devptr(xd.ptr, n, xd.ptr, 4, sd.ptr)                    # events on the input
    with pytest.raises(ya.ConfigError):
        q.detect_block_devptr(xd.ptr, n, ed.ptr, 4, xd.ptr + 8 * (n - 1))      # status on the last input sample
    with pytest.raises(ya.ConfigError):
        q.detect_block_devptr(xd.ptr, n, ed.ptr, 4, ed.ptr + 48)               # status inside the events
    with pytest.raises(ya.ConfigError):
        q.detect_block_devptr(xd.ptr, n, None, 4, sd.ptr)                      # no events buffer, but a capacity
    with pytest.raises(ya.ConfigError):
        q.detect_block_devptr(xd.ptr, n, ed.ptr, 4, None)
    with pytest.raises(ya.ConfigError):
        q.correlate_block_devptr(xd.ptr, n, xd.ptr + 8 * (n - 1), fd.ptr)      # rxy on the last input sample
    with pytest.raises(ya.ConfigError):
        q.correlate_block_devptr(xd.ptr, n, yd.ptr, yd.ptr + 8 * (3 * n - 1))  # energy inside the last row of rxy
    with pytest.raises(ya.ConfigError):
        q.correlate_block_devptr(xd.ptr, n, yd.ptr, xd.ptr)                    # energy on the input
    with pytest.raises(ya.ConfigError):
        q.correlate_block_devptr(xd.ptr, n, None, fd.ptr)
    with pytest.raises(ya.ConfigError):
        q.correlate_block_devptr(None, n, yd.ptr, fd.ptr)
    assert q.position == 0
    q.detect_block_devptr(xd.ptr, n, xd.ptr + 8 * n, 1, sd.ptr)                # adjacent is fine
    q.correlate_block_devptr(xd.ptr, n, xd.ptr + 8 * n, fd.ptr)
    ya.synchronize()
    assert q.position == 2 * n
