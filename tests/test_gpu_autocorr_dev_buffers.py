"""Autocorr.execute_block_devptr on tests/dev_arena.py arenas, as tests/test_gpu_ordfilt_dev_buffers.py does for OrdFilt:
input and outputs sit at an offset inside guarded allocations filled with 0xFF; afterwards the input is intact, every
output word is written, the guards are untouched and the results equal tests/autocorr_ref.py bit for bit, with and without
an energy buffer.  The inputs are finite, so a guard word (a NaN) that reached a result would show as a non-finite
output."""
import numpy as np
import pytest

import autocorr_ref as acr
from dev_arena import GUARD_MIN, Arena

pytestmark = pytest.mark.gpu
T, WMAX = acr.TILE, acr.WMAX
GUARD = max(GUARD_MIN, 2 * T + WMAX)                  # the delayed span of the last case starts T + 9 + 15 samples back
CASES = [(4, 3, 17), (64, 64, T + 1), (WMAX, 1, T - 1), (16, T + 9, 3 * T + 17)]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


_REF = {}


def reference(W, d, nb):
    """two consecutive calls of nb samples: (x, [(rxx, energy)] * 2), computed once"""
    if (W, d, nb) not in _REF:
        x = acr.stream(np.random.default_rng(W * 10 + d), "cccf", 2 * nb)
        r = acr.Autocorr("cccf", W, d)
        _REF[W, d, nb] = (x, [r.execute_block(x[:nb], energy=True), r.execute_block(x[nb:], energy=True)])
    return _REF[W, d, nb]


@pytest.mark.parametrize("with_energy", [True, False], ids=["energy", "rxx-only"])
@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("W,d,nb", CASES)
def test_execute_block_devptr_on_arenas(ya, W, d, nb, off, with_energy):
    x, want = reference(W, d, nb)
    q = ya.Autocorr("cccf", W, d)
    for i, part in enumerate((x[:nb], x[nb:])):                   # the second call reads the history of the first
        ax = Arena(ya, np.complex64, nb, off=off, guard=GUARD).load(part)
        ay = Arena(ya, np.complex64, nb, off=(off + 2) % 4, guard=GUARD)
        ae = Arena(ya, np.float32, nb, off=(off + 1) % 4, guard=GUARD) if with_energy else None
        q.execute_block_devptr(ax.ptr, nb, ay.ptr, ae.ptr if with_energy else None)
        got = ay.fetch_output()
        ax.assert_input_intact(part)
        assert got.tobytes() == want[i][0].tobytes(), (W, d, nb, off, i)
        if with_energy:
            assert ae.fetch_output().tobytes() == want[i][1].tobytes(), (W, d, nb, off, i)
            ae.free()
        ax.free()
        ay.free()


def test_overlapping_buffers_are_config_errors(ya):
    n = 64
    q = ya.Autocorr("cccf", 8, 8)
    xd = ya.DeviceArray(2 * n, np.complex64)
    xd.zero()
    ed = ya.DeviceArray(n, np.float32)
    with pytest.raises(ya.ConfigError):
        q.execute_block_devptr(xd.ptr, n, xd.ptr)                              # in place
    with pytest.raises(ya.ConfigError):
        q.execute_block_devptr(xd.ptr, n, xd.ptr + 8 * (n - 1))                # rxx starts on the last input sample
    with pytest.raises(ya.ConfigError):
        q.execute_block_devptr(xd.ptr, n, xd.ptr + 8 * n, xd.ptr + 8 * n)      # energy on rxx
    q.execute_block_devptr(xd.ptr, n, xd.ptr + 8 * n, ed.ptr)                  # adjacent is fine
    ya.synchronize()
