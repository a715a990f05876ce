"""OrdFilt.execute_block_devptr on tests/dev_arena.py arenas, as tests/test_gpu_dev_buffers.py does for the older
objects: input and output sit at an offset inside guarded allocations filled with 0xFF; afterwards the input is intact,
every output word is written, the guards are untouched and the result equals tests/ordfilt_ref.py bit for bit.  The
inputs are finite, so a guard word (a NaN) that reached a result would show as a non-finite output."""
import numpy as np
import pytest

import ordfilt_ref as ofr
from dev_arena import GUARD_MIN, Arena

pytestmark = pytest.mark.gpu
T, NMAX = ofr.TILE, ofr.NMAX
GUARD = max(GUARD_MIN, T + NMAX)
CASES = [(5, 17), (64, T + 1), (255, 3 * T + 17), (NMAX, T - 1)]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("n,nb", CASES)
def test_execute_block_devptr_on_arenas(ya, n, nb, off):
    rng = np.random.default_rng(n * 10 + off)
    x = ofr.tie_heavy(rng, 2 * nb)
    x[1::3] = rng.standard_normal(x[1::3].size).astype(np.float32)
    k = n // 2
    q, r = ya.OrdFilt(n, k), ofr.OrdFilt(n, k)
    for part in (x[:nb], x[nb:]):                                 # the second call reads the history of the first
        ax = Arena(ya, np.float32, nb, off=off, guard=GUARD).load(part)
        ay = Arena(ya, np.float32, nb, off=(off + 2) % 4, guard=GUARD)
        q.execute_block_devptr(ax.ptr, nb, ay.ptr)
        got = ay.fetch_output()
        ax.assert_input_intact(part)
        assert got.tobytes() == r.execute_block(part).tobytes(), (n, nb, off)
        ax.free()
        ay.free()
