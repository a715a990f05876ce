"""write_samples_devptr of SymStreamR on tests/dev_arena.py arenas, as tests/test_gpu_symstream_dev_buffers.py does for
SymStream: the output sits at an offset inside a guarded allocation filled with 0xFF (NaN); afterwards the guards are
untouched (nothing outside [y, y + n) is written), every output word is written and finite, and the result equals the
composition of tests/symstreamr_ref.py byte for byte.  At element offsets 1 and 3 the buffer is 8- but not 16-byte
aligned.  The calls include one that the leftover alone serves (no kernel runs) and run at zero, four, five and eight
half-band stages and on the composition route (Dpsk4)."""
import numpy as np
import pytest

from dev_arena import GUARD_MIN, Arena
from test_gpu_symstreamr import make, same

pytestmark = pytest.mark.gpu
GUARD = max(GUARD_MIN, 2 * 1024)                    # elements: more than a tile of the fused kernel's outputs
SHAPES = [(0.77, None), (0.4, None), (0.03, None), (0.01, None), (0.001, None), (0.2, "Dpsk4")]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("bw,scheme", SHAPES)
def test_write_samples_devptr_on_arenas(ya, bw, scheme, off):
    q, ref, _ = make(ya, bw, seed=300 + off, scheme=None if scheme is None else ya.ModulationScheme[scheme])
    g = 1 << q.get_params()[1]
    assert q.is_fused() == (scheme is None)
    for n in (1, 1025 * g + g // 2 + 1, 0, 2 * g + 1, 777):
        if n == 0:                                  # a call that the leftover alone serves
            n = q.get_pending()
            if n == 0:
                continue
            state = q.source_get_state()
        else:
            state = None
        ay = Arena(ya, np.complex64, n, off=off, guard=GUARD)
        q.write_samples_devptr(ay.ptr, n)
        assert same(ay.fetch_output(), ref.write_samples(n)), (bw, n, off)
        assert q.get_pending() == ref.fifo.size
        assert state is None or (q.source_get_state() == state and q.get_pending() == 0)
        ay.free()


def test_misaligned_output_is_a_config_error(ya):
    q, _, _ = make(ya, 0.4)
    buf = ya.DeviceArray(64, np.complex64)
    with pytest.raises(ya.ConfigError, match="aligned"):
        q.write_samples_devptr(buf.ptr + 4, 8)
