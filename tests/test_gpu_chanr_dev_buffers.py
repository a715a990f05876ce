"""The analyzer_execute_devptr and synthesizer_execute_devptr forms of FirPfbChr on tests/dev_arena.py arenas, as
tests/test_gpu_ddc_dev_buffers.py does for Ddc and Duc: every operand sits at an offset inside a guarded allocation
filled with 0xFF (NaN); afterwards the input is intact, every output element is written and finite, the guards are
untouched, the result equals the host-pointer form's word for word, and a second call reads the state the first one left.
At element offset 1 and 3 the buffers are 8- but not 16-byte aligned.  Both analyzer kernels."""
import numpy as np
import pytest

from dev_arena import GUARD_MIN, Arena
from gpu_util import rand_samples

pytestmark = pytest.mark.gpu
GUARD = max(GUARD_MIN, 2 * 16 * 256)               # elements: two of the column kernel's widest windows (16 taps, M = 256)


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


def _same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint32), np.ascontiguousarray(b).reshape(-1).view(np.uint32))


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("M,P,m,choice", [(64, 48, 4, 2), (64, 48, 4, 1), (256, 192, 5, 2), (128, 80, 2, 2), (10, 7, 3, 1),
                                          (512, 384, 2, 1)])
def test_analyzer_dev_on_arenas(ya, M, P, m, choice, off):
    """65 steps (a partial last workgroup of the column kernel), then 67 from an odd step, then 1"""
    rng = np.random.default_rng(8000 + M + P + off)
    h = rng.standard_normal(2 * M * m).astype(np.float32)
    q, ref = ya.FirPfbChr(M, P, m, h), ya.FirPfbChr(M, P, m, h)
    q.set_kernel(choice)
    ref.set_kernel(choice)
    for n in (65, 67, 1):
        x = rand_samples(rng, "crcf", n * P)
        ax = Arena(ya, np.complex64, n * P, off=off, guard=GUARD).load(x)
        ay = Arena(ya, np.complex64, n * M, off=(off + 1) % 4, guard=GUARD)
        q.analyzer_execute_devptr(ax.ptr, n, ay.ptr)
        got = ay.fetch_output()
        ax.assert_input_intact(x)
        assert q.get_last_kernel() == choice
        assert _same_words(got, ref.analyzer_execute(x)), (n, off)
        ax.free()
        ay.free()


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("M,P,m", [(64, 48, 4), (10, 7, 3), (256, 192, 2), (6, 1, 2)])
def test_synthesizer_dev_on_arenas(ya, M, P, m, off):
    rng = np.random.default_rng(8100 + M + P + off)
    h = rng.standard_normal(2 * M * m).astype(np.float32)
    q, ref = ya.FirPfbChr(M, P, m, h), ya.FirPfbChr(M, P, m, h)
    for n in (65, 67, 1):
        X = rand_samples(rng, "crcf", n * M)
        ax = Arena(ya, np.complex64, n * M, off=off, guard=GUARD).load(X)
        ay = Arena(ya, np.complex64, n * P, off=(off + 1) % 4, guard=GUARD)
        q.synthesizer_execute_devptr(ax.ptr, n, ay.ptr)
        got = ay.fetch_output()
        ax.assert_input_intact(X)
        assert _same_words(got, ref.synthesizer_execute(X)), (n, off)
        ax.free()
        ay.free()


def test_overlapping_operands_are_config_errors(ya):
    h = np.ones(2 * 8 * 2, np.float32)
    buf = ya.DeviceArray(4096, np.complex64)
    with pytest.raises(ya.ConfigError, match="overlap"):
        ya.FirPfbChr(8, 6, 2, h).analyzer_execute_devptr(buf, 64, buf.ptr + 8 * 383)
    with pytest.raises(ya.ConfigError, match="overlap"):
        ya.FirPfbChr(8, 6, 2, h).synthesizer_execute_devptr(buf.ptr + 8 * 383, 64, buf)
