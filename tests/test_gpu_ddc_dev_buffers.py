"""The execute_block_dev forms of Ddc and Duc on tests/dev_arena.py arenas, as tests/test_gpu_sequence_dev_buffers.py does
for the sequences: every operand sits at an offset inside a guarded allocation filled with 0xFF (NaN); afterwards the
input is intact, every output element is written and finite, the guards are untouched, the result equals the
composition Osc + FirDecimationFilter / FirInterpolationFilter + Osc, and a second call reads the state the first one
left.  At element offset 1 and 3 the buffers are 8- but not 16-byte aligned."""
import numpy as np
import pytest

from dev_arena import GUARD_MIN, Arena
from gpu_util import rand_samples, rand_taps
from test_gpu_ddc import DdcParts, DucParts, same_words, tune

pytestmark = pytest.mark.gpu
GUARD = max(GUARD_MIN, 2 * 2048 * 16)              # elements: more than two of the widest tile's input span (M = 16)


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("scheme", [0, 1], ids=["nco", "vco"])
@pytest.mark.parametrize("choice", [2, 1], ids=["fused", "two-launch"])
@pytest.mark.parametrize("kind,M,L", [("crcf", 2, 65), ("cccf", 8, 129), ("crcf", 3, 64), ("cccf", 16, 33)])
def test_ddc_dev_on_arenas(ya, kind, M, L, choice, scheme, off):
    """2049 + 1 outputs then 700: interior tiles (descriptor staging), a ragged last tile, a call below the 512-output
    threshold of the register-window kernels"""
    rng = np.random.default_rng(5000 + 31 * M + L + off)
    h = rand_taps(rng, kind, L)
    q, ref = ya.Ddc(kind, scheme, M, h), DdcParts(ya, kind, scheme, M, h, 0.5)
    q.set_scale(0.5)
    q.set_kernel(choice)
    tune(q, "ordinary")
    tune(ref.osc, "ordinary")
    for n in (2050, 700, 100):
        x = rand_samples(rng, "crcf", n * M)
        ax = Arena(ya, np.complex64, n * M, off=off, guard=GUARD).load(x)
        ay = Arena(ya, np.complex64, n, off=(off + 1) % 4, guard=GUARD)
        q.execute_block_devptr(ax.ptr, n, ay.ptr)
        got = ay.fetch_output()
        ax.assert_input_intact(x)
        assert q.get_last_kernel() == choice
        assert same_words(got, ref.execute_block(x, n)), (n, off)
        assert q.get_state() == ref.osc.get_state()
        ax.free()
        ay.free()


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("scheme", [0, 1], ids=["nco", "vco"])
@pytest.mark.parametrize("choice", [2, 1], ids=["fused", "two-launch"])
@pytest.mark.parametrize("kind,interp,hl", [("crcf", 2, 9), ("cccf", 5, 101), ("crcf", 16, 33), ("cccf", 20, 100)])
def test_duc_dev_on_arenas(ya, kind, interp, hl, choice, scheme, off):
    rng = np.random.default_rng(5100 + 31 * interp + hl + off)
    h = rand_taps(rng, kind, hl)
    q, ref = ya.Duc(kind, scheme, interp, h), DucParts(ya, kind, scheme, interp, h, 0.5)
    q.set_scale(0.5)
    q.set_kernel(choice)
    tune(q, "ordinary")
    tune(ref.osc, "ordinary")
    for n in (513, 300, 1):
        x = rand_samples(rng, "crcf", n)
        ax = Arena(ya, np.complex64, n, off=off, guard=GUARD).load(x)
        ay = Arena(ya, np.complex64, n * interp, off=(off + 1) % 4, guard=GUARD)
        q.execute_block_devptr(ax.ptr, n, ay.ptr)
        got = ay.fetch_output()
        ax.assert_input_intact(x)
        assert q.get_last_kernel() == choice
        assert same_words(got, ref.execute_block(x)), (n, off)
        assert q.get_state() == ref.osc.get_state()
        ax.free()
        ay.free()


def test_overlapping_operands_are_config_errors(ya):
    h = np.ones(8, np.float32)
    buf = ya.DeviceArray(4096, np.complex64)
    with pytest.raises(ya.ConfigError, match="overlap"):
        ya.Ddc("crcf", 0, 4, h).execute_block_devptr(buf, 64, buf.ptr + 8 * 255)
    with pytest.raises(ya.ConfigError, match="overlap"):
        ya.Duc("crcf", 0, 4, h).execute_block_devptr(buf.ptr + 8 * 255, 64, buf)
