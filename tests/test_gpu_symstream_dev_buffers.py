"""The device-pointer forms of SymStream on tests/dev_arena.py arenas, as tests/test_gpu_ddc_dev_buffers.py does for Ddc
and Duc: every operand sits at an offset inside a guarded allocation filled with 0xFF (NaN); afterwards the guards are
untouched, the input is intact, every output word is written and finite, the result equals the composition of
tests/symstream_ref.py byte for byte, and a second call starts inside the symbol the first one ended in.  At element
offsets 1 and 3 the sample buffers are 8- but not 16-byte aligned; the symbol bytes sit at byte offsets 0, 1 and 3."""
import numpy as np
import pytest

from dev_arena import GUARD_MIN, Arena
from test_gpu_sequence_dev_buffers import ByteArena
from test_gpu_symstream import make, same

pytestmark = pytest.mark.gpu
GUARD = max(GUARD_MIN, 2 * 256 * 64)               # elements: more than two of the widest tile's outputs (k = 64)
SHAPES = [(2, 7, "Qpsk"), (5, 17, "Qam64"), (17, 3, "Psk8"), (64, 100, "Qam16"), (5, 17, "Dpsk4")]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("k,m,scheme", SHAPES)
def test_write_samples_devptr_on_arenas(ya, k, m, scheme, off):
    q, ref, _ = make(ya, k, m, ya.ModulationScheme[scheme], 300 + off)
    assert q.is_fused() == (scheme != "Dpsk4")
    for n in (257 * k + k // 2 + 1, 300 * k - 1, 1, 2 * k):        # the second call starts inside a symbol
        ay = Arena(ya, np.complex64, n, off=off, guard=GUARD)
        q.write_samples_devptr(ay.ptr, n)
        assert same(ay.fetch_output(), ref.write_samples(n)), (n, off)
        assert q.get_buf_index() == ref.p
        ay.free()


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("k,m,scheme", SHAPES)
def test_modulate_symbols_devptr_on_arenas(ya, k, m, scheme, off):
    q, ref, _ = make(ya, k, m, ya.ModulationScheme[scheme], 400 + off)
    M = 1 << ya.Modem(ya.ModulationScheme[scheme]).get_bps()
    rng = np.random.default_rng(410 + off)
    for nsym in (515, 64, 1):
        sym = rng.integers(0, M, nsym).astype(np.uint8)
        ax = ByteArena(ya, nsym, off).load(sym)
        ay = Arena(ya, np.complex64, nsym * k, off=(off + 1) % 4, guard=GUARD)
        q.modulate_symbols_devptr(ax.ptr, nsym, ay.ptr)
        assert same(ay.fetch_output(), ref.modulate_symbols(sym)), (nsym, off)
        assert np.array_equal(ax.fetch(sentinel_free=False), sym)
        if M < 256:                                               # a symbol >= M: nothing is written, no state moves
            bad = sym.copy()
            bad[nsym // 2] = M
            ab = ByteArena(ya, nsym, off).load(bad)
            an = Arena(ya, np.complex64, nsym * k, off=off, guard=GUARD)
            with pytest.raises(ya.RangeError):
                q.modulate_symbols_devptr(ab.ptr, nsym, an.ptr)
            ya.synchronize()
            assert np.all(an.dev.to_numpy().view(np.uint32) == 0xFFFFFFFF)
            ab.free()
            an.free()
        ax.free()
        ay.free()
    n = 3 * k + 1                                                 # the streams still agree, and mix with the source
    ay = Arena(ya, np.complex64, n, off=off, guard=GUARD)
    q.write_samples_devptr(ay.ptr, n)
    assert same(ay.fetch_output(), ref.write_samples(n))
    with pytest.raises(ya.ModeError):
        q.modulate_symbols_devptr(ay.ptr, 1, ay.ptr + 64)
    ay.free()


def test_overlapping_operands_are_config_errors(ya):
    q, _, _ = make(ya, 4, 5, ya.ModulationScheme.Qpsk, 500)
    buf = ya.DeviceArray(4096, np.complex64)
    with pytest.raises(ya.ConfigError, match="overlap"):
        q.modulate_symbols_devptr(buf.ptr + 100, 64, buf)
    with pytest.raises(ya.ConfigError, match="overlap"):
        q.modulate_symbols_devptr(buf, 64, buf.ptr + 8)
