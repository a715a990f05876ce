"""Every `_dev` entry point of Modem on tests/dev_arena.py arenas, as tests/test_gpu_dev_buffers.py does for the older
objects: each operand sits at an offset inside a guarded allocation filled with 0xFF, the inputs are intact afterwards,
every output element is written and nothing is written outside [0, n) / [0, n * bps).

The byte operands (symbols, soft bits) are carved out of uint32 arenas at a BYTE offset, so the sentinel check is made
here on bytes: 0xFF is no symbol of the schemes used (M <= 64); soft bytes may be 255, so an unwritten soft byte shows
as a mismatch with the expected value instead."""
import numpy as np
import pytest

import modem_ref as mr
from dev_arena import Arena

pytestmark = pytest.mark.gpu
TD, TM = 2048, 4096


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


class ByteArena:
    """n bytes `off` bytes behind an Arena's operand start"""

    def __init__(self, ya, n, off):
        self.n, self.off = n, off
        self.a = Arena(ya, np.uint32, (n + off + 3) // 4 + 1, off=1)
        self.ptr = self.a.ptr + off
        self.lo = self.a.first * 4 + off

    def load(self, host):
        host = np.ascontiguousarray(host, np.uint8)
        assert host.size == self.n
        raw = self.a.dev.to_numpy().view(np.uint8).copy()
        raw[self.lo:self.lo + self.n] = host
        rc = self.a.ya.lib.yagi_hip_memcpy_h2d(self.a.dev.ptr, raw.ctypes.data, raw.nbytes)
        assert rc == 0
        return self

    def fetch(self, written=True, sentinel_free=True):
        self.a.ya.synchronize()
        raw = self.a.dev.to_numpy().view(np.uint8)
        assert np.all(raw[:self.lo] == 0xFF), "wrote in front of the operand"
        assert np.all(raw[self.lo + self.n:] == 0xFF), "wrote behind the operand"
        y = raw[self.lo:self.lo + self.n].copy()
        if written and sentinel_free:
            assert not np.any(y == 0xFF), "an output byte was never written"
        return y


CASES = [("Qam16", 17, 1), ("Qam8", TD + 1, 3), ("Ask4", 3 * TD + 17, 2), ("Psk8", TD - 1, 1), ("Dpsk4", 2 * TD + 5, 3),
         ("Bpsk", 33, 1), ("Qam64", TD, 0)]


def _inputs(D, n, seed):
    rng = np.random.default_rng(seed)
    if D.kind in (mr.PSK, mr.DPSK):
        half = np.pi / D.M
        ph = (2 * rng.integers(0, D.M, n) + 1) * half + rng.uniform(1e-3, half - 1e-3, n)
        ph = np.cumsum(ph) if D.kind == mr.DPSK else ph
        return np.exp(1j * ph).astype(np.complex64)
    return (D.map[rng.integers(0, D.M, n)] + 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


@pytest.mark.parametrize("name,n,off", CASES)
def test_demodulate_dev_on_arenas(ya, name, n, off):
    m = ya.Modem(ya.ModulationScheme[name])
    D = mr.design(*mr.SCHEMES[name])
    cmap, nbr = m.get_constellation(), m.get_neighbours()
    x = _inputs(D, n, n)
    want_s, want_xh, want_sb, _ = mr.block_demod(D, cmap, nbr, x, np.float32(0), True)
    ax = Arena(ya, np.complex64, n, off=off).load(x)
    asym = ByteArena(ya, n, off)
    axh = Arena(ya, np.complex64, n, off=off + 1)
    m.demodulate_block_devptr(ax.ptr, n, asym.ptr, axh.ptr)
    assert np.array_equal(asym.fetch(), want_s)
    xh = axh.fetch_output()
    if D.kind != mr.DPSK:
        assert np.array_equal(xh.view(np.uint32), want_xh.view(np.uint32))
    ax.assert_input_intact(x)
    m.reset()
    asym2 = ByteArena(ya, n, (off + 2) % 4)
    asoft = ByteArena(ya, n * D.bps, off)
    m.demodulate_soft_block_devptr(ax.ptr, n, asym2.ptr, asoft.ptr)
    assert np.array_equal(asym2.fetch(), want_s)
    assert np.array_equal(asoft.fetch(sentinel_free=False).reshape(n, D.bps), want_sb)
    ax.assert_input_intact(x)
    m.reset()                                                     # without the optional output
    asym3 = ByteArena(ya, n, off)
    m.demodulate_block_devptr(ax.ptr, n, asym3.ptr, None)
    assert np.array_equal(asym3.fetch(), want_s)


@pytest.mark.parametrize("name,n,off", [("Qam16", 17, 1), ("Psk8", TM + 1, 3), ("Dpsk4", 3 * TM + 17, 2), ("Dpsk8", TM, 1),
                                        ("Ask4", TM - 1, 0)])
def test_modulate_dev_on_arenas(ya, name, n, off):
    m = ya.Modem(ya.ModulationScheme[name])
    D = mr.design(*mr.SCHEMES[name])
    cmap = m.get_constellation()
    sym = np.random.default_rng(n).integers(0, D.M, n).astype(np.uint8)
    k = mr.dpsk_indices(sym, D.M) if D.kind == mr.DPSK else sym
    asym = ByteArena(ya, n, off).load(sym)
    ay = Arena(ya, np.complex64, n, off=off)
    m.modulate_block_devptr(asym.ptr, n, ay.ptr)
    assert np.array_equal(ay.fetch_output().view(np.uint32), cmap[k].view(np.uint32))
    assert np.array_equal(asym.fetch(sentinel_free=False), sym)
    # a rejected block leaves the whole output arena untouched
    bad = sym.copy()
    bad[n // 2] = D.M
    abad = ByteArena(ya, n, off).load(bad)
    ay2 = Arena(ya, np.complex64, n, off=off)
    with pytest.raises(ya.RangeError):
        m.modulate_block_devptr(abad.ptr, n, ay2.ptr)
    ya.synchronize()
    assert np.all(ay2.dev.to_numpy().view(np.uint32) == 0xFFFFFFFF)


def test_overlapping_operands_are_config_errors(ya):
    m = ya.Modem(ya.ModulationScheme.Qam16)
    buf = ya.DeviceArray(4096, np.complex64)
    with pytest.raises(ya.ConfigError):
        m.demodulate_block_devptr(buf.ptr, 64, buf.ptr + 8, None)
    with pytest.raises(ya.ConfigError):
        m.demodulate_soft_block_devptr(buf.ptr, 64, buf.ptr + 4096, buf.ptr + 4100)
    with pytest.raises(ya.ConfigError):
        m.modulate_block_devptr(buf.ptr + 16, 64, buf.ptr)
