"""tests/firhilb_ref.py (the restatement the GPU tests compare FirHilbertFilter against bit for bit) pinned to the
reference's own tests (src/filter/fir/firhilb.rs:265-460) at their tolerances, its closed form pinned to its per-sample
loop bit for bit, and the library's host design code pinned to it.  Runs without a GPU."""
import numpy as np
import pytest

from conftest import has_gpu
from firhilb_ref import C2R, DECIM, INTERP, MODES, R2C, FirHilbRef, block, design, f32, same_bits
from psd_util import validate_psd_signal

DECIM_X = [1.0000, 0.7071, 0.0000, -0.7071, -1.0000, -0.7071, -0.0000, 0.7071,
           1.0000, 0.7071, 0.0000, -0.7071, -1.0000, -0.7071, -0.0000, 0.7071,
           1.0000, 0.7071, 0.0000, -0.7071, -1.0000, -0.7071, -0.0000, 0.7071,
           1.0000, 0.7071, -0.0000, -0.7071, -1.0000, -0.7071, -0.0000, 0.7071]
DECIM_Y = [(0.0000, -0.0055), (-0.0000, 0.0231), (0.0000, -0.0605), (-0.0000, 0.1459),
           (0.0000, -0.5604), (-0.7071, -0.7669), (-0.7071, 0.7294), (0.7071, 0.7008),
           (0.7071, -0.7064), (-0.7071, -0.7064), (-0.7071, 0.7064), (0.7071, 0.7064),
           (0.7071, -0.7064), (-0.7071, -0.7064), (-0.7071, 0.7064), (0.7071, 0.7064)]
INTERP_X = [(1.0, 0.0), (-0.0, -1.0), (-1.0, 0.0), (0.0, 1.0), (1.0, -0.0), (-0.0, -1.0), (-1.0, 0.0), (0.0, 1.0),
            (1.0, -0.0), (-0.0, -1.0), (-1.0, 0.0), (0.0, 1.0), (1.0, -0.0), (0.0, -1.0), (-1.0, 0.0), (0.0, 1.0)]
INTERP_Y = [0.0000, -0.0055, -0.0000, -0.0231, -0.0000, -0.0605, -0.0000, -0.1459,
            -0.0000, -0.5604, -0.0000, 0.7669, 1.0000, 0.7294, 0.0000, -0.7008,
            -1.0000, -0.7064, -0.0000, 0.7064, 1.0000, 0.7064, 0.0000, -0.7064,
            -1.0000, -0.7064, -0.0000, 0.7064, 1.0000, 0.7064, 0.0000, -0.7064]
TOL = 0.005


def _c(pairs):
    return np.array([complex(a, b) for a, b in pairs], np.complex64)


@pytest.fixture(scope="module")
def taps(oracle):
    cache = {}

    def get(m, as_=60.0):
        if (m, as_) not in cache:
            cache[(m, as_)] = design(m, as_, oracle.fir_design_kaiser)
        return cache[(m, as_)]
    return get


def test_firhilbf_decim(taps):                                # firhilb.rs:272-304
    q = FirHilbRef(taps(5))
    x = np.array(DECIM_X, f32)
    y = np.array([complex(*q.decim_execute(x[2 * i: 2 * i + 2])) for i in range(16)])
    t = _c(DECIM_Y)
    assert np.max(np.abs(y.real - t.real)) < TOL and np.max(np.abs(y.imag - t.imag)) < TOL


def test_firhilbf_interp(taps):                               # firhilb.rs:306-337
    q = FirHilbRef(taps(5))
    y = np.array([q.interp_execute(v) for v in _c(INTERP_X)], f32).reshape(-1)
    assert np.max(np.abs(y - np.array(INTERP_Y, f32))) < TOL


def psd_buffers(oracle, run_interp, reset, run_decim):
    """test_firhilbf_psd (firhilb.rs:339-394): the pulse, its interpolation, and the decimation of that"""
    bw, p, m = 0.4, 40, 25
    h_len = 2 * p + 1
    num = h_len + 2 * m + 8
    w = f32(0.36) * f32(bw)
    h = oracle.fir_design_kaiser(h_len, float(w), 80.0, 0.0)
    buf0 = np.zeros(num, np.complex64)
    buf0[:h_len] = (f32(2.0) * w * h).astype(f32)
    buf1 = run_interp(buf0)
    reset()
    buf2 = run_decim(buf1)
    return buf0, buf1, buf2


def psd_check(buf0, buf1, buf2, as_=60.0, tol=1.0, bw=0.4):
    orig = [(-0.5, -0.5 * bw, 0.0, -as_ + tol, False, True), (-0.3 * bw, 0.3 * bw, -1.0, 1.0, True, True),
            (0.5 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    interp = [(-0.5, -0.25 - 0.25 * bw, 0.0, -as_ + tol, False, True),
              (-0.25 - 0.15 * bw, -0.25 + 0.15 * bw, -1.0, 1.0, True, True),
              (-0.25 + 0.25 * bw, 0.25 - 0.25 * bw, 0.0, -as_ + tol, False, True),
              (0.25 - 0.15 * bw, 0.25 + 0.15 * bw, -1.0, 1.0, True, True),
              (0.25 + 0.25 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    for buf, regions in ((buf0, orig), (buf1.astype(np.complex64), interp), (buf2, orig)):
        ok, worst = validate_psd_signal(buf, regions)
        assert ok, worst


def test_firhilbf_psd(oracle, taps):
    q = FirHilbRef(taps(25))
    psd_check(*psd_buffers(oracle, lambda b: q.run(INTERP, b), q.reset, lambda b: q.run(DECIM, b)))


def test_invalid_config(oracle):                              # firhilb.rs:396-406
    import yagi_amd
    for m in (0, 1):
        with pytest.raises(ValueError):
            design(m, 60.0, oracle.fir_design_kaiser)
        with pytest.raises(yagi_amd.ConfigError):
            yagi_amd.firhilb_design(m, 60.0)


def _copy_case(taps, mode):                                   # firhilb.rs:408-459
    rng = np.random.default_rng(7)
    q0 = FirHilbRef(taps(12, 120.0))
    for _ in range(80):
        if mode == INTERP:
            q0.interp_execute(complex(*rng.standard_normal(2)))
        else:
            q0.decim_execute(rng.standard_normal(2).astype(f32))
    q1 = q0.clone()
    for _ in range(80):
        if mode == INTERP:
            x = complex(*rng.standard_normal(2))
            a, b = q0.interp_execute(x), q1.interp_execute(x)
        else:
            x = rng.standard_normal(2).astype(f32)
            a, b = q0.decim_execute(x), q1.decim_execute(x)
        assert a == b


def test_copy_interp(taps):
    _copy_case(taps, INTERP)


def test_copy_decim(taps):
    _copy_case(taps, DECIM)


def rand_input(rng, mode, n):
    """random f32 data with +-0 and subnormals mixed in, in the mode's input layout (n units)"""
    nf = n if mode == R2C else 2 * n
    v = rng.standard_normal(nf).astype(f32)
    k = rng.integers(0, 8, nf)
    v[k == 0] = f32(0.0)
    v[k == 1] = f32(-0.0)
    v[k == 2] = (rng.standard_normal(int((k == 2).sum())) * 1e-39).astype(f32)
    return v if mode in (R2C, DECIM) else v.view(np.complex64)


def units(mode, x):
    return len(x) // 2 if mode == DECIM else len(x)


@pytest.mark.parametrize("m", [2, 3, 5, 12, 25])
@pytest.mark.parametrize("mode", MODES)
def test_closed_form_equals_loop(taps, mode, m):
    rng = np.random.default_rng(100 + m)
    q = FirHilbRef(taps(m))
    st = q.state()
    for n in (0, 1, 3, 0, 7, 1, 2, 13, 64, 5, 1, 31):
        x = rand_input(rng, mode, n)
        y_ref = q.run(mode, x)
        y, st = block(mode, q.hq, st, x)
        assert same_bits(y, y_ref), (mode, m, n)
        assert same_bits(st[0], q.w) and st[1] == q.toggle, (mode, m, n)


@pytest.mark.parametrize("m", [2, 5, 12])
def test_closed_form_mixed_modes(taps, m):
    rng = np.random.default_rng(200 + m)
    q = FirHilbRef(taps(m))
    st = q.state()
    for _ in range(40):
        mode = MODES[rng.integers(0, 4)]
        n = int(rng.choice([0, 1, 2, 3, 5, 8, 17]))
        x = rand_input(rng, mode, n)
        y_ref = q.run(mode, x)
        y, st = block(mode, q.hq, st, x)
        assert same_bits(y, y_ref), (mode, m, n)
        assert same_bits(st[0], q.w) and st[1] == q.toggle


def test_library_design_matches_restatement(oracle):
    import yagi_amd
    for m, as_ in [(2, 60.0), (5, 60.0), (12, 120.0), (25, 60.0), (64, 80.0), (7, -60.0), (600, 60.0)]:
        a = yagi_amd.firhilb_design(m, as_)
        b = design(m, as_, oracle.fir_design_kaiser)
        assert a.shape == (2 * m,)
        np.testing.assert_allclose(a, b, rtol=2e-6, atol=1e-9)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_no_device_gives_device_error():
    import yagi_amd
    with pytest.raises(yagi_amd.DeviceError):
        yagi_amd.FirHilbertFilter(12, 60.0)
