"""FirHilbertFilter on the device (firhilb_kernels.hip) against tests/firhilb_ref.py, with the object's own taps
(firhilb_design): the reference's known-answer and spectral tests through every form of call, and every output word of
the block forms bit for bit, on any length, cut and mix of calls and modes."""
import numpy as np
import pytest

from firhilb_ref import C2R, DECIM, INTERP, MODES, R2C, FirHilbRef, block, f32, same_bits
from test_firhilb_ref_cpu import (DECIM_X, DECIM_Y, INTERP_X, INTERP_Y, TOL, _c, psd_buffers, psd_check, rand_input,
                                  units)

pytestmark = pytest.mark.gpu

FAST_M_LIMIT = 512                      # kFirhilbFastM: above it the general kernel runs


def ya():
    import yagi_amd
    return yagi_amd


def in_dtype(mode):
    return np.float32 if mode in (R2C, DECIM) else np.complex64


def out_len(mode, n):                   # elements of the output array for n units
    return n if mode in (R2C, DECIM) else 2 * n


def out_dtype(mode):
    return np.complex64 if mode in (R2C, DECIM) else np.float32


def run_dev(q, mode, x, offset=0):
    """one device block call; offset > 0 places x and y that many floats past an allocation's start"""
    Y = ya()
    n = units(mode, x)
    xf = np.ascontiguousarray(x).view(np.float32)
    yf_len = 2 * n
    xd = Y.DeviceArray(xf.size + offset + 1, np.float32)
    yd = Y.DeviceArray(yf_len + offset + 1, np.float32)
    if xf.size:
        buf = np.zeros(xf.size + offset + 1, np.float32)
        buf[offset: offset + xf.size] = xf
        xd = Y.DeviceArray.from_numpy(buf)
    getattr(q, mode + "_execute_block_dev")(xd.ptr + 4 * offset, n, yd.ptr + 4 * offset)
    Y.synchronize()
    y = yd.to_numpy(yf_len, offset) if yf_len else np.zeros(0, np.float32)
    return y.view(out_dtype(mode))


def run_host(q, mode, x):
    return getattr(q, mode + "_execute_block")(x)


def run_single(q, mode, x):
    if mode == R2C:
        return np.array([q.r2c_execute(v) for v in x], np.complex64)
    if mode == DECIM:
        return np.array([q.decim_execute(x[2 * i: 2 * i + 2]) for i in range(len(x) // 2)], np.complex64)
    if mode == C2R:
        return np.array([q.c2r_execute(v) for v in x], np.float32).reshape(-1)
    return np.concatenate([q.interp_execute(v) for v in x] or [np.zeros(0, np.float32)])


RUN = {"single": run_single, "host": run_host, "dev": run_dev}


@pytest.mark.parametrize("path", ["single", "host", "dev"])
def test_kats_and_psd(oracle, path):                          # firhilb.rs:272-394
    Y = ya()
    run = RUN[path]
    q = Y.FirHilbertFilter(5, 60.0)
    y = run(q, DECIM, np.array(DECIM_X, f32))
    t = _c(DECIM_Y)
    assert np.max(np.abs(y.real - t.real)) < TOL and np.max(np.abs(y.imag - t.imag)) < TOL
    q = Y.FirHilbertFilter(5, 60.0)
    y = run(q, INTERP, _c(INTERP_X))
    assert np.max(np.abs(y - np.array(INTERP_Y, f32))) < TOL
    q = Y.FirHilbertFilter(25, 60.0)
    psd_check(*psd_buffers(oracle, lambda b: run(q, INTERP, b), q.reset, lambda b: run(q, DECIM, b)))


LENGTHS = [0, 1, 2, 3, 4095, 4096, 4097, (1 << 20) + 3]


@pytest.mark.parametrize("m", [2, 5, 12, 25, 64, FAST_M_LIMIT + 1])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", ["host", "dev"])
def test_block_bitwise(mode, m, path):
    Y = ya()
    rng = np.random.default_rng(1000 + 7 * m + MODES.index(mode))
    q = Y.FirHilbertFilter(m, 60.0)
    hq = Y.firhilb_design(m, 60.0)
    st = FirHilbRef(hq).state()
    for n in LENGTHS:
        x = rand_input(rng, mode, n)
        y = RUN[path](q, mode, x)
        y_ref, st = block(mode, hq, st, x)
        assert same_bits(y, y_ref), (mode, m, path, n)


@pytest.mark.parametrize("mode", MODES)
def test_big_block(mode):
    Y = ya()
    m, n = 12, (1 << 24) + 1
    rng = np.random.default_rng(5)
    q = Y.FirHilbertFilter(m, 60.0)
    hq = Y.firhilb_design(m, 60.0)
    st = FirHilbRef(hq).state()
    x0 = rand_input(rng, mode, 3)                 # start from a state with the toggle set
    y, st = block(mode, hq, st, x0)
    assert same_bits(run_dev(q, mode, x0), y)
    x = rand_input(rng, mode, n)
    y_ref, st = block(mode, hq, st, x)
    assert same_bits(run_dev(q, mode, x), y_ref)


@pytest.mark.parametrize("mode", MODES)
def test_odd_cuts_offset_buffers(mode):
    Y = ya()
    m = 12
    rng = np.random.default_rng(77)
    q = Y.FirHilbertFilter(m, 60.0)
    hq = Y.firhilb_design(m, 60.0)
    st = FirHilbRef(hq).state()
    cuts = [1, 3, 5, 0, 7, 4095, 4097, 1, 9, 2049, 33, 1, 65537, 3, 8191, 11, 1, 5, 12289, 7, 1, 31]
    for n in cuts:
        x = rand_input(rng, mode, n)
        y_ref, st = block(mode, hq, st, x)
        assert same_bits(run_dev(q, mode, x, offset=1), y_ref), (mode, n)


def test_mixed_sequence():
    """per-sample, host-block and device-block calls of all four modes on one object: the shared windows and toggle"""
    Y = ya()
    m = 5
    rng = np.random.default_rng(9)
    q = Y.FirHilbertFilter(m, 60.0)
    hq = Y.firhilb_design(m, 60.0)
    ref = FirHilbRef(hq)
    for c in range(240):
        mode = MODES[rng.integers(0, 4)]
        path = ["single", "host", "dev"][rng.integers(0, 3)]
        n = int(rng.choice([1, 2, 3, 5, 16, 37, 129, 4097, 5003])) if path != "single" else int(rng.integers(1, 4))
        x = rand_input(rng, mode, n)
        y_ref, st = block(mode, hq, ref.state(), x)
        ref.w, ref.toggle = st
        assert same_bits(RUN[path](q, mode, x), y_ref), (c, mode, path, n)


def test_clone_and_reset():
    Y = ya()
    m = 12
    rng = np.random.default_rng(3)
    q = Y.FirHilbertFilter(m, 120.0)
    hq = Y.firhilb_design(m, 120.0)
    st = FirHilbRef(hq).state()
    for mode, n in ((R2C, 5001), (DECIM, 77), (C2R, 4099)):
        x = rand_input(rng, mode, n)
        run_dev(q, mode, x)
        _, st = block(mode, hq, st, x)
    q1 = q.clone()
    for mode, n in ((INTERP, 3), (R2C, 6000), (DECIM, 1), (C2R, 9)):
        x = rand_input(rng, mode, n)
        a = run_dev(q, mode, x) if n > 100 else run_single(q, mode, x)
        b = run_dev(q1, mode, x) if n > 100 else run_single(q1, mode, x)
        y_ref, st = block(mode, hq, st, x)
        assert same_bits(a, y_ref) and same_bits(b, y_ref), (mode, n)
    x = rand_input(rng, DECIM, 4500)
    y0 = run_dev(q, DECIM, x)
    q.reset()
    q1.reset()
    fresh = FirHilbRef(hq).state()
    y_ref, _ = block(DECIM, hq, fresh, x)
    assert same_bits(run_dev(q, DECIM, x), y_ref)
    assert same_bits(run_host(q1, DECIM, x), y_ref)
    assert not same_bits(y0, y_ref)


@pytest.mark.parametrize("mode", MODES)
def test_nonfinite_inputs(mode):
    Y = ya()
    m = 12
    rng = np.random.default_rng(11)
    q = Y.FirHilbertFilter(m, 60.0)
    hq = Y.firhilb_design(m, 60.0)
    st = FirHilbRef(hq).state()
    x = rand_input(rng, mode, 20000)
    xf = x.view(np.float32)
    for i, v in zip(rng.integers(0, xf.size, 6), (np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf)):
        xf[i] = v
    y = run_dev(q, mode, x)
    y_ref, _ = block(mode, hq, st, x)
    yf, rf = y.view(np.float32), y_ref.view(np.float32)
    assert not np.isfinite(rf).all()
    assert np.array_equal(np.isfinite(yf), np.isfinite(rf))
    assert np.array_equal(np.isnan(yf), np.isnan(rf))
    fin = np.isfinite(rf)
    assert same_bits(yf[fin], rf[fin])


def test_errors():
    Y = ya()
    q = Y.FirHilbertFilter(5, 60.0)
    with pytest.raises(Y.RangeError):
        q.decim_execute_block(np.zeros(6, np.float32), np.zeros(2, np.complex64))
    with pytest.raises(Y.RangeError):
        q.interp_execute_block(np.zeros(3, np.complex64), np.zeros(5, np.float32))
    with pytest.raises(Y.RangeError):
        q.r2c_execute_block(np.zeros(3, np.float32), np.zeros(4, np.complex64))
    with pytest.raises(Y.RangeError):
        q.c2r_execute_block(np.zeros(3, np.complex64), np.zeros(3, np.float32))
    buf = Y.DeviceArray(4096, np.float32)
    with pytest.raises(Y.ConfigError):
        q.r2c_execute_block_dev(buf.ptr, 1000, buf.ptr + 4 * 500)
    with pytest.raises(Y.ConfigError):
        q.decim_execute_block_dev(buf.ptr, 1000, buf.ptr)
    for bad in (0, 1):
        with pytest.raises(Y.ConfigError):
            Y.FirHilbertFilter(bad, 60.0)
