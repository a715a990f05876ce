"""The restatements of iirmap_ref (IirDecimationFilter, IirInterpolationFilter, IirHilbertFilter over iir_ref.Seq32)
pinned with the reference's own properties: the copy tests (iirinterp.rs:195-218, iirhilb.rs:331-380), reset, the
equivalence of the two real Hilbert filters with the virtual complex stream, and the spectral masks of
iirhilb.rs:175-317 with filters from iir_design_lowpass_sos and the pulse from fir_design_kaiser."""
import numpy as np
import pytest

import yagi_amd as ya
from iir_ref import Seq32
from iirmap_ref import IirDecimRef, IirHilbRef, IirInterpRef, hilb_input, hilb_output, zero_stuff
from psd_util import validate_psd_signal

RNG = np.random.default_rng(7)


def crand(n):
    return ((RNG.standard_normal(n) + 1j * RNG.standard_normal(n))).astype(np.complex64)


def butter(n, fc):
    b, a = ya.iir_design_lowpass_sos(ya.IirFilterShape.Butter, n, fc, 0.1, 60.0)
    return b.ravel(), a.ravel(), len(b)


def test_rate_copy_and_virtual_stream():
    b, a, ns = butter(7, 0.5 / 3)
    for R, per_in in ((IirInterpRef, 1), (IirDecimRef, 3)):
        q0 = R("crcf", 3, b, a, nsos=ns, scale=3.0 if R is IirInterpRef else 1.0)
        x = crand(20 * per_in)
        q0.execute_block(x)
        q1 = q0.clone()
        x = crand(20 * per_in)
        y0 = q0.execute_block(x)
        assert np.array_equal(y0, q1.execute_block(x))
        # the wrapper is the filter over the virtual stream
        f = Seq32("crcf", b, a, nsos=ns, scale=q0.f.scale)
        q0.reset()
        v = f.execute_block(zero_stuff(x, 3) if R is IirInterpRef else x)
        assert np.array_equal(q0.execute_block(x), v if R is IirInterpRef else v[::3])


@pytest.mark.parametrize("mode", ["r2c", "c2r", "decim", "interp"])
def test_hilbert_copy_reset_and_virtual_stream(mode):
    b, a, ns = butter(7, 0.25)
    q0 = IirHilbRef(b, a, ns)
    real_in = mode in ("r2c", "decim")
    per = 2 if mode == "decim" else 1
    mk = lambda n: RNG.standard_normal(n * per).astype(np.float32) if real_in else crand(n)
    run = lambda q, x: getattr(q, mode + "_execute_block")(x)
    x0 = mk(81)
    first = run(q0, x0)
    q1 = q0.clone()
    x = mk(80)
    st = q0.state
    y0 = run(q0, x)
    assert np.array_equal(y0, run(q1, x))
    # one complex filter over the mapped stream gives the same words as the two real filters
    f = Seq32("crcf", b, a, nsos=ns)
    f.execute_block(hilb_input(mode, x0, 0))
    v = f.execute_block(hilb_input(mode, x, st))
    assert np.array_equal(hilb_output(mode, v, st).view(np.uint32), y0.view(np.uint32))
    q0.reset()
    assert q0.state == 0
    assert np.array_equal(run(q0, x0), first)


def test_iirhilbf_interp_decim_masks():                      # iirhilb.rs:175-231
    tol, bw, as_, p, m = 1.0, 0.4, 60.0, 40, 5
    b, a, ns = butter(m, 0.25)
    q = IirHilbRef(b, a, ns)
    h_len = 2 * p + 1
    n = h_len + 2 * m + 8
    w = np.float32(0.36 * bw)
    h = ya.fir_design_kaiser(h_len, float(w), 80.0, 0.0)
    buf0 = np.zeros(n, np.complex64)
    buf0[:h_len] = np.float32(2.0) * w * h
    buf1 = q.interp_execute_block(buf0)
    q.reset()
    buf2 = q.decim_execute_block(buf1)
    orig = [(-0.5, -0.5 * bw, 0.0, -as_ + tol, False, True), (-0.3 * bw, 0.3 * bw, -1.0, 1.0, True, True),
            (0.5 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    interp = [(-0.5, -0.25 - 0.25 * bw, 0.0, -as_ + tol, False, True), (-0.25 - 0.15 * bw, -0.25 + 0.15 * bw, -1.0, 1.0, True, True),
              (-0.25 + 0.25 * bw, 0.25 - 0.25 * bw, 0.0, -as_ + tol, False, True),
              (0.25 - 0.15 * bw, 0.25 + 0.15 * bw, -1.0, 1.0, True, True), (0.25 + 0.25 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    assert validate_psd_signal(buf0, orig)[0]
    assert validate_psd_signal(buf1, interp)[0]
    assert validate_psd_signal(buf2, orig)[0]


def test_iirhilbf_filter_masks():                            # iirhilb.rs:233-317
    tol, bw, f0, ft, as_, p, m = 1.0, 0.2, 0.3, -0.3, 60.0, 50, 7
    b, a, ns = butter(m, 0.25)
    q = IirHilbRef(b, a, ns)
    h_len = 2 * p + 1
    n = h_len + 2 * m + 8
    w = 0.36 * bw
    h = ya.fir_design_kaiser(h_len, w, 80.0, 0.0).astype(np.float64)
    i = np.arange(h_len)
    buf0 = np.zeros(n, np.complex128)
    buf0[:h_len] = 2.0 * w * h * np.exp(2j * np.pi * f0 * i) + 1e-3 * np.kaiser(n, 10.0)[:h_len] * np.exp(2j * np.pi * ft * i)
    buf0 = buf0.astype(np.complex64)
    buf1 = q.c2r_execute_block(buf0) * np.float32(2.0)
    q.reset()
    buf2 = q.r2c_execute_block(buf1) * np.float32(0.5)
    orig = [(-0.5, ft - 0.03, 0.0, -as_ + tol, False, True), (ft - 0.01, ft + 0.01, -40.0, 0.0, True, False),
            (ft + 0.03, f0 - 0.5 * bw, 0.0, -as_ + tol, False, True), (f0 - 0.3 * bw, f0 + 0.3 * bw, -1.0, 1.0, True, True),
            (f0 + 0.5 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    c2r = [(-0.5, -f0 - 0.5 * bw, 0.0, -as_ + tol, False, True), (-f0 - 0.3 * bw, -f0 + 0.3 * bw, -1.0, 1.0, True, True),
           (-f0 + 0.5 * bw, f0 - 0.5 * bw, 0.0, -as_ + tol, False, True), (f0 - 0.3 * bw, f0 + 0.3 * bw, -1.0, 1.0, True, True),
           (f0 + 0.5 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    r2c = [(-0.5, f0 - 0.5 * bw, 0.0, -as_ + tol, False, True), (f0 - 0.3 * bw, f0 + 0.3 * bw, -1.0, 1.0, True, True),
           (f0 + 0.5 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    for name, buf, reg in (("input", buf0, orig), ("c2r", buf1, c2r), ("r2c", buf2, r2c)):
        ok, worst = validate_psd_signal(buf, reg)
        assert ok, (name, worst)
