"""iir_design_lowpass_sos (host.cpp) -- the low-pass / second-order-section branch of iir_design
(src/filter/iir/design/mod.rs:567-717) with the Butterworth and Chebyshev-II prototypes.  The cascade response is
evaluated in f64 and compared with the closed forms, W = tan(pi f) / tan(pi fc), e = 10^(-as/20):
    Butterworth   |H|^2 = 1 / (1 + W^(2n))
    Chebyshev-II  |H|^2 = 1 / (1 + 1 / (e^2 T_n(1/W)^2))
A numpy restatement of the design deviates from the Butterworth form by at most 1.2e-5 dB above -80 dB and from the
Chebyshev-II form by at most 8.4e-6 in |H|^2; the bounds below (1e-3 dB, the tolerance of the reference's own masks at
design/mod.rs:1214, and 1e-4) leave room for another libm.  No device is needed."""
import numpy as np
import pytest

import yagi_amd as ya

BUTTER = [(1, .25), (2, .25), (5, .05), (5, .2), (7, 1 / 6), (9, .125), (9, .25), (15, .35)]
CHEBY2 = [(1, .25), (2, .25), (5, .05), (5, .2), (7, 1 / 6), (9, .125), (9, .25), (12, .3)]
F = np.arange(800) / 1600.0                                  # 800 points on [0, 0.5)


def response(b, a, f=F):
    z = np.exp(-2j * np.pi * f)
    h = np.ones(len(f), np.complex128)
    for bk, ak in zip(b.astype(np.float64), a.astype(np.float64)):
        h *= (bk[0] + bk[1] * z + bk[2] * z * z) / (ak[0] + ak[1] * z + ak[2] * z * z)
    return h


def cheb(n, x):
    x = np.asarray(x, np.float64)
    ax = np.abs(x)
    big = np.cosh(n * np.arccosh(np.maximum(ax, 1.0))) * np.where((x < 0) & (n % 2 == 1), -1.0, 1.0)
    return np.where(ax <= 1.0, np.cos(n * np.arccos(np.clip(x, -1.0, 1.0))), big)


@pytest.mark.parametrize("n,fc", BUTTER)
def test_butterworth_closed_form(n, fc):
    b, a = ya.iir_design_lowpass_sos(ya.IirFilterShape.Butter, n, fc)
    assert b.shape == a.shape == ((n + 1) // 2, 3)
    want = 1.0 / (1.0 + (np.tan(np.pi * F) / np.tan(np.pi * fc)) ** (2 * n))
    got = np.abs(response(b, a)) ** 2
    sel = 10 * np.log10(want) > -80.0
    err = np.max(np.abs(10 * np.log10(got[sel]) - 10 * np.log10(want[sel])))
    print(f"butter n={n} fc={fc:.4f}: {err:.3e} dB")
    assert err <= 1e-3


@pytest.mark.parametrize("n,fc", CHEBY2)
def test_cheby2_closed_form(n, fc):
    as_ = 60.0
    b, a = ya.iir_design_lowpass_sos(ya.IirFilterShape.Cheby2, n, fc, 0.1, as_)
    eps = 10.0 ** (-as_ / 20)
    with np.errstate(divide="ignore", over="ignore"):
        W = np.tan(np.pi * F) / np.tan(np.pi * fc)
        t = cheb(n, 1.0 / W)
        want = 1.0 / (1.0 + 1.0 / (eps * eps * t * t))
    want[0] = 1.0
    err = np.max(np.abs(np.abs(response(b, a)) ** 2 - want))
    print(f"cheby2 n={n} fc={fc:.4f}: {err:.3e}")
    assert err <= 1e-4


@pytest.mark.parametrize("n,fc,fs", [(5, 0.20, 0.40), (5, 0.05, 0.19), (15, 0.35, 0.41)])
def test_iirdes_butter_lowpass_masks(n, fc, fs):             # design/mod.rs:1213-1269 (_0, _1, _4)
    tol = 1e-3
    b, a = ya.iir_design_lowpass_sos(ya.IirFilterShape.Butter, n, fc, 1.0, 60.0)
    f = np.arange(800) / 800.0 - 0.5                          # validate_psd_iirfilt: nfft points on [-0.5, 0.5)
    psd = 20 * np.log10(np.abs(response(b, a, f)) + 1e-300)
    sel = (f >= 0.0) & (f <= 0.98 * fc)
    assert psd[sel].min() >= -3.0 - tol and psd[sel].max() <= tol
    sel = (f >= fs) & (f <= 0.5)
    assert psd[sel].max() <= -60.0 + tol


def test_iirdes_butter_2():
    """design/mod.rs:993-1022 as the closed form: with fc = 0.25 the prewarp is tan(pi/4) = 1, the poles are
    +-j (sqrt2 - 1) and unit DC gain gives b = (1 - sqrt2/2) [1, 2, 1] = (2 - sqrt2)/2 [1, 2, 1], the reference's
    table b_test = 0.292893218813452 [1, 2, 1] (:1013-1014), and a = [1, 0, 3 - 2 sqrt2]"""
    b, a = ya.iir_design_lowpass_sos(ya.IirFilterShape.Butter, 2, 0.25, 1.0, 40.0)
    r2 = np.sqrt(2.0)
    assert abs((2 - r2) / 2 - 0.292893218813452) < 1e-15
    assert np.allclose(b[0], (2 - r2) / 2 * np.array([1.0, 2.0, 1.0]), rtol=0, atol=1e-6)
    assert np.allclose(a[0], [1.0, 0.0, 3 - 2 * r2], rtol=0, atol=1e-6)


@pytest.mark.parametrize("shape", ["Butter", "Cheby2"])
@pytest.mark.parametrize("n,fc", [(1, .25), (2, .1), (5, .2), (8, .05), (9, .25), (15, .35)])
def test_structure(shape, n, fc):
    b, a = ya.iir_design_lowpass_sos(ya.IirFilterShape[shape], n, fc, 0.1, 60.0)
    for k in range(len(a)):
        assert a[k][0] == 1.0
        assert np.all(np.abs(np.roots(a[k][:3 if a[k][2] != 0 else 2].astype(np.float64))) < 1.0)
        if shape == "Butter":
            nz = 2 if (k < n // 2) else 1
            assert np.allclose(np.roots(b[k][:nz + 1].astype(np.float64)), -1.0, atol=2e-3)   # a double root in f32
    if n % 2:
        assert b[-1][2] == 0.0 and a[-1][2] == 0.0
    dc = np.prod(b.astype(np.float64).sum(axis=1) / a.astype(np.float64).sum(axis=1))
    assert abs(dc - 1.0) < 1e-4


def test_config_errors():
    S = ya.IirFilterShape
    for args in [(S.Butter, 5, 0.0), (S.Butter, 5, 0.5), (S.Butter, 5, -0.1), (S.Butter, 5, 0.7),
                 (S.Butter, 5, 0.2, 0.0), (S.Butter, 5, 0.2, -1.0), (S.Butter, 5, 0.2, 0.1, 0.0),
                 (S.Cheby2, 5, 0.2, 0.1, -3.0), (S.Butter, 0, 0.2), (S.Cheby2, 0, 0.2)]:
        with pytest.raises(ya.ConfigError):
            ya.iir_design_lowpass_sos(*args)
    for shape in (S.Cheby1, S.Ellip, S.Bessel):
        with pytest.raises(ya.ConfigError, match="not built"):
            ya.iir_design_lowpass_sos(shape, 5, 0.2)
