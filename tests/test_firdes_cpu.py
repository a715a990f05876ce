"""fir_design_prototype and the prototype constructors at the C ABI (host code: no device needed).

Bound.  The taps must match the f64 evaluation of the same formulas (tests/firdes_ref.py) within
    2 x (worst deviation of the f32 restatement from f64 for that case) + 1e-6 max|h|:
the restatement's own deviation is what single precision costs for the case, the factor 2 covers another libm's sinf /
cosf / logf / expf rounding and fused multiply-adds, the second term the taps that are (near) zero.  Each case prints
its measured deviation (pytest -s)."""
import itertools

import numpy as np
import pytest

import firdes_ref as fr
from conftest import has_gpu

KS, MS, BETAS, DTS = (2, 3, 8), (1, 3, 12), (0.2, 0.3, 1.0), (0.0, 0.25)


def _allows(shape, beta):
    return not (shape == "Arkaiser" and beta >= 1.0)          # rkaiser.rs:57: beta in (0, 1)


CASES = [(s, k, m, b, dt) for s in fr.SHAPES for k, m, b, dt in itertools.product(KS, MS, BETAS, DTS) if _allows(s, b)]
CASES += [("Rrcos", 2, m, 0.25, dt) for m in MS for dt in DTS]      # 16 beta^2 z^2 = 1 exactly at z = +-1


@pytest.fixture(scope="module")
def designs():
    """(lib, f32 restatement, f64) taps per case, computed once"""
    import yagi_amd as ya
    out = {}
    for case in CASES:
        s, k, m, b, dt = case
        f = fr.SHAPES[s]
        out[case] = (ya.fir_design_prototype(f, k, m, b, dt), fr.design_prototype(f, k, m, b, dt, np.float32),
                     fr.design_prototype(f, k, m, b, dt, np.float64))
    return out


def test_cases_keep_clear_of_the_branch_thresholds():
    """f64: every compared quantity of Rrcos is at least 1e-3 from its threshold (|z| from 1e-5, |1 - 16 beta^2 z^2| from
    sqrt(1e-5)) except at the exact centre tap; deep inside a branch counts as clear, and beta = 0.25, k = 2 is inside the
    second branch on purpose.  Rcos: |1 - 4 beta^2 z^2| at least 5e-4 from 1e-3 (f32 rounds that quantity to 1e-6)."""
    for s, k, m, b, dt in CASES:
        if s == "Rrcos":
            dz, dg = fr.rrcos_branch_distances(k, m, b, dt)
            assert dz >= 1e-3 and dg >= 1e-3, (k, m, b, dt, dz, dg)
        if s == "Rcos":
            assert fr.rcos_branch_distance(k, m, b, dt) >= 5e-4, (k, m, b, dt)
    z = (np.arange(2 * 2 * 3 + 1, dtype=np.float32) / np.float32(2)) - np.float32(3)
    g = np.float32(1) - np.float32(16) * np.float32(0.25) * np.float32(0.25) * z * z
    assert (g[np.abs(z) == 1] == 0).all()                     # the special branch is taken at z = +-1, exactly


def test_prototype_matches_f64_within_twice_the_f32_restatement(designs):
    worst = {}
    for case, (got, h32, h64) in designs.items():
        assert got.dtype == np.float32 and got.size == 2 * case[1] * case[2] + 1
        own = np.max(np.abs(h32.astype(np.float64) - h64))
        dev = np.max(np.abs(got.astype(np.float64) - h64))
        bound = 2 * own + 1e-6 * np.max(np.abs(h64))
        print(f"{case}: lib {dev:.3e} restatement {own:.3e} bound {bound:.3e}")
        worst[case[0]] = max(worst.get(case[0], 0.0), dev / np.max(np.abs(h64)))
        assert dev <= bound, (case, dev, own, bound)
    print("worst deviation / max|h| per shape:", {s: f"{v:.2e}" for s, v in worst.items()})


def test_taps_symmetric_without_a_fractional_delay(designs):
    """dt = 0: Kaiser and Arkaiser are symmetric bit for bit (t = i - (n-1)/2 is exact, sin is odd, cos and I0 even).
    Rcos and Rrcos go through z = n/k - m, exact for k a power of two (symmetric bit for bit again); for k = 3 the two
    roundings of n/k and (2km - n)/k differ by up to an ulp of m, 1e-6 relative at m = 12, and the tap's slope in z is
    at most pi max|h|, so the two sides agree to 4e-6 max|h|."""
    for (s, k, m, b, dt), (got, _, _) in designs.items():
        if dt != 0.0:
            continue
        if s in ("Kaiser", "Arkaiser") or k & (k - 1) == 0:
            assert got.tobytes() == got[::-1].tobytes(), (s, k, m, b)
        else:
            assert np.max(np.abs(got - got[::-1])) <= 4e-6 * np.max(np.abs(got)), (s, k, m, b)


def test_rcos_is_a_nyquist_pulse(designs):
    for (s, k, m, b, dt), (got, _, _) in designs.items():
        if s == "Rcos" and dt == 0.0:
            c = k * m
            idx = [c + j * k for j in range(-m, m + 1) if j != 0]
            assert np.max(np.abs(got[idx])) <= 1e-6 * got[c], (k, m, b)


def test_arkaiser_has_energy_k(designs):
    for (s, k, m, b, dt), (got, _, _) in designs.items():
        if s == "Arkaiser":
            assert abs(np.sum(got.astype(np.float64) ** 2) - k) <= 1e-5 * k, (k, m, b, dt)


def test_stopband_estimate_matches_the_restatement():
    import yagi_amd as ya
    for df, n in [(0.1, 5), (0.025, 193), (0.15, 37), (0.5, 13)]:
        got = ya.estimate_req_filter_stopband_attenuation(df, n)
        want = fr.estimate_stopband_attenuation(np.float32(df), n, np.float64)
        assert abs(float(got) - float(want)) <= 1e-3, (df, n, got, want)     # one bisection step is 2e-4 dB
    for df in (0.0, -0.1, 0.6):
        with pytest.raises(ya.ConfigError):
            ya.estimate_req_filter_stopband_attenuation(df, 13)


def test_config_errors():
    import yagi_amd as ya
    S = ya.FirFilterShape
    for name, num in fr.UNSUPPORTED.items():                  # every shape that is not built
        assert int(S[name]) == num
        with pytest.raises(ya.ConfigError, match="not built"):
            ya.fir_design_prototype(S[name], 2, 3, 0.3)
    for name, num in fr.SHAPES.items():                       # the reference's order
        assert int(S[name]) == num
    with pytest.raises(ya.ConfigError):
        ya.fir_design_prototype(15, 2, 3, 0.3)
    with pytest.raises(ya.ConfigError):
        ya.fir_design_prototype(-1, 2, 3, 0.3)
    with pytest.raises(ya.ConfigError, match=r"leaves \(0, 1\)"):
        ya.fir_design_prototype(S.Arkaiser, 2, 1, 0.05)       # the closed-form rho_hat is negative there
    assert not 0 < fr.arkaiser_rho(1, 0.05, np.float64) < 1
    for k in range(2, 13):                                    # the reference's own test shapes stay inside
        for m, b in ((4, 0.3), (12, 0.3), (31, 0.3), (25, 0.2), (11, 0.35), (17, 0.27)):
            assert 0 < fr.arkaiser_rho(m, b, np.float64) < 1
    for shape in (S.Kaiser, S.Rcos, S.Rrcos, S.Arkaiser):
        for bad in ((0, 3, 0.3, 0.0), (2, 0, 0.3, 0.0), (2, 3, 0.0, 0.0), (2, 3, -0.1, 0.0), (2, 3, 1.1, 0.0)):
            with pytest.raises(ya.ConfigError):
                ya.fir_design_prototype(shape, *bad)
    for bad in ((1, 3, 0.3, 0.0), (2, 3, 1.0, 0.0), (2, 3, 0.3, 1.5), (2, 3, 0.3, -1.5)):     # rkaiser.rs:51-62
        with pytest.raises(ya.ConfigError):
            ya.fir_design_prototype(S.Arkaiser, *bad)
    for dt in (0.6, -0.5):                                    # kaiser.rs:18
        with pytest.raises(ya.ConfigError):
            ya.fir_design_prototype(S.Kaiser, 2, 3, 0.3, dt)


def test_constructor_argument_errors_come_before_the_device():
    """firinterp.rs:105-124, firdecim.rs:102-121, firfilt.rs:112-116: their own checks and the design's are ConfigError
    with or without a device"""
    import yagi_amd as ya
    S = ya.FirFilterShape
    for kind in ("rrrf", "crcf", "cccf"):
        for bad in ((S.Rrcos, 1, 3, 0.3, 0.0), (S.Rrcos, 2, 0, 0.3, 0.0), (S.Rrcos, 2, 3, 1.5, 0.0), (S.Rrcos, 2, 3, 0.3, 1.5),
                    (S.Pm, 2, 3, 0.3, 0.0), (S.Arkaiser, 2, 1, 0.05, 0.0)):
            with pytest.raises(ya.ConfigError):
                ya.FirInterpolationFilter.new_prototype(kind, *bad)
            with pytest.raises(ya.ConfigError):
                ya.FirDecimationFilter.new_prototype(kind, *bad)
        for bad in ((S.Pm, 2, 3, 0.3, 0.0), (S.Rrcos, 2, 0, 0.3, 0.0), (S.Arkaiser, 2, 1, 0.05, 0.0)):
            with pytest.raises(ya.ConfigError):
                ya.FirFilter.new_rnyquist(kind, *bad)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_prototype_constructors_without_a_gpu_are_a_device_error():
    import yagi_amd as ya
    S = ya.FirFilterShape
    with pytest.raises(ya.DeviceError):
        ya.FirInterpolationFilter.new_prototype("crcf", S.Rrcos, 2, 3, 0.3)
    with pytest.raises(ya.DeviceError):
        ya.FirDecimationFilter.new_prototype("crcf", S.Rrcos, 2, 3, 0.3)
    with pytest.raises(ya.DeviceError):
        ya.FirFilter.new_rnyquist("crcf", S.Rrcos, 2, 3, 0.3)
