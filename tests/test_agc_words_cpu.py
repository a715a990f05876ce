"""The library's ln, exp and log10 in f32 (yagi_hip.h, the Agc block; yagi_amd.lnf / expf / log10f run them on the host):
bit for bit the Python restatement of tests/agc_ref.py, and within half an ulp plus the f64 evaluation error of the
true value (mpmath), with no cap on mismatches."""
import math

import mpmath
import numpy as np
import pytest

import agc_ref as ar

import yagi_amd as ya

F = np.float32
TINY, SUB_MAX, NORM_MIN, NORM_MAX = (np.array([b], np.uint32).view(F)[0] for b in (1, 0x007fffff, 0x00800000, 0x7f7fffff))
LANDMARKS = np.array([1.0, TINY, SUB_MAX, NORM_MIN, NORM_MAX] + [2.0 ** k for k in range(-149, 128)]
                     + [10.0 ** k for k in range(-45, 39)], np.float64).astype(F)
WORDS = {"ln": (ya.lnf, ar.lnf, mpmath.log), "log10": (ya.log10f, ar.log10f, mpmath.log10),
         "exp": (ya.expf, ar.expf, mpmath.exp)}


def positive_patterns(seed, n):
    """seeded positive finite f32 bit patterns, subnormals included"""
    return np.random.default_rng(seed).integers(1, 0x7f800000, n).astype(np.uint32).view(F)


def restated(fn, x):
    return np.array([fn(v) for v in x], F)


@pytest.mark.parametrize("word", ["ln", "log10"])
def test_ln_and_log10_equal_the_restatement(word):
    lib, ref, _ = WORDS[word]
    x = np.concatenate([positive_patterns(7, 1 << 20), LANDMARKS])
    assert ar.same_words(lib(x), restated(ref, x))


def test_exp_equals_the_restatement():
    lib, ref, _ = WORDS["exp"]
    grid = np.linspace(-110.0, 95.0, (1 << 20) + 1).astype(F)
    x = np.concatenate([grid, LANDMARKS, -LANDMARKS, np.array([-104.0, -103.98, -103.97, -87.4, 88.72, 88.73, 0.0, -0.0], F)])
    assert ar.same_words(lib(x), restated(ref, x))


def test_special_values():
    inf, nan = F(np.inf), F(np.nan)
    for lib, ref in ((ya.lnf, ar.lnf), (ya.log10f, ar.log10f)):
        got = lib(np.array([0.0, -0.0, inf, -1.0, -TINY, -inf, nan, 1.0], F))
        assert got[0] == -inf and got[1] == -inf and got[2] == inf and np.isnan(got[3:7]).all()
        assert got[7] == 0 and not np.signbit(got[7])
        assert ar.same_words(got, restated(ref, np.array([0.0, -0.0, inf, -1.0, -TINY, -inf, nan, 1.0], F)))
        assert np.isfinite(lib(np.array([TINY, SUB_MAX], F))).all(), "subnormal arguments are ordinary ones"
    x = np.array([nan, -inf, inf, 0.0, -200.0, 200.0, -103.0, -100.0], F)
    got = ya.expf(x)
    assert np.isnan(got[0]) and got[1] == 0 and not np.signbit(got[1]) and got[2] == inf and got[3] == 1
    assert got[4] == 0 and got[5] == inf
    assert 0 < got[6] < NORM_MIN and 0 < got[7] < NORM_MIN, "subnormal results come from the f64 -> f32 rounding"
    assert ar.same_words(got, restated(ar.expf, x))
    assert ya.lnf(np.zeros(0, F)).size == 0


def ulp32(v):
    v = abs(float(v))
    return 2.0 ** -149 if v < 2.0 ** -126 else 2.0 ** (math.frexp(v)[1] - 24)


@pytest.mark.parametrize("word", ["ln", "log10", "exp"])
def test_accuracy_against_mpmath(word):
    """|float64(word) - true| <= (0.5 + 2^-12) ulp32(word), and the f64 evaluation itself within 2^-45 relative"""
    lib, _, true = WORDS[word]
    if word == "exp":
        x = np.random.default_rng(3).uniform(-103.0, 88.7, 20000).astype(F)
        f64 = [ar.exp64(float(v)) for v in x]
    else:
        x = positive_patterns(5, 20000)
        f64 = [ar.ln64(float(v)) * (ar.INV_LN10 if word == "log10" else 1.0) for v in x]
    got = lib(x)
    with mpmath.workprec(120):
        worst_ulp = worst_rel = 0.0
        for v, g, d in zip(x, got, f64):
            t = true(mpmath.mpf(float(v)))
            worst_ulp = max(worst_ulp, float(abs(mpmath.mpf(float(g)) - t) / ulp32(g)))
            if t != 0:
                worst_rel = max(worst_rel, float(abs((mpmath.mpf(d) - t) / t)))
    print(f"{word}: worst {worst_ulp:.6f} ulp32, f64 evaluation 2^{math.log2(worst_rel):.2f} relative")
    assert worst_rel < 2.0 ** -45
    assert worst_ulp <= 0.5 + 2.0 ** -12


def test_set_rssi_word():
    """set_rssi's 10^(-rssi / 20) = (float)exp64((double)fl32(-rssi / 20) ln 10) runs on the host inside set_rssi (the GPU
    tests compare it with this restatement); here the restated word is held against the true power of ten"""
    for rssi in (0.0, -37.5, 20.0, 330.0, -400.0, 1e30):
        g = ar.exp10_rssi(rssi)
        with mpmath.workprec(120):
            t = mpmath.power(10, mpmath.mpf(float(-F(rssi) / F(20.0))))
        if 1e-38 < t < 1e38:
            assert abs(mpmath.mpf(float(g)) - t) <= (0.5 + 2.0 ** -12) * ulp32(g)
