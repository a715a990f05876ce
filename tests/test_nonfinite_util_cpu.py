"""nonfinite_util.py against the C oracle (built without fast-math, so it propagates NaN and Inf), and proof that
check_footprint can fail: on a mask one element too wide, one too narrow, and on one changed bit outside the mask."""
import numpy as np
import pytest

from gpu_util import rand_samples, rand_taps
from nonfinite_util import VALUES, check_footprint, dilate, mask, poison, runs

KINDS = ["rrrf", "crcf", "cccf"]


def test_poison_writes_one_component_of_a_copy():
    x = np.arange(8, dtype=np.float32)
    for name, v in VALUES.items():
        p = poison(x, 3, name)
        assert np.array_equal(x, np.arange(8, dtype=np.float32)) and p.dtype == x.dtype
        assert np.array_equal(np.flatnonzero(mask(p)), [3])
        assert np.isnan(p[3]) if np.isnan(v) else p[3] == v
    z = (np.arange(8) + 1j * np.arange(8)).astype(np.complex64)
    re, im, both = poison(z, 5, "-inf", "re"), poison(z, 5, "nan", "im"), poison(z, [0, 7], np.inf, "both")
    assert re[5].real == -np.inf and re[5].imag == 5.0
    assert im[5].real == 5.0 and np.isnan(im[5].imag)
    assert np.array_equal(np.flatnonzero(mask(both)), [0, 7]) and both[7].real == both[7].imag == np.inf
    assert np.array_equal(mask(re), mask(im)) and not mask(z).any()
    with pytest.raises(AssertionError):
        poison(x, 3, 1.0)
    with pytest.raises(AssertionError):
        poison(x, 3, "nan", "im")
    with pytest.raises(AssertionError):
        poison(x, 8, "nan")


def test_dilate_is_the_padded_length_rule():
    """a filter of L taps zero-padded to Lp taps: the sample at s reaches outputs s .. s + Lp - 1 instead of
    s .. s + L - 1, i.e. the reference's mask widened to the right by Lp - L, clipped at the end of the block"""
    n = 400
    for L, Lp in [(33, 64), (31, 32), (32, 32), (1, 64), (130, 256)]:
        for s in (0, 17, n - Lp - 1, n - Lp, n - L, n - 1):
            m = np.zeros(n, bool)
            m[s:s + L] = True
            want = np.zeros(n, bool)
            want[s:s + Lp] = True
            assert np.array_equal(dilate(m, Lp - L), want), (L, Lp, s)
    m = np.zeros(40, bool)
    m[[3, 4, 20, 38]] = True
    assert np.array_equal(np.flatnonzero(dilate(m, 2)), [3, 4, 5, 6, 20, 21, 22, 38, 39])
    assert np.array_equal(dilate(m, 0), m) and not dilate(np.zeros(9, bool), 5).any()
    assert runs(dilate(m, 2)) == [(3, 4), (20, 3), (38, 2)]
    assert runs(np.zeros(5, bool)) == [] and runs(np.ones(5, bool)) == [(0, 5)]
    m2 = np.zeros((3, 4), bool)                                 # per-frame masks keep their shape
    m2[1, 3] = True
    assert dilate(m2, 1).shape == (3, 4) and np.array_equal(np.flatnonzero(dilate(m2, 1)), [7, 8])


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_firfilt_poisons_its_window(oracle, kind, value):
    """FirFilter of L taps: the sample at s is in the window of outputs s .. s + L - 1, across call cuts"""
    rng = np.random.default_rng(77)
    n = 700
    for L in (1, 31, 33, 130):
        h, x = rand_taps(rng, kind, L), rand_samples(rng, kind, n)
        for s, part in ((0, "re"), (311, "im" if kind != "rrrf" else "re"), (499, "re"), (n - 1, "re")):
            q, c = oracle.FirFilter(kind, h), oracle.FirFilter(kind, h)
            q.set_scale(0.5), c.set_scale(0.5)
            xp = poison(x, s, value, part)
            got = np.concatenate([q.execute_block(xp[:500]), q.execute_block(xp[500:])])
            clean = np.concatenate([c.execute_block(x[:500]), c.execute_block(x[500:])])
            want = np.zeros(n, bool)
            want[s:s + L] = True
            check_footprint(got, clean, want, f"{kind} L {L} s {s} {value}")
            q.reset()
            assert not mask(q.execute_block(x[:64])).any()        # reset() clears the poisoned window


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_firdecim_poisons_its_window(oracle, kind, value):
    """decimator by M: output o sees samples M o - (L - 1) .. M o (the set test_firdecim_register_window_kernel states)"""
    rng = np.random.default_rng(78)
    n = 300
    for M, L in [(2, 9), (3, 64), (5, 7), (8, 129)]:
        h, x = rand_taps(rng, kind, L), rand_samples(rng, kind, n * M)
        for s in (0, 100 * M + 1, 200 * M - 1, n * M - 1):
            q, c = oracle.FirDecimationFilter(kind, M, h), oracle.FirDecimationFilter(kind, M, h)
            xp = poison(x, s, value)
            got = np.concatenate([q.execute_block(xp[:200 * M], 200), q.execute_block(xp[200 * M:], 100)])
            clean = np.concatenate([c.execute_block(x[:200 * M], 200), c.execute_block(x[200 * M:], 100)])
            o = np.arange(n)
            want = (M * o >= s) & (M * o - (L - 1) <= s)
            check_footprint(got, clean, want, f"{kind} M {M} L {L} s {s} {value}")


def _fir_case(oracle):
    rng = np.random.default_rng(79)
    L, n, s = 33, 256, 100
    h, x = rand_taps(rng, "crcf", L), rand_samples(rng, "crcf", n)
    got = oracle.FirFilter("crcf", h).execute_block(poison(x, s, "nan"))
    clean = oracle.FirFilter("crcf", h).execute_block(x)
    want = np.zeros(n, bool)
    want[s:s + L] = True
    check_footprint(got, clean, want)                            # the true footprint passes
    return got, clean, want, s, L


def test_check_footprint_fails_on_a_mask_widened_by_one(oracle):
    got, clean, want, s, L = _fir_case(oracle)
    wide = want.copy()
    wide[s + L] = True
    with pytest.raises(AssertionError, match=rf"first {s + L}, last {s + L}"):
        check_footprint(got, clean, wide)
    with pytest.raises(AssertionError, match="footprint differs"):
        check_footprint(got, clean, dilate(want, 1))
    early = want.copy()
    early[s - 1] = True                                           # one output before the bad sample
    with pytest.raises(AssertionError, match=rf"first {s - 1}, last {s - 1}"):
        check_footprint(got, clean, early)


def test_check_footprint_fails_on_a_mask_narrowed_by_one(oracle):
    got, clean, want, s, L = _fir_case(oracle)
    for drop in (s, s + L - 1):
        narrow = want.copy()
        narrow[drop] = False
        with pytest.raises(AssertionError, match=rf"first {drop}, last {drop}"):
            check_footprint(got, clean, narrow)
    with pytest.raises(AssertionError, match=r"poisoned but not expected: 33 elements in 1 runs, \(first, length\) \[\(100, 33\)\]"):
        check_footprint(got, clean, np.zeros_like(want))


def test_check_footprint_fails_on_one_changed_bit_outside_the_mask(oracle):
    got, clean, want, s, L = _fir_case(oracle)
    for i, word in ((0, 0), (s - 1, 1), (s + L, 0), (got.size - 1, 1)):
        bent = got.copy()
        w = bent.view(np.uint32)
        w[2 * i + word] ^= 1                                      # one ulp of one component
        with pytest.raises(AssertionError, match=rf"outside the footprint differ from the clean run, first {i} "):
            check_footprint(bent, clean, want)
    bent = got.copy()
    bent[s + 3] = 0                                               # inside the mask: a finite value there is a mask error
    with pytest.raises(AssertionError, match="expected but finite"):
        check_footprint(bent, clean, want)
    pz, nz = np.zeros(8, np.float32), np.zeros(8, np.float32)
    nz[5] = -0.0                                                  # -0.0 == +0.0 as floats, not as bits
    assert np.array_equal(pz, nz)
    with pytest.raises(AssertionError, match="first 5 "):
        check_footprint(nz, pz, np.zeros(8, bool))


def test_firdecim_cases_of_the_gpu_module_reach_every_instantiation():
    """pure Python: the shapes test_gpu_nonfinite.py feeds FirDecimationFilter reach every launch_fir_decim_consec
    instantiation and the general kernel, by its restatement of the dispatch"""
    from test_gpu_nonfinite import DECIM_CASES, DECIM_FORMS, decim_dispatch
    reached = {decim_dispatch(k, M, L, 2600)[0] for k, M, L in DECIM_CASES}
    assert reached == DECIM_FORMS, reached
    assert decim_dispatch("crcf", 12, 50, 2600) == ("general", 256)      # the tile halves until the span fits 48 KiB
    assert decim_dispatch("rrrf", 5, 7, 2600) == ("general", 1024)
