"""Non-finite footprints of FirPfbChr (tests/nonfinite_util.py): one NaN / +Inf / -Inf in the stream poisons an exact set
of outputs, every other output equals the clean stream's word for word, and after reset() a clean block equals a fresh
object's.

  general analyzer kernel   sample t poisons exactly the steps s with 0 <= (s+1)P - 1 - t < 2Mm, every channel; across a
                            call boundary too (the carried history is the last 2Mm - P samples: the same window)
  column analyzer kernel    built for Pb = 4 / 8 / 16 taps per branch, zero taps behind the 2m real ones (0 * NaN = NaN):
                            0 <= (s+1)P - 1 - t < Pb M, within the call
  synthesizer               a non-finite X_s[k] poisons exactly the output samples sP .. sP + 2Mm - 1 (the transform
                            spreads it over the step, the combine reads the step with every tap), across calls"""
import numpy as np
import pytest

from gpu_util import rand_samples
from nonfinite_util import VALUES, check_footprint, poison

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


def _taps(rng, M, m):
    return rng.uniform(0.1, 1.0, 2 * M * m).astype(np.float32)           # no zero among the real taps


def _steps_mask(nsteps, M, P, t, width):
    s = np.arange(nsteps)
    lag = (s + 1) * P - 1 - t
    return np.repeat((lag >= 0) & (lag < width), M)


def _run(q, fn, x, unit, calls):
    out, a = [], 0
    for c in calls:
        out.append(np.asarray(getattr(q, fn)(x[a * unit: (a + c) * unit])).reshape(-1))
        a += c
    return np.concatenate(out)


def _after_reset(ya, make, fn, q, x):
    q.reset()
    assert np.array_equal(np.asarray(getattr(q, fn)(x)).view(np.uint32), np.asarray(getattr(make(), fn)(x)).view(np.uint32))


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("M,P,m,calls,t", [(16, 12, 4, [40, 31], 455),      # the footprint crosses the call boundary
                                           (10, 7, 3, [29, 30], 101), (64, 48, 2, [9, 20], 430), (12, 9, 8, [50, 60], 3),
                                           (512, 1, 1, [700, 900], 650)])
def test_general_analyzer_footprint(ya, M, P, m, calls, t, value):
    rng = np.random.default_rng(7000 + M + P)
    h, n = _taps(rng, M, m), sum(calls)
    x = rand_samples(rng, "crcf", n * P)

    def make():
        q = ya.FirPfbChr(M, P, m, h)
        q.set_kernel(1)
        return q
    clean = _run(make(), "analyzer_execute", x, P, calls)
    q = make()
    got = _run(q, "analyzer_execute", poison(x, t, value, "im"), P, calls)
    assert q.get_last_kernel() == 1
    want = _steps_mask(n, M, P, t, 2 * M * m)
    assert want.any() and not want.all()
    check_footprint(got, clean, want, f"general M {M} P {P} m {m} t {t} {value}")
    _after_reset(ya, make, "analyzer_execute", q, x[: calls[0] * P])


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("M,P,p,pb,n,t", [(64, 48, 8, 8, 150, 2000), (64, 48, 6, 8, 150, 2001), (64, 16, 2, 4, 200, 1500),
                                          (128, 80, 4, 4, 130, 4000), (256, 192, 10, 16, 90, 5000), (64, 64, 16, 16, 80, 1999)])
def test_column_analyzer_footprint(ya, M, P, p, pb, n, t, value):
    rng = np.random.default_rng(7100 + M + P + p)
    m = p // 2
    h = _taps(rng, M, m)
    x = rand_samples(rng, "crcf", n * P)

    def make():
        q = ya.FirPfbChr(M, P, m, h)
        q.set_kernel(2)
        return q
    clean = _run(make(), "analyzer_execute", x, P, [n])
    q = make()
    got = _run(q, "analyzer_execute", poison(x, t, value), P, [n])
    assert q.get_last_kernel() == 2
    want = _steps_mask(n, M, P, t, pb * M)
    assert want.any() and not want.all() and not want[-M:].any()          # the whole footprint lies inside the call
    check_footprint(got, clean, want, f"column M {M} P {P} 2m {p} on {pb} t {t} {value}")
    _after_reset(ya, make, "analyzer_execute", q, x)


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("M,P,m,calls,s,k", [(16, 12, 4, [40, 31], 33, 5), (10, 7, 3, [29, 30], 28, 0), (64, 48, 2, [9, 20], 3, 63),
                                             (6, 1, 2, [40, 50], 30, 1), (512, 1, 1, [700, 900], 650, 100)])
def test_synthesizer_footprint(ya, M, P, m, calls, s, k, value):
    rng = np.random.default_rng(7200 + M + P)
    h, n = _taps(rng, M, m), sum(calls)
    X = rand_samples(rng, "crcf", n * M)

    def make():
        return ya.FirPfbChr(M, P, m, h)
    clean = _run(make(), "synthesizer_execute", X, M, calls)
    q = make()
    got = _run(q, "synthesizer_execute", poison(X, s * M + k, value), M, calls)
    t = np.arange(n * P)
    want = (t >= s * P) & (t < s * P + 2 * M * m)
    assert want.any() and not want.all()
    check_footprint(got, clean, want, f"synthesizer M {M} P {P} m {m} step {s} channel {k} {value}")
    _after_reset(ya, make, "synthesizer_execute", q, X[: calls[0] * M])
