"""tests/fdelay_ref.py (the restatement the GPU tests compare Fdelay against bit for bit) pinned to the reference's own
tests (src/filter/fdelay.rs:146-279) at their tolerance, its closed form pinned to its per-sample loop bit for bit, and
the per-sample-delay form pinned to a Doppler property.  Runs without a GPU."""
import numpy as np
import pytest

from fdelay_ref import KINDS, Design, FdelayRef, block, delay_estimate, f32, lag, lags, reset_state, same_bits

# (nmax, m, npfb): Ls = 2m + 1 with lag 0 or 1; a small odd bank; the default; the reference's test shape; a history
# longer than a tile and longer than the calls
SHAPES = [(1, 1, 1), (5, 2, 3), (200, 8, 64), (200, 12, 64), (3000, 4, 16)]
DELAYS = [0.0, 0.0001, 0.1, 0.9, 0.9999, 16.99, 17.0, 17.01, 199.9, 200.0]      # fdelay.rs:183-222


def splits(Ls):
    """call lengths: empty, shorter than both histories, across the 1024- and 2048-sample tile seams"""
    return [0, 1, Ls - 1, Ls, 1023, 1025, 2500]


def rand_input(rng, kind, n):
    x = rng.standard_normal(n).astype(f32)
    if kind != "rrrf":
        x = (x + 1j * rng.standard_normal(n).astype(f32)).astype(np.complex64)
    return x


def tracks(rng, nmax, npfb, n):
    """delay tracks of n samples over [0, nmax]"""
    t = np.arange(n, dtype=np.float64)
    step = np.zeros(n, f32)
    for b in range(0, n, 37):
        step[b: b + 37] = (0.0, nmax, nmax * 0.5)[(b // 37) % 3]
    wrap = (rng.integers(0, nmax, n) + 1.0 / (4 * npfb)).astype(f32)      # the branch rounds up to npfb and wraps
    out = {"ramp": (t * nmax / max(n - 1, 1)).astype(f32),
           "sine": (0.5 * nmax * (1 + np.sin(2 * np.pi * t / 411.0))).astype(f32),
           "random": (rng.random(n) * nmax).astype(f32),
           "step": step,
           "wrap": wrap}
    return {k: np.clip(v, 0, nmax).astype(f32) for k, v in out.items()}


def doppler_input():
    n = np.arange(4096)
    x = np.exp(2j * np.pi * 0.125 * n).astype(np.complex64)
    return x, (n / 64.0).astype(f32)


def doppler_peak(y):
    return int(np.argmax(np.abs(np.fft.fft(np.asarray(y, np.complex128) * np.hanning(4096)))))


@pytest.mark.parametrize("shape", SHAPES[:4])
@pytest.mark.parametrize("kind", list(KINDS))
def test_block_equals_loop(oracle, kind, shape):
    d = Design(oracle, kind, *shape)
    q, st = FdelayRef(oracle, d), reset_state(d)
    rng = np.random.default_rng(21)
    cuts = [0, 1, d.Ls - 1, d.Ls, 300, 77]
    trs = tracks(rng, d.nmax, d.npfb, sum(cuts))
    for name in ("random", "wrap", "step"):
        at = 0
        for i, n in enumerate(cuts):
            x = rand_input(rng, kind, n)
            if i % 2 == 0:
                tr = trs[name][at: at + n]
                want = q.execute_track(tr, x)
                got, st = block(d, st, x, tr)
            else:
                dl = f32(rng.random() * d.nmax) if i > 1 else f32(d.nmax)
                q.set_delay(dl)
                st = st[:2] + (dl,) + lag(dl, d.nmax, d.npfb)
                want = q.execute_block(x)
                got, st = block(d, st, x)
            assert same_bits(got, want), (kind, shape, name, i, n)
            s = q.state()
            assert same_bits(s[0], st[0]) and same_bits(s[1], st[1]) and s[2:] == st[2:]
            at += n


def test_block_equals_loop_long_history(oracle):
    d = Design(oracle, "crcf", 3000, 4, 16)
    q, st = FdelayRef(oracle, d), reset_state(d)
    rng = np.random.default_rng(22)
    for n in (500, 700):
        x, tr = rand_input(rng, "crcf", n), (rng.random(n) * 3000).astype(f32)
        want = q.execute_track(tr, x)
        got, st = block(d, st, x, tr)
        assert same_bits(got, want)


def test_branch_length_and_reset_lag(oracle):
    assert Design(oracle, "rrrf", 1, 1, 1).Ls == 3 and Design(oracle, "rrrf", 5, 2, 3).Ls == 4
    q = FdelayRef(oracle, Design(oracle, "rrrf", 200, 8, 64))
    assert (q.get_delay(), q.w_index, q.f_index) == (0.0, 199, 0)          # fdelay.rs:59-62
    assert lag(0.0, 200, 64) == (200, 0)


@pytest.mark.parametrize("delay", DELAYS)
def test_reference_delay_estimates(oracle, delay):                # fdelay.rs:146-222
    nmax, m, npfb = 200, 12, 64
    q = FdelayRef(oracle, Design(oracle, "rrrf", nmax, m, npfb))
    q.set_delay(f32(delay) * f32(0.7))
    q.adjust_delay(f32(delay) * f32(0.3))
    assert abs(float(q.get_delay()) - delay) <= 1e-6 * max(1.0, delay)
    x = np.zeros(nmax + 2 * m, f32)
    x[0] = 1.0
    y = q.execute_block(x)
    assert abs(float(delay_estimate(y, m)) - delay) <= 0.01
    # 0.0001: offset 199.9999 has fraction 0.9999, 64 * 0.9999 rounds to 64 = npfb and wraps into the window index;
    # 0.9999: offset 199.0001 rounds its branch down to 0
    if delay == 0.0001:
        assert (q.w_index, q.f_index) == (200, 0)
    if delay == 0.9999:
        assert (q.w_index, q.f_index) == (199, 0)


def test_lags_vector_equals_scalar():
    rng = np.random.default_rng(23)
    for nmax, npfb in ((1, 1), (5, 3), (200, 64), (3000, 16)):
        d = np.concatenate([(rng.random(2000) * nmax).astype(f32), np.arange(nmax + 1).astype(f32),
                            (np.arange(nmax) + 1.0 / (4 * npfb)).astype(f32),
                            (np.arange(nmax) + 1 - 0.5 / npfb).astype(f32)])
        D, f = lags(d, nmax, npfb)
        for i, v in enumerate(d):
            w1, f1 = lag(v, nmax, npfb)
            assert (nmax - D[i], f[i]) == (w1, f1), (nmax, npfb, v)
        assert np.all((D >= 0) & (D <= nmax) & (f >= 0) & (f < npfb))
    for bad in (-1.0, 201.0, float("nan")):
        with pytest.raises(ValueError):
            lag(bad, 200, 64)


def test_config_errors(oracle):                                   # fdelay.rs:224-249
    for bad in ((0, 12, 64), (200, 0, 64), (200, 12, 0)):
        with pytest.raises(ValueError):
            Design(oracle, "rrrf", *bad)
    q = FdelayRef(oracle, Design(oracle, "rrrf", 200, 8, 64))
    for fn in (lambda: q.set_delay(-1.0), lambda: q.set_delay(201.0), lambda: q.adjust_delay(-1.0)):
        with pytest.raises(ValueError):
            fn()
        assert (q.get_delay(), q.w_index, q.f_index) == (0.0, 199, 0)


def test_doppler_peak(oracle):
    """a delay growing by 1/64 sample per sample compresses a tone at 0.125 to 0.125 (1 - 1/64): bin 504 of 4096"""
    d = Design(oracle, "crcf", 200, 12, 64)
    x, tr = doppler_input()
    y, _ = block(d, reset_state(d), x, tr)
    spec = np.abs(np.fft.fft(y.astype(np.complex128) * np.hanning(4096)))
    assert doppler_peak(y) == 504
    assert 0.4 < spec[503] / spec[504] < 0.6 and 0.4 < spec[505] / spec[504] < 0.6       # a Hann main lobe on the bin
