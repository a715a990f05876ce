"""tests/autocorr_ref.py on the CPU: the fast numpy form against the composition of oracle.Window and oracle.dotprod
that defines Autocorr (bytes-equal), the d = 0 identity, the repeated-preamble property the object exists for, and the
stream semantics (split blocks, push / execute, clone, reset).  No GPU."""
import numpy as np
import pytest

import autocorr_ref as acr

SHAPES = [(1, 1, 50), (4, 3, 100), (16, 16, 300), (64, 5, 400), (7, 100, 300), (1, 0, 50), (33, 0, 200)]
KINDS = ["cccf", "rrrf"]


def seed(*v):
    return int(np.dot(v, [1000003, 1009, 17][:len(v)]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,d,n", SHAPES)
def test_fast_form_equals_the_oracle_composition(oracle, kind, W, d, n):
    x = acr.stream(np.random.default_rng(seed(W, d, n)), kind, n)
    u = x.view(np.uint32)
    assert np.any(u == 0x80000000) and np.any(u == 0)
    rxx, en = acr.Autocorr(kind, W, d).execute_block(x, energy=True)
    want_rxx, want_en = acr.SlowAutocorr(oracle, kind, W, d).execute_block(x)
    assert rxx.dtype == want_rxx.dtype and en.dtype == np.float32
    assert rxx.tobytes() == want_rxx.tobytes()
    assert en.tobytes() == want_en.tobytes()


@pytest.mark.parametrize("W", [1, 33])
def test_zero_delay_gives_the_energy_and_a_positive_zero(W):
    """fl(-ab) + fl(ba) = +0 and a.re a.re - a.im (-a.im) is the energy's own expression"""
    x = acr.stream(np.random.default_rng(W), "cccf", 200)
    rxx, en = acr.Autocorr("cccf", W, 0).execute_block(x, energy=True)
    assert np.ascontiguousarray(rxx.real).tobytes() == en.tobytes()
    assert np.ascontiguousarray(rxx.imag).tobytes() == np.zeros(x.size, np.float32).tobytes()
    xr = acr.stream(np.random.default_rng(W + 1), "rrrf", 200)
    rr, er = acr.Autocorr("rrrf", W, 0).execute_block(xr, energy=True)
    assert rr.tobytes() == er.tobytes()


def test_repeated_preamble_plateau_and_carrier_offset():
    """a noise-free preamble of period 32, three repeats, 0.01 cycles/sample of carrier offset, d = W = 32: on the plateau
    (both windows inside the repeats) |rxx| / energy = 1 and angle(rxx) / (2 pi d) is the offset"""
    P, f0 = 32, 0.01
    rng = np.random.default_rng(5)
    pre = (rng.standard_normal(P) + 1j * rng.standard_normal(P)) / np.sqrt(2)
    x = np.tile(pre, 3) * np.exp(2j * np.pi * f0 * np.arange(3 * P))
    rxx, en = acr.Autocorr("cccf", P, P).execute_block(x.astype(np.complex64), energy=True)
    plateau = slice(2 * P - 1, 3 * P)
    ratio = np.abs(rxx[plateau].astype(np.complex128)) / en[plateau].astype(np.float64)
    freq = np.angle(rxx[plateau].astype(np.complex128)) / (2 * np.pi * P)
    print("ratio", ratio.min(), ratio.max(), "freq", freq.min(), freq.max())
    assert np.all(np.abs(ratio - 1.0) <= 1e-5), (ratio.min(), ratio.max())
    assert np.all(np.abs(freq - f0) <= 1e-6), (freq.min(), freq.max())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,d", [(4, 3), (16, 16), (7, 100), (1, 0)])
def test_split_stream_push_clone_and_reset(kind, W, d):
    x = acr.stream(np.random.default_rng(seed(W, d)), kind, 400)
    whole_rxx, whole_en = acr.Autocorr(kind, W, d).execute_block(x, energy=True)
    q = acr.Autocorr(kind, W, d)
    assert (q.window_size, q.delay) == (W, d)
    rxx, en, at = [], [], 0
    for step, n in enumerate([1, 2, 5, W + d + 3, 1, 60, 3, 100]):          # several shorter than W - 1 + d
        if step % 2:
            for v in x[at:at + n]:
                q.push(v)
                rxx.append(np.array([q.execute()], q.T))
                en.append(np.array([q.get_energy()], np.float32))
        else:
            r, e = q.execute_block(x[at:at + n], energy=True)
            rxx.append(r)
            en.append(e)
        at += n
    c = q.clone()
    for o in (q, c):
        r, e = o.execute_block(x[at:], energy=True)
        assert np.concatenate(rxx + [r]).tobytes() == whole_rxx.tobytes()
        assert np.concatenate(en + [e]).tobytes() == whole_en.tobytes()
    w = acr.Autocorr(kind, W, d)                                              # write() pushes without computing
    w.write(x[:150])
    assert w.execute_block(x[150:]).tobytes() == whole_rxx[150:].tobytes()
    q.reset()
    assert q.execute_block(x).tobytes() == whole_rxx.tobytes()
