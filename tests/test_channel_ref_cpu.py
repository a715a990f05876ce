"""tests/channel_ref.py against itself and against what it is built from: its two forms agree bit for bit across uneven
calls; the cos and sin words stay within half an f32 ulp plus E of numpy's f64 values on all 2^24 arguments; a delta
channel is the identity; the offset alone is tests/osc_ref.py's mix_block_up; the multipath alone stays inside the FIR
family's a-priori bound of the f64 convolution; the noise has the stated moments; a seek continues the sequence."""
import numpy as np
import pytest

import channel_ref as cr
import osc_ref as orf
from gpu_util import fir_bound

F = np.float32


@pytest.mark.parametrize("vco", [False, True])
@pytest.mark.parametrize("L", [1, 2, 5, 17])
def test_the_two_forms_agree_across_uneven_calls(L, vco):
    C = 3
    cuts = [0, 1, max(L - 2, 0), L - 1, 130]
    x = cr.streams(sum(cuts), C, 3 + L)
    a, b, whole = (cr.ChannelRef(C, L, vco) for _ in range(3))
    for o in (a, b, whole):
        cr.configure(o, C, L)
        o.seed = 77
    at, ya_, yb = 0, [], []
    for n in cuts:
        ya_.append(a.execute_seq(x[at:at + n]))
        yb.append(b.execute_block(x[at:at + n]))
        at += n
    ya_, yb = np.concatenate(ya_), np.concatenate(yb)
    assert cr.same_words(ya_, yb)
    assert cr.same_words(yb, whole.execute_block(x)), "one call differs from the cut stream"
    assert a.theta == b.theta == whole.theta and a.t == b.t == whole.t
    assert cr.same_words(a.win, b.win) and cr.same_words(b.win, whole.win)


def test_the_bcast_form_is_the_same_stream_into_every_link():
    C, L = 3, 4
    x = cr.streams(50, 1, 9)[:, 0]
    a, b = cr.ChannelRef(C, L), cr.ChannelRef(C, L)
    for o in (a, b):
        cr.configure(o, C, L)
    assert cr.same_words(a.execute_block(x), b.execute_seq(np.repeat(x[:, None], C, axis=1)))


def _ulp32(v):
    """the spacing of f32 at |v| (v an f64 array); the smallest normal's below it"""
    _, e = np.frexp(np.abs(v))
    return np.ldexp(1.0, np.maximum(e, -125) - 24)


def test_cos_sin_words_on_all_arguments():
    worst = -np.inf
    for lo in range(0, 1 << 24, 1 << 22):
        k2 = np.arange(lo, lo + (1 << 22), dtype=np.int64)
        c, s = cr.cos_sin64(k2)
        arg = k2.astype(np.float64) * (2.0 * np.pi / 2.0 ** 24)
        for word, true in ((c.astype(F), np.cos(arg)), (s.astype(F), np.sin(arg))):
            err = np.abs(word.astype(np.float64) - true)
            slack = err - (0.5 * _ulp32(true) + cr.COSSIN_E)
            worst = max(worst, float(slack.max()))
            assert (slack <= 0).all(), (lo, int(k2[np.argmax(slack)]), float(slack.max()))
        assert np.abs(c - np.cos(arg)).max() <= cr.COSSIN_E and np.abs(s - np.sin(arg)).max() <= cr.COSSIN_E
    print("largest |word - true| - (ulp/2 + E):", worst)


def test_cos_sin_exact_points():
    c, s = cr.cos_sin64(np.array([0, 1 << 22, 1 << 23, 3 << 22]))
    assert cr.same_words(c.astype(F), np.array([1, 0, -1, 0], F)), c
    assert cr.same_words(s.astype(F), np.array([0, 1, 0, -1], F)), s
    assert list(np.signbit(c)) == [False, False, True, False]
    assert list(np.signbit(s)) == [False, False, False, True]


def test_radius_ends():
    r = cr.radius(np.array([1, 1 << 23, 1 << 24]))
    assert r[0] == F(np.sqrt(24 * np.log(2.0))) and r[1] == F(np.sqrt(np.log(2.0)))
    assert r[2] == 0 and np.signbit(r[2]), "k1 = 2^24 gives -0, which is kept"


@pytest.mark.parametrize("L", [1, 6])
def test_a_delta_channel_is_the_identity(L):
    x = cr.streams(200, 2, 1)
    assert np.isfinite(x.view(F)).all()
    for vco in (False, True):
        r = cr.ChannelRef(2, L, vco)
        assert cr.same_words(r.execute_block(x), x) and cr.same_words(cr.ChannelRef(2, L, vco).execute_seq(x), x)


@pytest.mark.parametrize("vco", [False, True])
def test_offset_alone_is_mix_block_up(vco):
    x = cr.streams(300, 1, 4)[:, 0]
    r, o = cr.ChannelRef(1, 1, vco), orf.OscRef(vco)
    r.set_carrier_offset(0, 0.37, 6.28)
    o.set_frequency(0.37), o.set_phase(6.28)
    for lo, hi in ((0, 7), (7, 300)):
        assert cr.same_words(r.execute_block(x[lo:hi])[:, 0], o.mix_block_up(x[lo:hi]))
    assert r.theta[0] == o.theta


def test_multipath_alone_within_the_fir_bound():
    L, n = 17, 400
    rng = np.random.default_rng(8)
    h = ((rng.standard_normal(L) + 1j * rng.standard_normal(L)) / np.sqrt(L)).astype(np.complex64)
    x = cr.streams(n, 1, 5)[:, 0]
    r = cr.ChannelRef(1, L)
    r.set_multipath(0, h)
    y = r.execute_block(x)[:, 0]
    truth = np.convolve(x.astype(np.complex128), h.astype(np.complex128))[:n]
    err, bound = float(np.abs(y - truth).max()), fir_bound("cccf", h, x)
    print("multipath max |y - f64|:", err, "bound:", bound)
    assert err <= bound


def test_noise_moments():
    N = 1 << 20
    t = np.arange(N, dtype=np.uint64)
    n0, n1 = (np.empty(N, np.complex128) for _ in range(2))
    for out, link in ((n0, 0), (n1, 1)):
        re, im = cr.noise(2024, link, t)
        out.real, out.imag = re, im
    for n in (n0, n1):
        power, mre, mim = float(np.mean(np.abs(n) ** 2)), float(np.mean(n.real)), float(np.mean(n.imag))
        lag1 = abs(np.mean(n[1:] * np.conj(n[:-1])))
        print("power - 1:", power - 1, "mean:", mre, mim, "lag 1:", lag1)
        assert abs(power - 1) <= 5 * 2.0 ** -10
        assert abs(mre) <= 5 * np.sqrt(0.5 / N) and abs(mim) <= 5 * np.sqrt(0.5 / N)
        assert lag1 <= 5 / np.sqrt(N)
    cross = abs(np.mean(n0 * np.conj(n1)))
    print("cross:", cross)
    assert cross <= 5 / np.sqrt(N)


def test_set_position_beyond_2_32_continues_the_sequence():
    """a run that crosses t = 2^32 equals a seek to the far side"""
    start, n = (1 << 32) - 5, 12
    a, b = cr.ChannelRef(1), cr.ChannelRef(1)
    for o in (a, b):
        o.set_gain_noise(0, 1.0, 0.5)
        o.seed = 3
    x = cr.streams(n, 1, 6)
    a.set_position(0, start)
    ya_ = a.execute_block(x)
    b.set_position(0, start + 7)
    assert b.t[0] > 1 << 32
    assert cr.same_words(b.execute_seq(x[7:]), ya_[7:])
    re, im = cr.noise(3, 0, np.array([(1 << 32) + 1], np.uint64))
    assert ya_[6, 0].real == x[6, 0].real * F(1.0) + F(0.5) * re[0] and ya_[6, 0].imag == x[6, 0].imag * F(1.0) + F(0.5) * im[0]
    lo, _ = cr.noise(3, 0, np.array([1], np.uint64))
    assert lo[0] != re[0], "the counter's high word takes part"
