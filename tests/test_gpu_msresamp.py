"""MsResamp through the C ABI -- mirrors src/filter/resampler/msresamp.rs:28-176 and its tests (:178-337).

MsResamp is a composition (MsResamp2 half-band stages around a Resamp), so the sample-level check is against the two
parts built separately and chained by hand; the counts follow the reference's formulas; the spectral tests drive
band-limited Gaussian noise instead of the reference's SymStreamR (framing code, out of scope) and keep its regions."""
import math

import numpy as np
import pytest

from gpu_util import rand_samples
from resamp_util import loop_count, rust_step

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 20, 7, 64, 4, 4, 4, 27]                 # msresamp.rs:267


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


def stages(rate):
    """msresamp.rs:33-51 in f32: (interp, number of half-band stages, arbitrary rate)"""
    ra, s = np.float32(rate), 0
    interp = ra > np.float32(1.0)
    if interp:
        while ra > np.float32(2.0):
            s, ra = s + 1, np.float32(ra * np.float32(0.5))
    else:
        while ra < np.float32(0.5):
            s, ra = s + 1, np.float32(ra * np.float32(2.0))
    return int(interp), s, ra


def test_config_and_getters(ya):
    for bad in (0.0, -1.0):
        with pytest.raises(ya.ConfigError):
            ya.MsResamp("crcf", bad, 60.0)
    for rate in (1.0, 1e3, 1e-3, 0.127115323, 7.3):
        q = ya.MsResamp("crcf", rate, 60.0)
        assert q.get_rate() == np.float32(rate)
        assert q.get_params() == stages(rate)


@pytest.mark.parametrize("rate", [1.0, 1e3, 1e-3, math.sqrt(2), math.sqrt(17), 1 / math.pi, math.exp(8), math.exp(-8)])
def test_num_output(ya, rate):
    """msresamp.rs:258-313 (num_output_0 .. 7): get_num_output(n) == nw of execute, and both equal the reference's
    formula (:109-120) over the arbitrary resampler's loop, the size sequence (x131 below rate 0.1) run 8 times"""
    rate = float(np.float32(rate))
    q = ya.MsResamp("crcf", rate, 60.0)
    interp, s, ra = stages(rate)
    step, phase, carry = rust_step(ra), 0, 0
    scale = 131 if rate < 0.1 else 1
    for _ in range(8):
        for size in SIZES:
            n = size * scale
            if interp:
                cnt, phase = loop_count(phase, step, n)
                want = cnt << s
            else:
                groups, carry = (carry + n) >> s, (carry + n) & ((1 << s) - 1)
                want, phase = loop_count(phase, step, groups)
            assert q.get_num_output(n) == want
            assert len(q.execute(np.zeros(n, np.complex64))) == want


def test_copy(ya):
    """msresamp.rs:315-337 (msresamp_crcf_copy): clone after one block of 640, equal outputs for the next"""
    rng = np.random.default_rng(3)
    q0 = ya.MsResamp("crcf", float(np.float32(0.071239213987520)), 60.0)
    q0.execute(rand_samples(rng, "crcf", 640))
    q1 = q0.clone()
    x = rand_samples(rng, "crcf", 640)
    y0, y1 = q0.execute(x), q1.execute(x)
    assert len(y0) == len(y1) > 0
    assert np.array_equal(y0, y1)


@pytest.mark.parametrize("rate", [1.0, 0.9, 0.3, 1e-3, 1.7, 7.3, 1e3])
def test_get_delay(ya, rate):
    """msresamp.rs:87-103 from the delays of separately built parts"""
    interp, s, ra = stages(rate)
    q = ya.MsResamp("crcf", rate, 60.0)
    dh = ya.MsResamp2("crcf", interp, s, 0.4, 0.0, 60.0).get_delay() if s else np.float32(0)
    dh, da = np.float32(dh), np.float32(7)
    if s == 0:
        want = da
    elif interp:
        want = np.float32(dh / ra) + da
    else:
        want = dh + np.float32(1 << s) * da
    assert q.get_delay() == np.float32(want)


class HandChain:
    """MsResamp2(type, S, 0.4, 0, as) and Resamp(ra, 7, min(0.515 ra, 0.49), as, 256) chained by hand on device buffers,
    the decimator's leftover inputs carried on the host"""

    def __init__(self, ya, kind, rate, as_):
        self.ya, self.interp, self.s, ra = ya, *stages(rate)
        self.dt = np.complex64 if kind != "rrrf" else np.float32
        self.half = ya.MsResamp2(kind, self.interp, self.s, 0.4, 0.0, as_)
        self.arb = ya.Resamp(kind, float(ra), 7, float(min(np.float32(0.515) * ra, np.float32(0.49))), as_, 256)
        self.carry = np.zeros(0, self.dt)

    def execute(self, x):
        ya, R = self.ya, 1 << self.s
        if self.interp:
            n1 = self.arb.get_num_output(len(x))
            md = ya.DeviceArray(max(n1, 1), self.dt)
            assert self.arb.execute_block_dev(ya.DeviceArray.from_numpy(x), len(x), md, n1) == n1
            if self.s == 0:
                return md.to_numpy(n1)
            yd = ya.DeviceArray(max(n1 * R, 1), self.dt)
            if n1:
                self.half.execute_block_dev(md, n1, yd)
            return yd.to_numpy(n1 * R)
        xs = np.concatenate([self.carry, x])
        g = len(xs) // R
        self.carry = xs[g * R:].copy()
        if g == 0:
            return np.zeros(0, self.dt)
        md = ya.DeviceArray(g, self.dt)
        if self.s:
            self.half.execute_block_dev(ya.DeviceArray.from_numpy(xs[: g * R]), g, md)
        else:
            md = ya.DeviceArray.from_numpy(xs[:g])
        ny = self.arb.get_num_output(g)
        yd = ya.DeviceArray(max(ny, 1), self.dt)
        assert self.arb.execute_block_dev(md, g, yd, ny) == ny
        return yd.to_numpy(ny)


@pytest.mark.parametrize("kind,rate", [("crcf", 0.127115323), ("crcf", 0.03), ("cccf", 0.676543210), ("rrrf", 0.2),
                                       ("crcf", 7.3), ("cccf", 2.9), ("rrrf", 1.3), ("crcf", 37.0)])
def test_composition(ya, kind, rate):
    """execute_dev == the separately built parts chained by hand, bit for bit, with ragged call lengths that leave
    every carry length of the decimator"""
    rng = np.random.default_rng(int(rate * 1000))
    rate = float(np.float32(rate))
    q = ya.MsResamp(kind, rate, 60.0)
    hand = HandChain(ya, kind, rate, 60.0)
    cuts = [1, 3, 7, 100, 2, 1000, 5, 64, 4097, 13, 31, 1, 20000, 6, 257]
    for n in cuts:
        x = rand_samples(rng, kind, n)
        ny = q.get_num_output(n)
        xd, yd = ya.DeviceArray.from_numpy(x), ya.DeviceArray(max(ny, 1), x.dtype)
        assert q.execute_dev(xd, n, yd, ny) == ny
        got = yd.to_numpy(ny)
        want = hand.execute(x)
        assert got.shape == want.shape, n
        assert np.array_equal(got, want), n
    with pytest.raises(ya.RangeError):
        x = np.zeros(5000, np.float32 if kind == "rrrf" else np.complex64)
        need = q.get_num_output(5000)
        q.execute_dev(ya.DeviceArray.from_numpy(x), 5000, ya.DeviceArray(max(need, 1), x.dtype), need - 1)


def band_noise(rng, n, r, bw):
    """complex Gaussian noise with a flat PSD of 1/r for |f| <= 0.4 r bw, a raised-cosine edge to 0 at 0.55 r bw
    (periodic: shaped in the frequency domain), so that after resampling by r the band +-0.4 bw sits at 0 dB"""
    f = np.fft.fftfreq(n)
    a = np.abs(f) / (r * bw)
    mask = np.where(a <= 0.4, 1.0, np.where(a >= 0.55, 0.0, 0.5 + 0.5 * np.cos(np.pi * (a - 0.4) / 0.15)))
    w = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
    return (np.fft.ifft(np.fft.fft(w) * mask) * np.sqrt(1.0 / r)).astype(np.complex64)


def welch_db(y, nfft=800):
    """the reference's Spgram(nfft, Hann, nfft/2, nfft/4) estimate: Hann frames of nfft/2, hop nfft/4, zero-padded to
    nfft, mean |X|^2 / sum w^2, fft-shifted, in dB"""
    wl, hop = nfft // 2, nfft // 4
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(wl) / (wl - 1))
    nf = (len(y) - wl) // hop + 1
    idx = np.arange(wl)[None, :] + hop * np.arange(nf)[:, None]
    fr = np.zeros((nf, nfft), np.complex128)
    fr[:, :wl] = y[idx] * w
    p = np.mean(np.abs(np.fft.fft(fr, axis=1)) ** 2, axis=0) / np.sum(w ** 2)
    return 10 * np.log10(np.fft.fftshift(p)), np.arange(nfft) / nfft - 0.5


@pytest.mark.parametrize("r", [0.127115323, 0.373737373, 0.676543210])
def test_spectral_mask(ya, r, as_=60.0):
    """msresamp.rs:212-256 (msresamp_crcf_01 .. 03): 800 000 output samples, PSD in +-0.4 bw within +-0.5 dB,
    beyond +-0.6 bw below -as + 0.5 dB"""
    bw, tol, n_out = 0.2, 0.5, 800000
    rng = np.random.default_rng(11)
    r = float(np.float32(r))
    x = band_noise(rng, int(n_out / r) + 4096, r, bw)
    q = ya.MsResamp("crcf", r, as_)
    y = np.concatenate([q.execute(x[i:i + (1 << 20)]) for i in range(0, len(x), 1 << 20)])
    assert len(y) >= n_out
    psd, f = welch_db(y[:n_out])
    inb = np.abs(f) <= 0.4 * bw
    out = np.abs(f) >= 0.6 * bw
    assert np.all(np.abs(psd[inb]) <= tol), (psd[inb].min(), psd[inb].max())
    assert np.all(psd[out] <= -as_ + tol), psd[out].max()
