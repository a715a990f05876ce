"""Restatement of the reference's Osc (src/nco/osc.rs, nco.rs, vco.rs) for tests only.  The tables are built with
libm's sinf through ctypes in the reference's order; phases are int64 masked to 32 bits; every f32 operation is a
separate, unfused numpy float32 operation (or, for long blocks, a separate real-valued torch op on the device, which
rounds the same way).  Also the reference's spectral-mask check for Spgram (src/utility/test_helpers.rs:19-52,
130-137) and its Hann window (src/math/windows.rs:100-106)."""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.sinf.restype, _libm.sinf.argtypes = ctypes.c_float, [ctypes.c_float]
_libm.cosf.restype, _libm.cosf.argtypes = ctypes.c_float, [ctypes.c_float]
_libm.atan2f.restype, _libm.atan2f.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]

PI = f32(np.pi)                 # std::f32::consts::PI
TWO_PI = f32(2.0) * PI
TWO32 = f32(4294967296.0)       # (1u64 << 32) as f32 == u32::MAX as f32
MASK = 0xFFFFFFFF


def sinf(x):
    return f32(_libm.sinf(float(f32(x))))


def cosf(x):
    return f32(_libm.cosf(float(f32(x))))


def atan2f(y, x):
    return f32(_libm.atan2f(float(f32(y)), float(f32(x))))


def _nco_table():                                             # nco.rs:19-28
    return np.array([sinf(TWO_PI * f32(i) / f32(1024)) for i in range(1024)], f32)


def _vco_table():                                             # vco.rs:34-77
    def fp_sin(th):
        return sinf(f32(th) * PI / f32(2147483648.0))
    v = np.zeros(1024, f32)
    s = np.zeros(1024, f32)
    th, dth = 0, MASK // 1024
    for i in range(256):
        value = fp_sin(th)
        skew = (fp_sin(th + dth) - value) / f32(dth)
        v[i], s[i] = value, skew
        v[i + 512], s[i + 512] = -value, -skew
        th = (th + dth) & MASK
    v[256] = f32(1.0)
    s[256] = -s[255]
    v[768] = -v[256]
    s[768] = s[255]
    for i in range(1, 256):
        k = i + 256
        value, skew = v[256 - i], s[256 - i - 1]
        v[k], s[k] = value, -skew
        v[k + 512], s[k + 512] = -value, skew
    return v, s


NCO_TAB = _nco_table()
VCO_V, VCO_S = _vco_table()


def constrain(theta):
    """osc.rs:191-201; None where the reference's loops never end"""
    t = f32(theta)
    while t >= TWO_PI:
        n = f32(t - TWO_PI)
        if n == t:
            return None
        t = n
    while t < f32(0.0):
        n = f32(t + TWO_PI)
        if n == t:
            return None
        t = n
    v = f32(t / TWO_PI) * TWO32
    if not v > 0:                                             # NaN, +-0: Rust's `as u32` gives 0
        return 0
    if v >= TWO32:                                            # saturates
        return MASK
    return int(v)


def sin_cos_words(vco, th):
    """vectorised sin_cos (nco.rs:41-51, vco.rs:99-108) of uint64/int64 phase words < 2^32 -> (sin, cos) float32"""
    th = np.asarray(th, np.int64)
    if not vco:
        i = ((th + (1 << 21)) >> 22) & 1023
        return NCO_TAB[i], NCO_TAB[(i + 256) & 1023]
    i = th >> 22
    j = (i + 256) & 1023
    acc = (th & 0x3FFFFF).astype(f32)
    return VCO_V[i] + acc * VCO_S[i], VCO_V[j] + acc * VCO_S[j]


def mix_words(vco, th, x, down):
    """x * (cos + i sin) (or its conjugate) per sample, num_complex's Mul, unfused"""
    s, c = sin_cos_words(vco, th)
    if down:
        s = -s
    xr, xi = np.real(x).astype(f32), np.imag(x).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):       # large inputs overflow to inf, as on the device
        re = xr * c - xi * s
        im = xr * s + xi * c
    y = np.empty(len(re), np.complex64)
    y.real, y.imag = re, im
    return y


def phase_words(theta0, d_theta, n, first=0):
    return (theta0 + (np.arange(n, dtype=np.int64) + first) * d_theta) & MASK


def mix_block_torch(vco, theta0, d_theta, x_dev, down):
    """the same on the device for long blocks: separate real-valued torch ops (int64 phases, gathers, f32 mul/add)"""
    import torch
    dev = x_dev.device
    n = x_dev.numel()
    th = (theta0 + torch.arange(n, dtype=torch.int64, device=dev) * d_theta) & MASK
    xr, xi = x_dev.real.contiguous(), x_dev.imag.contiguous()
    if not vco:
        tab = torch.from_numpy(NCO_TAB).to(dev)
        i = ((th + (1 << 21)) >> 22) & 1023
        s = tab[i]
        c = tab[(i + 256) & 1023]
        del i
    else:
        tv, ts = torch.from_numpy(VCO_V).to(dev), torch.from_numpy(VCO_S).to(dev)
        i = th >> 22
        acc = (th & 0x3FFFFF).to(torch.float32)
        s = torch.add(tv[i], torch.mul(acc, ts[i]))
        i = (i + 256) & 1023
        c = torch.add(tv[i], torch.mul(acc, ts[i]))
        del i, acc
    del th
    if down:
        s = torch.neg(s)
    re = torch.sub(torch.mul(xr, c), torch.mul(xi, s))
    im = torch.add(torch.mul(xr, s), torch.mul(xi, c))
    return torch.complex(re, im)


class OscRef:
    """nco::Osc, one sample at a time, u32 state as Python ints"""

    def __init__(self, vco):
        self.vco = bool(vco)
        self.theta = self.d_theta = 0
        self.pll_set_bandwidth(0.1)

    def reset(self):
        self.theta = self.d_theta = 0

    def set_frequency(self, f):
        self.d_theta = constrain(f)

    def adjust_frequency(self, df):
        self.d_theta = (self.d_theta + constrain(df)) & MASK

    def set_phase(self, p):
        self.theta = constrain(p)

    def adjust_phase(self, dp):
        self.theta = (self.theta + constrain(dp)) & MASK

    def step(self):
        self.theta = (self.theta + self.d_theta) & MASK

    def get_phase(self):
        return TWO_PI * f32(self.theta) / TWO32

    def get_frequency(self):
        d = TWO_PI * f32(self.d_theta) / TWO32
        return d - TWO_PI if d > PI else d

    def sin_cos(self):
        s, c = sin_cos_words(self.vco, np.array([self.theta]))
        return f32(s[0]), f32(c[0])

    def sin(self):
        return self.sin_cos()[0]

    def cos(self):
        return self.sin_cos()[1]

    def cexp(self):
        s, c = self.sin_cos()
        return np.complex64(complex(c, s))

    def pll_set_bandwidth(self, bw):
        if bw < 0:
            raise ValueError("Bandwidth must be positive")
        self.alpha = f32(bw)
        self.beta = f32(np.sqrt(f32(bw), dtype=f32))

    def pll_step(self, dphi):
        self.adjust_frequency(f32(dphi) * self.alpha)
        self.adjust_phase(f32(dphi) * self.beta)

    def mix_up(self, x):
        return mix_words(self.vco, np.array([self.theta]), np.array([x], np.complex64), False)[0]

    def mix_down(self, x):
        return mix_words(self.vco, np.array([self.theta]), np.array([x], np.complex64), True)[0]

    def mix_block(self, x, down):
        x = np.asarray(x, np.complex64)
        y = mix_words(self.vco, phase_words(self.theta, self.d_theta, len(x)), x, down)
        self.theta = (self.theta + len(x) * self.d_theta) & MASK
        return y

    def mix_block_up(self, x):
        return self.mix_block(x, False)

    def mix_block_down(self, x):
        return self.mix_block(x, True)


def phase_error(r, v):
    """(r * v.conj()).arg() in f32 (osc.rs:246)"""
    rr, ri, vr, vi = f32(r.real), f32(r.imag), f32(v.real), -f32(v.imag)
    re = rr * vr - ri * vi
    im = rr * vi + ri * vr
    return atan2f(im, re)


def pll_error(a, b):                                          # osc.rs:217-226
    e = f32(a) - f32(b)
    while e >= TWO_PI:
        e = e - TWO_PI
    while e <= -TWO_PI:
        e = e + TWO_PI
    return e


def hann(i, wlen):                                            # windows.rs:100-106
    return f32(0.5) - f32(0.5) * cosf((f32(2.0) * PI * f32(i)) / f32(wlen - 1))


def validate_psd_spectrum(psd, nfft, regions):                # test_helpers.rs:19-52
    """regions: (fmin, fmax, pmin, pmax, test_lo, test_hi)"""
    psd = np.asarray(psd, f32)
    f = np.arange(nfft, dtype=f32) / f32(nfft) - f32(0.5)
    fail = np.zeros(nfft, bool)
    for fmin, fmax, pmin, pmax, lo, hi in regions:
        if fmin < -0.5 or fmax > 0.5 or fmin > fmax:
            raise ValueError("invalid frequency range")
        sel = (f >= f32(fmin)) & (f <= f32(fmax))
        if lo:
            fail |= sel & (psd < f32(pmin))
        if hi:
            fail |= sel & (psd > f32(pmax))
    return not fail.any()


def validate_psd_spgramcf(spgram, regions):                   # test_helpers.rs:130-137
    return validate_psd_spectrum(spgram.get_psd(), spgram.get_nfft(), regions)
