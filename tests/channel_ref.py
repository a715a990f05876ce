"""Channel restated in numpy (include/yagi_hip.h, "Channel: the definition"), in two forms that must agree bit for bit: a
per-sample sequential loop (window push, inner product, mix_up and step, gain and noise, t += 1) and a block form with the
closed-form phase theta + (u32)j d_theta and counter t + j.  The words of channel_words.hpp are restated here too: the
counter-based SplitMix64 draws, R = (float)sqrt(-ln64(k1 2^-24)) and the octant-reduced f64 polynomials of cos and sin.
numpy's f64 and f32 + - * / sqrt are IEEE operations rounded one by one, which is all the definition uses."""
import math

import numpy as np

import agc_ref as ar
import osc_ref as orf

F = np.float32
U64 = np.uint64
CHANNELS_MAX = 1 << 20          # YAGI_CHANNEL_CHANNELS_MAX
TAPS_MAX = 64                   # YAGI_CHANNEL_TAPS_MAX
COSSIN_E = 2.0 ** -45           # YAGI_CHANNEL_COSSIN_E
STEP = float.fromhex("0x1.921fb54442d18p-22")     # fl64(2 pi) 2^-24
SIN_COEF = [s / math.factorial(k) for k, s in ((15, -1.0), (13, 1.0), (11, -1.0), (9, 1.0), (7, -1.0), (5, 1.0), (3, -1.0))]
COS_COEF = [s / math.factorial(k) for k, s in ((16, 1.0), (14, -1.0), (12, 1.0), (10, -1.0), (8, 1.0), (6, -1.0), (4, 1.0),
                                                (2, -1.0))]
same_words = ar.same_words


# ---- the words ---------------------------------------------------------------------------------------------------------
def splitmix64_at(seed, idx):
    """word idx of the sequence of seed: u64 arithmetic, wrapping (arrays wrap silently)"""
    seed, idx = np.atleast_1d(np.asarray(seed, U64)), np.atleast_1d(np.asarray(idx, U64))
    z = seed + (idx + U64(1)) * U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def ln64(x):
    """agc_ref.ln64 on an array of positive finite f64"""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)
    m, e = m * 2.0, e - 1
    big = m >= ar.SQRT2
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = np.full_like(z, ar.LN_COEF[0])
    for c in ar.LN_COEF[1:]:
        p = p * z + c
    return e.astype(np.float64) * ar.LN2 + (2.0 * s) * p


def radius(k1):
    """R[k1], k1 in 1 .. 2^24; k1 = 2^24 gives -0"""
    x = np.asarray(k1, np.int64).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-ln64(x)).astype(F)


def cos_sin64(k2):
    """the f64 evaluations (C, S) of cos and sin(2 pi k2 / 2^24), k2 in [0, 2^24)"""
    k2 = np.asarray(k2, np.int64)
    octant, r = k2 >> 21, k2 & 0x1FFFFF
    odd = (octant & 1) != 0
    m = np.where(odd, 0x200000 - r, r)
    x = m.astype(np.float64) * STEP
    z = x * x
    p = np.full_like(z, SIN_COEF[0])
    for c in SIN_COEF[1:]:
        p = p * z + c
    sn = x + (x * z) * p
    q = np.full_like(z, COS_COEF[0])
    for c in COS_COEF[1:]:
        q = q * z + c
    cs = 1.0 + z * q
    ss = np.where(odd, 0.0 - sn, sn)
    quad = ((octant + 1) >> 1) & 3
    C = np.select([quad == 0, quad == 1, quad == 2], [cs, 0.0 - ss, 0.0 - cs], ss)
    S = np.select([quad == 0, quad == 1, quad == 2], [ss, cs, 0.0 - ss], 0.0 - cs)
    return C, S


def noise(seed, link, t):
    """the noise samples (R C, R S) of (seed, link) at the counters t (u64 array) -> (re, im) float32"""
    t = np.atleast_1d(np.asarray(t, U64))
    seed_c = splitmix64_at(seed, link)
    a, b = splitmix64_at(seed_c, U64(2) * t), splitmix64_at(seed_c, U64(2) * t + U64(1))
    k1, k2 = (a >> U64(40)).astype(np.int64) + 1, (b >> U64(40)).astype(np.int64)
    R = radius(k1)
    c, s = cos_sin64(k2)
    return R * c.astype(F), R * s.astype(F)


def p10(t):
    """(float)exp64((double)t ln 10) of an f32 t; a NaN stays"""
    t = F(t)
    if t != t:
        return t
    with np.errstate(all="ignore"):
        return F(ar.exp64(float(t) * ar.LN10))


def awgn_words(n0_db, snr_db):
    """(gamma, nstd) of set_awgn: the arguments are formed in f32"""
    with np.errstate(all="ignore"):
        n0, snr = F(n0_db), F(snr_db)
        return p10((snr + n0) / F(20.0)), p10(n0 / F(20.0))


# ---- the object --------------------------------------------------------------------------------------------------------
def _cmul_add(acc_r, acc_i, hr, hi, xr, xi):
    """acc + h x: num-complex's product, every product and add rounded on its own in f32"""
    rr, ii, ri, ir = hr * xr, hi * xi, hr * xi, hi * xr
    return acc_r + (rr - ii), acc_i + (ri + ir)


class ChannelRef:
    def __init__(self, channels, L=1, vco=False):
        self.C, self.L, self.vco = channels, L, bool(vco)
        self.h = np.zeros((channels, L), np.complex64)
        self.h[:, 0] = 1
        self.gamma, self.nstd = np.ones(channels, F), np.zeros(channels, F)
        self.theta, self.d_theta, self.phi = ([0] * channels for _ in range(3))
        self.t = [0] * channels
        self.seed = 0
        self.win = np.zeros((L - 1, channels), np.complex64)            # oldest first

    # parameters
    def set_awgn(self, c, n0_db, snr_db):
        self.gamma[c], self.nstd[c] = awgn_words(n0_db, snr_db)

    def set_gain_noise(self, c, gamma, nstd):
        self.gamma[c], self.nstd[c] = F(gamma), F(nstd)

    def set_carrier_offset(self, c, dphi, phi=0.0):
        d, p = orf.constrain(dphi), orf.constrain(phi)
        if d is None or p is None:
            raise ar.ConfigError("constrain() would not end")
        self.d_theta[c], self.theta[c], self.phi[c] = d, p, p

    def set_multipath(self, c, h):
        self.h[c] = np.asarray(h, np.complex64)

    def set_position(self, c, t):
        self.t[c] = int(t)

    def reset_channel(self, c):
        self.win[:, c] = 0
        self.t[c] = 0
        self.theta[c] = self.phi[c]

    def reset(self):
        for c in range(self.C):
            self.reset_channel(c)

    def _input(self, x):
        x = np.asarray(x, np.complex64)
        if x.ndim == 1:                                                 # the broadcast form
            x = np.repeat(x[:, None], self.C, axis=1)
        assert x.ndim == 2 and x.shape[1] == self.C
        return x

    def _finish(self, c, v, theta, t):
        """mix_up at the phases theta, gain and noise at the counters t, for the samples v of link c"""
        w = orf.mix_words(self.vco, theta, v, False)
        nr, ni = noise(self.seed, c, t)
        y = np.empty(len(v), np.complex64)
        with np.errstate(all="ignore"):
            y.real = w.real * self.gamma[c] + self.nstd[c] * nr
            y.imag = w.imag * self.gamma[c] + self.nstd[c] * ni
        return y

    # form 1: the sequential loop
    def execute_seq(self, x):
        x = self._input(x)
        y = np.zeros(x.shape, np.complex64)
        L = self.L
        for c in range(self.C):
            hrev = self.h[c, ::-1]
            win = list(self.win[:, c])
            for s in range(x.shape[0]):
                win.append(x[s, c])                                     # push
                ar_, ai_ = F(0.0), F(0.0)
                with np.errstate(all="ignore"):
                    for j in range(L):
                        ar_, ai_ = _cmul_add(ar_, ai_, hrev[j].real, hrev[j].imag, win[j].real, win[j].imag)
                v = np.array([complex(ar_, ai_)], np.complex64)
                v.real, v.imag = ar_, ai_                               # keeps a NaN or Inf part as it is
                y[s, c] = self._finish(c, v, np.array([self.theta[c]], np.int64), np.array([self.t[c]], U64))[0]
                self.theta[c] = (self.theta[c] + self.d_theta[c]) & orf.MASK        # step
                self.t[c] = (self.t[c] + 1) & (2 ** 64 - 1)
                win.pop(0)
            self.win[:, c] = win
        return y

    # form 2: the block form
    def execute_block(self, x):
        x = self._input(x)
        n, L = x.shape[0], self.L
        y = np.zeros(x.shape, np.complex64)
        xx = np.concatenate([self.win, x], axis=0)                      # [L - 1 + n][C]
        j_idx = np.arange(n, dtype=np.int64)
        for c in range(self.C):
            hrev = self.h[c, ::-1]
            col = xx[:, c]
            ar_, ai_ = np.zeros(n, F), np.zeros(n, F)
            with np.errstate(all="ignore"):
                for j in range(L):
                    seg = col[j:j + n]
                    ar_, ai_ = _cmul_add(ar_, ai_, hrev[j].real, hrev[j].imag, seg.real, seg.imag)
            v = np.empty(n, np.complex64)
            v.real, v.imag = ar_, ai_
            theta = (self.theta[c] + j_idx * self.d_theta[c]) & orf.MASK
            t = U64(self.t[c]) + j_idx.astype(U64) if n else np.zeros(0, U64)
            y[:, c] = self._finish(c, v, theta, t)
            self.theta[c] = (self.theta[c] + n * self.d_theta[c]) & orf.MASK
            self.t[c] = (self.t[c] + n) & (2 ** 64 - 1)
        self.win = xx[n:].copy() if L > 1 else self.win
        return y

    def words(self):
        """the arguments of execute_host: h, gamma, nstd, theta, d_theta, t"""
        return (self.h.copy(), self.gamma.copy(), self.nstd.copy(), np.array(self.theta, np.uint32),
                np.array(self.d_theta, np.uint32), np.array(self.t, np.uint64))


def configure(obj, C, L, seed=5):
    """the same varied parameters on a ChannelRef or a yagi_amd.Channel: per link taps, an offset that wraps the phase
    word early, a gain, noise on the even links"""
    r = np.random.default_rng(seed)
    for c in range(C):
        h = ((r.standard_normal(L) + 1j * r.standard_normal(L)) * (0.7 ** np.arange(L))).astype(np.complex64)
        obj.set_multipath(c, h)
        obj.set_carrier_offset(c, float(F(0.05 * (c % 7 + 1) * (-1) ** c)), float(F(6.2 - 0.3 * (c % 5))))
        if c % 2 == 0:
            obj.set_awgn(c, float(F(-20.0 - c % 3)), float(F(10.0 + c % 4)))
        else:
            obj.set_gain_noise(c, float(F(0.5 + 0.25 * (c % 3))), 0.0)


def streams(n, C, seed):
    return ar.noise(seed, n, C)
