"""The reference's Modem (src/modem/modem.rs, src/modem/modem/*.rs) restated in numpy for the schemes the library builds:
per-sample modulate / demodulate / demodulate_soft with every operation a separate np.float32 rounding (a helper, not a
conftest).  The run-time functions take the constellation and the neighbour table as ARGUMENTS, so a test can feed them
the library's own tables and no transcendental rounding of the construction leaks into a comparison; design() builds the
tables the way the reference does.  The reference's sequential f32 DPSK modulator is here as written (RefModem.modulate),
next to the exact running index the library uses instead (dpsk_indices)."""
import math

import numpy as np

f32 = np.float32
PI = f32(math.pi)
TWO_PI = f32(2.0) * PI
SQRT_2 = f32(math.sqrt(2.0))
FRAC_1_SQRT_2 = f32(math.sqrt(0.5))
MAX_BPS = 8

PSK, DPSK, ASK, QAM, BPSK, QPSK, OOK, ARB = "psk", "dpsk", "ask", "qam", "bpsk", "qpsk", "ook", "arb"
# name -> (kind, bps), numbered as ModulationScheme (modem.rs:27-79)
SCHEMES = {}
for _b in range(1, 9):
    SCHEMES[f"Psk{1 << _b}"] = (PSK, _b)
    SCHEMES[f"Dpsk{1 << _b}"] = (DPSK, _b)
    SCHEMES[f"Ask{1 << _b}"] = (ASK, _b)
    if _b >= 2:
        SCHEMES[f"Qam{1 << _b}"] = (QAM, _b)
SCHEMES.update(Bpsk=(BPSK, 1), Qpsk=(QPSK, 2), Ook=(OOK, 1))
UNSUPPORTED = [f"Apsk{1 << b}" for b in range(2, 9)] + ["Sqam32", "Sqam128", "V29", "Arb16Opt", "Arb32Opt", "Arb64Opt",
                                                         "Arb128Opt", "Arb256Opt", "Arb64Vt", "Arb64Ui", "Pi4Dqpsk"]


def gray_encode(s):
    return s ^ (s >> 1)


def gray_decode(s):                                           # modem.rs:521-537
    mask = out = s
    for _ in range(0, MAX_BPS, 4):
        out ^= mask >> 1
        out ^= mask >> 2
        out ^= mask >> 3
        out ^= mask >> 4
        mask >>= 4
    return out


def pack_soft_bits(soft, bps):                                # :543-555
    s = 0
    for b in list(soft)[:bps]:
        s = (s << 1) | (1 if int(b) > 127 else 0)
    return s


def unpack_soft_bits(sym, bps):                               # :561-575
    return np.array([255 if (sym >> (bps - i - 1)) & 1 else 0 for i in range(bps)], np.uint8)


def soft_byte(v):
    """`v.clamp(0.0, 255.0) as u8`: NaN -> 0, truncation toward zero"""
    v = f32(v)
    if np.isnan(v) or v < 0:
        return 0
    return 255 if v > 255 else int(v)


def _polar1(a):
    return complex(f32(np.cos(f32(a))), f32(np.sin(f32(a))))


_ASK_E = [1.0, 5.0, 21.0, 85.0, 341.0, 1365.0, 5461.0, 21845.0]
_QAM_E = {2: 2.0, 3: 6.0, 4: 10.0, 5: 26.0, 6: 42.0, 7: 106.0, 8: 170.0}


class Design:
    """kind, bps, M, alpha, reference[], d_phi, the symbol map and the neighbour table (M x p) of one scheme"""


def neighbours(c, p):
    """init_demod_soft_tab :465-511 on f32 hypot; the mark of an empty slot is out of range (the reference's `M as u8`
    is 0 at M = 256 and would bar symbol 0 from every list)"""
    M = len(c)
    t = -np.ones((M, p), np.int64)
    c = np.asarray(c, np.complex64)
    for i in range(M):
        d = np.hypot((c[i].real - c.real).astype(f32), (c[i].imag - c.imag).astype(f32)).astype(f32)
        for k in range(p):
            dmin, best = f32(1e9), -1
            for j in range(M):
                if i != j and j not in t[i] and d[j] < dmin:
                    dmin, best = d[j], j
            t[i, k] = best
    return t.astype(np.uint8)


def design(kind, bps, table=None):
    D = Design()
    D.kind, D.bps, D.M = kind, bps, 1 << bps
    M = D.M
    D.alpha, D.d_phi, D.p, D.gamma = f32(0), f32(0), 0, f32(0)
    m = np.zeros(M, np.complex64)
    if kind in (PSK, DPSK):
        D.alpha = PI / f32(M)
        D.d_phi = PI * (f32(1) - f32(1) / f32(M))
        for i in range(M):
            sd = gray_decode(i) if kind == PSK else i
            m[i] = _polar1(f32(sd) * f32(2) * D.alpha)
        D.p = 2 if kind == PSK and bps >= 3 else 0
    elif kind == ASK:
        D.alpha = f32(1) if bps == 1 else f32(1) / np.sqrt(f32(_ASK_E[bps - 1]))
        for i in range(M):
            m[i] = f32(2 * gray_decode(i) - M + 1) * D.alpha
        D.p = 2 if 2 <= bps < 8 else 0
    elif kind == QAM:
        D.alpha = f32(1) / np.sqrt(f32(_QAM_E[bps]))
        mi, mq = (bps + 1) >> 1, bps >> 1
        for i in range(M):
            si, sq = gray_decode(i >> mq), gray_decode(i & ((1 << mq) - 1))
            m[i] = complex(f32(2 * si - (1 << mi) + 1) * D.alpha, f32(2 * sq - (1 << mq) + 1) * D.alpha)
        D.p = 3 if bps == 3 else 4 if bps >= 4 else 0
    elif kind == BPSK:
        m[:] = [1, -1]
    elif kind == QPSK:
        m[:] = [complex(FRAC_1_SQRT_2 if (i & 1) == 0 else -FRAC_1_SQRT_2, FRAC_1_SQRT_2 if (i & 2) == 0 else -FRAC_1_SQRT_2)
                for i in range(4)]
    elif kind == OOK:
        m[:] = [SQRT_2, 0]
    elif kind == ARB:                                         # arb.rs:4-13, 76-94
        t = np.asarray(table, np.complex64)
        sr = si = f32(0)
        for v in t:
            sr, si = sr + v.real, si + v.imag
        mr, mi_ = sr / f32(M), si / f32(M)
        e = f32(0)
        for i, v in enumerate(t):
            re, im = f32(v.real - mr), f32(v.imag - mi_)
            m[i] = complex(re, im)
            e = e + (re * re + im * im)
        scale = np.sqrt(e / f32(M))
        m = (m.real / scale).astype(f32) + 1j * (m.imag / scale).astype(f32)
        m = m.astype(np.complex64)
        D.gamma = f32(1.2) * f32(bps)
    else:
        raise ValueError(kind)
    D.ref = np.array([f32(1 << k) * D.alpha for k in range(bps)], f32)
    D.map = m
    D.nbr = neighbours(m, D.p) if D.p else np.zeros((M, 0), np.uint8)
    return D


def _linear(ref, v, m):                                       # demodulate_linear_array_ref :296-315
    s, v = 0, f32(v)
    for k in range(m):
        s <<= 1
        if v > 0:
            s |= 1
            v = v - ref[m - k - 1]
        else:
            v = v + ref[m - k - 1]
    return s, f32(v)


class RefModem:
    """The reference's per-sample object on a Design whose map / nbr may be replaced by the library's own."""

    def __init__(self, D, cmap=None, nbr=None):
        self.D = D
        self.map = np.asarray(D.map if cmap is None else cmap, np.complex64)
        self.nbr = np.asarray(D.nbr if nbr is None else nbr, np.uint8).reshape(D.M, -1)
        self.reset()

    def reset(self):                                          # :218-224
        self.r = self.x_hat = np.complex64(1)
        self.phi = f32(0)          # dpsk.rs: ONE field, the modulator's phase and the demodulator's last angle
        self.k = 0                 # the library's exact modulator index (not in the reference)

    def copy(self):
        c = RefModem(self.D, self.map, self.nbr)
        c.r, c.x_hat, c.phi, c.k = self.r, self.x_hat, self.phi, self.k
        return c

    # -- modulate :243-253
    def modulate(self, s):
        D = self.D
        if s >= D.M:
            raise ValueError("input symbol exceeds constellation size")
        if D.kind == DPSK:                                    # dpsk.rs:50-72, sequential f32 phase as written
            self.phi = self.phi + f32(gray_decode(s)) * f32(2) * D.alpha
            if self.phi > TWO_PI:
                self.phi = self.phi - TWO_PI
            y = np.complex64(_polar1(self.phi))
            self.r = y
            return y
        return self.map[s]

    def get_demodulator_sample(self):
        return self.x_hat

    def get_demodulator_phase_error(self):                    # (r * conj(x_hat)).im
        r, xh = self.r, self.x_hat
        return f32(f32(r.real) * f32(-xh.imag)) + f32(f32(r.imag) * f32(xh.real))

    def get_demodulator_evm(self):
        return f32(np.hypot(f32(self.x_hat.real - self.r.real), f32(self.x_hat.imag - self.r.imag)))

    # -- demodulate :255-257
    def demodulate(self, x, theta=None):
        """theta: atan2 of x where the caller wants to supply it (f64-rounded), else np.arctan2 in f32"""
        D = self.D
        x = np.complex64(x)
        re, im = f32(x.real), f32(x.imag)
        if D.kind in (PSK, DPSK) and theta is None:
            theta = np.arctan2(im, re)
        if D.kind == ASK:
            s, _ = _linear(D.ref, re, D.bps)
            s = gray_encode(s)
            xh = self.map[s]
        elif D.kind == QAM:
            mi, mq = (D.bps + 1) >> 1, D.bps >> 1
            si, ri = _linear(D.ref, re, mi)
            sq, rq = _linear(D.ref, im, mq)
            s = (gray_encode(si) << mq) + gray_encode(sq)
            xh = np.complex64(complex(re - ri, im - rq))
        elif D.kind == PSK:
            t = f32(theta) - D.d_phi
            if t < -PI:
                t = t + TWO_PI
            s, _ = _linear(D.ref, t, D.bps)
            s = gray_encode(s)
            xh = self.map[s]
        elif D.kind == DPSK:
            theta = f32(theta)
            d = theta - self.phi
            self.phi = theta
            d = d - D.d_phi
            if d > PI:
                d = d - TWO_PI
            elif d < -PI:
                d = d + TWO_PI
            s, res = _linear(D.ref, d, D.bps)
            s = gray_encode(s)
            xh = np.complex64(_polar1(theta - res))
        elif D.kind == BPSK:
            s = 0 if re > 0 else 1
            xh = np.complex64(1 if s == 0 else -1)
        elif D.kind == QPSK:
            s = (0 if re > 0 else 1) + (0 if im > 0 else 2)
            xh = np.complex64(complex(FRAC_1_SQRT_2 if (s & 1) == 0 else -FRAC_1_SQRT_2,
                                      FRAC_1_SQRT_2 if (s & 2) == 0 else -FRAC_1_SQRT_2))
        elif D.kind == OOK:
            s = 0 if re > FRAC_1_SQRT_2 else 1
            xh = np.complex64(0 if s else SQRT_2)
        else:                                                 # arb.rs:21-35 (hypot)
            d = np.hypot((re - self.map.real).astype(f32), (im - self.map.imag).astype(f32)).astype(f32)
            s = int(np.argmin(d))                             # first minimum
            xh = self.map[s]
        self.x_hat, self.r = xh, x
        return s

    # -- demodulate_soft :259-271
    def demodulate_soft(self, x, theta=None, fixed=False):
        """fixed=True: Arb's loop with the bit of the CANDIDATE index, which the reference does not do"""
        D = self.D
        x = np.complex64(x)
        re, im = f32(x.real), f32(x.imag)
        bps = D.bps
        if D.kind == BPSK:
            soft = [soft_byte((f32(-2) * re) * f32(4) * f32(16) + f32(127))]
            return self.demodulate(x), np.array(soft, np.uint8)
        if D.kind == QPSK:
            soft = [soft_byte((f32(-2) * im) * f32(5.8) * f32(16) + f32(127)),
                    soft_byte((f32(-2) * re) * f32(5.8) * f32(16) + f32(127))]
            return self.demodulate(x), np.array(soft, np.uint8)
        if D.kind == ARB:                                     # arb.rs:37-74
            d0, d1 = [f32(4)] * bps, [f32(4)] * bps
            dmin, s = f32(np.inf), 0
            for idx in range(D.M):
                c = self.map[idx]
                er, ei = re - f32(c.real), im - f32(c.imag)
                d = er * er + ei * ei
                if d < dmin:
                    dmin, s = d, idx
                t = idx if fixed else s
                for k in range(bps):
                    if (t >> (bps - k - 1)) & 1 == 0:
                        if d < d0[k]:
                            d0[k] = d
                    elif d < d1[k]:
                        d1[k] = d
            soft = [soft_byte(((d0[k] - d1[k]) * D.gamma) * f32(16) + f32(127)) for k in range(bps)]
            self.x_hat, self.r = self.map[s], x
            return s, np.array(soft, np.uint8)
        p = self.nbr.shape[1]
        if p > 0:                                             # demodulate_soft_table :317-364
            s = self.demodulate(x, theta)
            gamma = f32(1.2) * f32(D.M)
            d0, d1 = [f32(8)] * bps, [f32(8)] * bps
            er, ei = re - f32(self.x_hat.real), im - f32(self.x_hat.imag)
            d = er * er + ei * ei
            for k in range(bps):
                if (s >> (bps - k - 1)) & 1:
                    d1[k] = d
                else:
                    d0[k] = d
            for i in range(p):
                nb = int(self.nbr[s, i])
                c = self.map[nb]
                er, ei = re - f32(c.real), im - f32(c.imag)
                d = er * er + ei * ei
                for k in range(bps):
                    if (nb >> (bps - k - 1)) & 1:
                        if d < d1[k]:
                            d1[k] = d
                    elif d < d0[k]:
                        d0[k] = d
            soft = [soft_byte(((d0[k] - d1[k]) * gamma) * f32(16) + f32(127)) for k in range(bps)]
            return s, np.array(soft, np.uint8)
        s = self.demodulate(x, theta)
        return s, unpack_soft_bits(s, bps)


def dpsk_indices(sym, M, k0=0):
    """the library's DPSK modulator: k_n = (k_{n-1} + gray_decode(s_n)) mod M"""
    g = np.array([gray_decode(int(s)) for s in sym], np.int64)
    return (k0 + np.cumsum(g)) % M


def dpsk_truth(sym, M, k0=0):
    """f64 truth of the DPSK modulator's output"""
    return np.exp(2j * np.pi * dpsk_indices(sym, M, k0) / M)


def dpsk_drift_bound(n, M):
    """How far the reference's sequential f32 DPSK modulator and the exact-index form (map[k_n], each table entry within
    2^-21 of truth) may be from f64 truth and so from each other after n symbols: every step rounds the sum (<= 1/2 ulp of a
    value below 4 pi, taken as 2^-21), the step itself carries f32(pi)'s error (k 2^(1-m) |f32(pi) - pi| <= 1.75e-7 per
    step), a wrap subtracts f32(2 pi), which is again off by 1.75e-7 and happens at most once per step; then one ulp of
    sin / cos (2^-22) and the table's 2^-21."""
    per_step = 2.0 ** -21 + 2 * 1.75e-7
    return n * per_step + 2.0 ** -22 + 2.0 ** -21


# ---- the same arithmetic on whole arrays (every numpy op on float32 arrays is one rounding per element) ---------------
# tests/test_modem_ref_cpu.py holds these to RefModem bit for bit; the GPU tests use them for speed.
def _linear_v(ref, v, m):
    s = np.zeros(v.shape, np.int64)
    v = v.astype(f32)
    for k in range(m):
        pos = v > 0
        s = (s << 1) | pos
        v = np.where(pos, v - ref[m - k - 1], v + ref[m - k - 1]).astype(f32)
    return s, v


def _soft_v(v):
    with np.errstate(invalid="ignore"):
        v = np.where(np.isnan(v) | (v < 0), f32(0), v)
        return np.where(v > 255, f32(255), v).astype(f32).astype(np.int64).astype(np.uint8)


def block_demod(D, cmap, nbr, x, phi0=f32(0), soft=False, fixed=False, theta=None):
    """-> (sym u8[n], xhat c64[n], soft u8[n, bps] or None, phi after the block).  theta: the phases to use (PSK, DPSK)
    in place of np.arctan2 in f32."""
    cmap = np.asarray(cmap, np.complex64)
    nbr = np.asarray(nbr, np.uint8).reshape(D.M, -1)
    x = np.asarray(x, np.complex64)
    re, im = x.real.astype(f32), x.imag.astype(f32)
    n, bps = x.size, D.bps
    sb = None
    phi = f32(phi0)
    with np.errstate(over="ignore", invalid="ignore"):
        if D.kind in (PSK, DPSK):
            theta = np.arctan2(im, re).astype(f32) if theta is None else np.asarray(theta, f32)
        if D.kind == ASK:
            s, _ = _linear_v(D.ref, re, bps)
            s = gray_encode(s)
            xh = cmap[s]
        elif D.kind == QAM:
            mi, mq = (bps + 1) >> 1, bps >> 1
            si, ri = _linear_v(D.ref, re, mi)
            sq, rq = _linear_v(D.ref, im, mq)
            s = (gray_encode(si) << mq) + gray_encode(sq)
            xh = ((re - ri).astype(f32) + 1j * (im - rq).astype(f32)).astype(np.complex64)
        elif D.kind == PSK:
            t = (theta - D.d_phi).astype(f32)
            t = np.where(t < -PI, t + TWO_PI, t).astype(f32)
            s, _ = _linear_v(D.ref, t, bps)
            s = gray_encode(s)
            xh = cmap[s]
        elif D.kind == DPSK:
            prev = np.concatenate([[phi], theta[:-1]]).astype(f32)
            d = ((theta - prev).astype(f32) - D.d_phi).astype(f32)
            d = np.where(d > PI, d - TWO_PI, np.where(d < -PI, d + TWO_PI, d)).astype(f32)
            s, res = _linear_v(D.ref, d, bps)
            s = gray_encode(s)
            a = (theta - res).astype(f32)
            xh = (np.cos(a).astype(f32) + 1j * np.sin(a).astype(f32)).astype(np.complex64)
            if n:
                phi = theta[-1]
        elif D.kind == BPSK:
            s = np.where(re > 0, 0, 1)
            xh = np.where(s == 0, f32(1), f32(-1)).astype(np.complex64)
            if soft:
                sb = _soft_v((f32(-2) * re) * f32(4) * f32(16) + f32(127))[:, None]
        elif D.kind == QPSK:
            s = np.where(re > 0, 0, 1) + np.where(im > 0, 0, 2)
            xh = (np.where(s & 1, -FRAC_1_SQRT_2, FRAC_1_SQRT_2) + 1j * np.where(s & 2, -FRAC_1_SQRT_2, FRAC_1_SQRT_2)).astype(np.complex64)
            if soft:
                sb = np.stack([_soft_v((f32(-2) * im) * f32(5.8) * f32(16) + f32(127)),
                               _soft_v((f32(-2) * re) * f32(5.8) * f32(16) + f32(127))], 1)
        elif D.kind == OOK:
            s = np.where(re > FRAC_1_SQRT_2, 0, 1)
            xh = np.where(s == 0, SQRT_2, f32(0)).astype(np.complex64)
        else:                                                 # Arb: squared distances, first minimum, the soft quirk
            dmin = np.full(n, np.inf, f32)
            s = np.zeros(n, np.int64)
            d0 = np.full((bps, n), 4, f32)
            d1 = np.full((bps, n), 4, f32)
            for idx in range(D.M):
                er, ei = re - f32(cmap[idx].real), im - f32(cmap[idx].imag)
                d = (er * er + ei * ei).astype(f32)
                lt = d < dmin
                dmin = np.where(lt, d, dmin)
                s = np.where(lt, idx, s)
                if soft:
                    t = np.full(n, idx) if fixed else s
                    for k in range(bps):
                        one = ((t >> (bps - k - 1)) & 1) != 0
                        d0[k] = np.where(~one & (d < d0[k]), d, d0[k])
                        d1[k] = np.where(one & (d < d1[k]), d, d1[k])
            xh = cmap[s]
            if soft:
                sb = np.stack([_soft_v(((d0[k] - d1[k]) * D.gamma) * f32(16) + f32(127)) for k in range(bps)], 1)
        if soft and sb is None:
            p = nbr.shape[1]
            if p > 0:
                gamma = f32(1.2) * f32(D.M)
                er, ei = re - xh.real.astype(f32), im - xh.imag.astype(f32)
                d = (er * er + ei * ei).astype(f32)
                bits = [((s >> (bps - k - 1)) & 1) != 0 for k in range(bps)]
                d0 = [np.where(b, f32(8), d).astype(f32) for b in bits]
                d1 = [np.where(b, d, f32(8)).astype(f32) for b in bits]
                for i in range(p):
                    nb = nbr[s, i].astype(np.int64)
                    c = cmap[nb]
                    er, ei = re - c.real.astype(f32), im - c.imag.astype(f32)
                    d = (er * er + ei * ei).astype(f32)
                    for k in range(bps):
                        one = ((nb >> (bps - k - 1)) & 1) != 0
                        d0[k] = np.where(~one & (d < d0[k]), d, d0[k])
                        d1[k] = np.where(one & (d < d1[k]), d, d1[k])
                sb = np.stack([_soft_v(((d0[k] - d1[k]) * gamma) * f32(16) + f32(127)) for k in range(bps)], 1)
            else:
                sb = np.stack([np.where((s >> (bps - k - 1)) & 1, 255, 0).astype(np.uint8) for k in range(bps)], 1)
    return np.asarray(s).astype(np.uint8), xh, sb, phi
