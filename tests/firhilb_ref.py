"""Restatement of FirHilbertFilter (src/filter/fir/firhilb.rs) for the tests: test infrastructure only.

FirHilbRef is the reference's per-sample loop: four Window<f32> of 2m samples (push drops the oldest, read() is oldest
first, index(m - 1) the m-th oldest), hq.dotprod(read()) as products and adds in f32, left to right from +0.0, and the
toggle.  block() is a vectorised closed form of the four block modes for long streams: each window is the virtual
stream window ++ the values pushed into it, every output is one delayed sample of one stream and a 2m-tap sum over
another, and the sums run tap by tap over whole arrays (one f32 rounding per product and per add, as in the loop)."""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.sinf.restype, _libm.sinf.argtypes = ctypes.c_float, [ctypes.c_float]
PI = f32(np.pi)                                        # std::f32::consts::PI

R2C, C2R, DECIM, INTERP = "r2c", "c2r", "decim", "interp"
MODES = (R2C, C2R, DECIM, INTERP)


def sinf(x):
    return f32(_libm.sinf(float(f32(x))))


def design(m, as_, kaiser):
    """new() :38-64 on top of fir_design_kaiser (kaiser: n, fc, as_, mu -> f32 taps)"""
    if m < 2:
        raise ValueError("filter semi-length (m) must be at least 2")
    h_len = 4 * m + 1
    h = np.asarray(kaiser(h_len, 0.25, abs(float(as_)), 0.0), f32).copy()
    for i in range(h_len):
        t = f32(i) - f32(h_len - 1) / f32(2.0)
        h[i] = h[i] * (f32(1.0) * sinf(f32(0.5) * PI * t))
    return np.array([h[h_len - i - 1] for i in range(1, h_len, 2)], f32)


def _neg(v):
    return f32(-v)


class FirHilbRef:
    """the per-sample loop; state = (w[4][2m], toggle)"""

    def __init__(self, hq):
        self.hq = np.asarray(hq, f32)
        self.L = len(self.hq)
        self.m = self.L // 2
        self.reset()

    def reset(self):                                  # :87-93
        self.w = np.zeros((4, self.L), f32)
        self.toggle = False

    def clone(self):
        c = FirHilbRef(self.hq)
        c.w = self.w.copy()
        c.toggle = self.toggle
        return c

    def state(self):
        return self.w.copy(), self.toggle

    def _push(self, i, v):                            # window.rs:77-85
        self.w[i, :-1] = self.w[i, 1:]
        self.w[i, -1] = f32(v)

    def _index(self, i):                              # index(m - 1)
        return self.w[i, self.m - 1]

    def _dot(self, i):                                # hq.dotprod(read())
        s = f32(0.0)
        for a, b in zip(self.hq, self.w[i]):
            s = f32(s + f32(a * b))
        return s

    def r2c_execute(self, x):                         # :104-137
        if not self.toggle:
            self._push(0, x)
            y = (self._index(0), self._dot(1))
        else:
            self._push(1, x)
            y = (self._index(1), self._dot(0))
        self.toggle = not self.toggle
        return y

    def c2r_execute(self, x):                         # :149-180 -> (lsb, usb)
        re, im = f32(np.real(x)), f32(np.imag(x))
        if not self.toggle:
            self._push(0, re)
            self._push(1, im)
            yi, yq = self._index(0), self._dot(3)
        else:
            self._push(2, re)
            self._push(3, im)
            yi, yq = self._index(2), self._dot(1)
        self.toggle = not self.toggle
        return f32(yi + yq), f32(yi - yq)

    def decim_execute(self, x):                       # :191-211
        self._push(1, x[0])
        yq = self._dot(1)
        self._push(0, x[1])
        yi = self._index(0)
        y = (_neg(yi), _neg(yq)) if self.toggle else (yi, yq)
        self.toggle = not self.toggle
        return y

    def interp_execute(self, x):                      # :233-248
        re, im = f32(np.real(x)), f32(np.imag(x))
        vi = _neg(re) if self.toggle else re
        vq = _neg(im) if self.toggle else im
        self._push(0, vq)
        y0 = self._index(0)
        self._push(1, vi)
        y1 = self._dot(1)
        self.toggle = not self.toggle
        return y0, y1

    def run(self, mode, x):
        """n per-sample calls, in the block layout: r2c / decim -> complex64, c2r / interp -> float32 pairs"""
        x = np.asarray(x)
        if mode == R2C:
            return _c64([self.r2c_execute(v) for v in x.astype(f32)])
        if mode == DECIM:
            x = x.astype(f32)
            return _c64([self.decim_execute(x[2 * i: 2 * i + 2]) for i in range(len(x) // 2)])
        fn = self.c2r_execute if mode == C2R else self.interp_execute
        out = [fn(v) for v in x.astype(np.complex64)]
        return np.array(out, f32).reshape(-1)


def _c64(pairs):
    a = np.array(pairs, f32).reshape(-1, 2) if len(pairs) else np.zeros((0, 2), f32)
    return a.view(np.complex64).reshape(-1)


def _sdot(hq, v, start, n):
    """s[i] = sum_k hq[k] v[start + i + k], k ascending, one f32 rounding per product and per add"""
    s = np.zeros(n, f32)
    for k in range(len(hq)):
        s = s + hq[k] * v[start + k: start + k + n]
    return s


def _flip(v, mask):
    v = v.copy()
    v[mask] = -v[mask]
    return v


def block(mode, hq, state, x):
    """closed form of n per-sample calls of one mode from state (w[4][2m], toggle); returns (y, new state)"""
    hq = np.asarray(hq, f32)
    w, t0 = np.array(state[0], f32), bool(state[1])
    L = len(hq)
    m = L // 2
    x = np.asarray(x)
    if mode in (R2C, DECIM):
        x = x.astype(f32)
    else:
        x = x.astype(np.complex64)
    n = len(x) // 2 if mode == DECIM else len(x)
    w1 = w.copy()
    if mode == R2C:
        a, b = (1, 0) if t0 else (0, 1)
        va = np.concatenate([w[a], x[0::2]])
        vb = np.concatenate([w[b], x[1::2]])
        ne, no = (n + 1) // 2, n // 2
        y = np.zeros((n, 2), f32)
        y[0::2, 0] = va[m: m + ne]
        y[0::2, 1] = _sdot(hq, vb, 0, ne)
        y[1::2, 0] = vb[m: m + no]
        y[1::2, 1] = _sdot(hq, va, 1, no)
        w1[a], w1[b] = va[-L:], vb[-L:]
        y = y.view(np.complex64).reshape(-1)
    elif mode == C2R:
        p, q = ((2, 3), (0, 1)) if t0 else ((0, 1), (2, 3))
        xe, xo = x[0::2], x[1::2]
        vpr = np.concatenate([w[p[0]], xe.real.astype(f32)])
        vpi = np.concatenate([w[p[1]], xe.imag.astype(f32)])
        vqr = np.concatenate([w[q[0]], xo.real.astype(f32)])
        vqi = np.concatenate([w[q[1]], xo.imag.astype(f32)])
        ne, no = (n + 1) // 2, n // 2
        yi = np.zeros(n, f32)
        yq = np.zeros(n, f32)
        yi[0::2] = vpr[m: m + ne]
        yq[0::2] = _sdot(hq, vqi, 0, ne)
        yi[1::2] = vqr[m: m + no]
        yq[1::2] = _sdot(hq, vpi, 1, no)
        y = np.stack([yi + yq, yi - yq], axis=1).reshape(-1)
        w1[p[0]], w1[p[1]], w1[q[0]], w1[q[1]] = vpr[-L:], vpi[-L:], vqr[-L:], vqi[-L:]
    elif mode == DECIM:
        v1 = np.concatenate([w[1], x[0: 2 * n: 2]])
        v0 = np.concatenate([w[0], x[1: 2 * n: 2]])
        neg = ((np.arange(n) & 1) == 1) != t0
        y = np.stack([_flip(v0[m: m + n], neg), _flip(_sdot(hq, v1, 1, n), neg)], axis=1)
        y = y.astype(f32).view(np.complex64).reshape(-1)
        w1[1], w1[0] = v1[-L:], v0[-L:]
    else:
        neg = ((np.arange(n) & 1) == 1) != t0
        v0 = np.concatenate([w[0], _flip(x.imag.astype(f32), neg)])
        v1 = np.concatenate([w[1], _flip(x.real.astype(f32), neg)])
        y = np.stack([v0[m: m + n], _sdot(hq, v1, 1, n)], axis=1).reshape(-1)
        w1[0], w1[1] = v0[-L:], v1[-L:]
    return y, (w1, t0 != bool(n & 1))


def same_bits(a, b):
    a = np.ascontiguousarray(a).view(np.uint32)
    b = np.ascontiguousarray(b).view(np.uint32)
    return a.shape == b.shape and np.array_equal(a, b)
