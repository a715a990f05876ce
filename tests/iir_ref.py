"""References for IirFilter (src/filter/iir/iirfilt.rs, iirfiltsos.rs).

(a) ``Seq32``: the reference's f32 recurrence in its exact operation order, one numpy float32 scalar operation at a
    time (products unfused, every sum left to right from zero).  The transfer-function form keeps the VecDeque's
    physical head: rotate_right(1) moves it back one slot and the dot products split into the two slices
    (dotprod/mod.rs:75-121) at n - head.  ``clone()`` restates derive(Clone): VecDeque::clone is contiguous (head 0).
(b) ``iir64``: an f64 reference vectorised over chunks (zero-start pass, sequential chunk scan with A^T, rerun).
(c) ``iir64_loop``: a plain f64 per-sample loop, which pins (b).
Coefficients are normalised like the reference (f32 division by a0, num-complex division for cccf) before (b), (c).
"""
import numpy as np

f32 = np.float32


def _cdiv32(a, b):
    a, b = complex(a), complex(b)
    ar, ai, br, bi = f32(a.real), f32(a.imag), f32(b.real), f32(b.imag)
    d = f32(f32(br * br) + f32(bi * bi))
    return complex(f32(f32(f32(ar * br) + f32(ai * bi)) / d), f32(f32(f32(ai * br) - f32(ar * bi)) / d))


def normalise(kind, b, a):
    """new(): b / a0 and a / a0 in f32 (as python floats / complexes holding f32 values)"""
    if kind == "cccf":
        a0 = a[0]
        return [_cdiv32(v, a0) for v in b], [_cdiv32(v, a0) for v in a]
    a0 = f32(np.real(a[0]))
    return [float(f32(f32(np.real(v)) / a0)) for v in b], [float(f32(f32(np.real(v)) / a0)) for v in a]


def normalise_sos(kind, b, a, nsos):
    nb, na = [], []
    for k in range(nsos):
        bk, ak = normalise(kind, list(b[3 * k:3 * k + 3]), list(a[3 * k:3 * k + 3]))
        nb += bk
        na += ak
    return nb, na


class _Ops:
    """f32 scalar arithmetic: real values as float32, complex values as (re, im) float32 pairs"""

    def __init__(self, complex_samples, complex_coeffs):
        self.cs, self.cc = complex_samples, complex_coeffs

    def zero(self):
        return (f32(0), f32(0)) if self.cs else f32(0)

    def smp(self, v):
        return (f32(np.real(v)), f32(np.imag(v))) if self.cs else f32(np.real(v))

    def coef(self, v):
        return (f32(np.real(v)), f32(np.imag(v))) if self.cc else f32(np.real(v))

    def add(self, x, y):
        return (f32(x[0] + y[0]), f32(x[1] + y[1])) if self.cs else f32(x + y)

    def sub(self, x, y):
        return (f32(x[0] - y[0]), f32(x[1] - y[1])) if self.cs else f32(x - y)

    def mul(self, x, c):          # sample * coefficient (num-complex Mul)
        if not self.cs:
            return f32(x * c)
        if not self.cc:
            return (f32(x[0] * c), f32(x[1] * c))
        return (f32(f32(x[0] * c[0]) - f32(x[1] * c[1])), f32(f32(x[0] * c[1]) + f32(x[1] * c[0])))

    def out(self, v):
        return complex(v[0], v[1]) if self.cs else float(v)


class Seq32:
    """restatement (a)"""

    def __init__(self, kind, b, a, nsos=None, scale=1.0):
        self.kind = kind
        self.o = _Ops(kind != "rrrf", kind == "cccf")
        self.sos = nsos is not None
        if self.sos:
            nb, na = normalise_sos(kind, list(b), list(a), nsos)
            self.nsos = nsos
            self.S = 2 * nsos
        else:
            nb, na = normalise(kind, list(b), list(a))
            n = max(len(nb), len(na))
            nb = nb + [0.0] * (n - len(nb))
            na = na + [0.0] * (n - len(na))
            self.n = n
            self.S = n - 1
            self.head = 0
        self.b = [self.o.coef(v) for v in nb]
        self.a = [self.o.coef(v) for v in na]
        self.s = [self.o.zero() for _ in range(self.S)]
        self.scale = self.o.coef(scale)

    def clone(self):
        c = object.__new__(Seq32)
        c.__dict__.update(self.__dict__)
        c.s = list(self.s)
        if not self.sos:
            c.head = 0
        return c

    def reset(self):
        self.s = [self.o.zero() for _ in range(self.S)]

    def _tf(self, x):
        o, n = self.o, self.n
        self.head = n - 1 if self.head == 0 else self.head - 1
        split = n if self.head == 0 else n - self.head
        l, r = o.add(o.zero(), o.mul(o.zero(), self.a[0])), o.zero()
        for i in range(1, n):
            q = o.mul(self.s[i - 1], self.a[i])
            if i < split:
                l = o.add(l, q)
            else:
                r = o.add(r, q)
        w = o.sub(x, o.add(l, r))
        l, r = o.add(o.zero(), o.mul(w, self.b[0])), o.zero()
        for i in range(1, n):
            q = o.mul(self.s[i - 1], self.b[i])
            if i < split:
                l = o.add(l, q)
            else:
                r = o.add(r, q)
        if self.S:
            self.s = [w] + self.s[:-1]
        return o.add(l, r)

    def _sos(self, x):
        o, u = self.o, x
        for k in range(self.nsos):
            v2, v1 = self.s[2 * k + 1], self.s[2 * k]
            v0 = o.sub(o.sub(u, o.mul(v1, self.a[3 * k + 1])), o.mul(v2, self.a[3 * k + 2]))
            u = o.add(o.add(o.mul(v0, self.b[3 * k]), o.mul(v1, self.b[3 * k + 1])), o.mul(v2, self.b[3 * k + 2]))
            self.s[2 * k], self.s[2 * k + 1] = v0, v1
        return u

    def execute(self, x):
        x = self.o.smp(x)
        y = self._sos(x) if self.sos else self._tf(x)
        return self.o.out(self.o.mul(y, self.scale))

    def execute_block(self, x):
        dt = np.float32 if self.kind == "rrrf" else np.complex64
        return np.array([self.execute(v) for v in x], dt)


# ---- f64 ---------------------------------------------------------------------------------------------------------
def _step64(sos, b, a, s, x):
    """one f64 step on arrays (s: list of S arrays); returns (y, new s)"""
    if not sos:
        n = len(b)
        w = x - sum(a[i] * s[i - 1] for i in range(1, n)) if n > 1 else x + 0.0
        y = b[0] * w + (sum(b[i] * s[i - 1] for i in range(1, n)) if n > 1 else 0.0)
        return y, ([w] + s[:-1] if n > 1 else s)
    u, t = x, list(s)
    for k in range(len(b) // 3):
        v1, v2 = s[2 * k], s[2 * k + 1]
        v0 = u - a[3 * k + 1] * v1 - a[3 * k + 2] * v2
        u = b[3 * k] * v0 + b[3 * k + 1] * v1 + b[3 * k + 2] * v2
        t[2 * k], t[2 * k + 1] = v0, v1
    return u, t


def _prep(kind, b, a, nsos, normalised):
    if normalised:
        b, a = list(b), list(a)
    elif nsos is None:
        b, a = normalise(kind, list(b), list(a))
    else:
        b, a = normalise_sos(kind, list(b), list(a), nsos)
    if nsos is None:
        n = max(len(b), len(a))
        b, a = b + [0.0] * (n - len(b)), a + [0.0] * (n - len(a))
    cd = np.complex128 if kind == "cccf" else np.float64
    return [cd(v) for v in b], [cd(v) for v in a], (nsos is not None), (2 * nsos if nsos is not None else len(b) - 1)


def iir64_loop(kind, b, a, x, nsos=None, scale=1.0, normalised=False):
    """(c): plain per-sample f64 loop"""
    b, a, sos, S = _prep(kind, b, a, nsos, normalised)
    dt = np.float64 if kind == "rrrf" else np.complex128
    s = [dt(0)] * S
    y = np.empty(len(x), dt)
    for t, v in enumerate(np.asarray(x, dt)):
        y[t], s = _step64(sos, b, a, s, v)
    return y * scale


def iir64(kind, b, a, x, nsos=None, scale=1.0, normalised=False, chunk=None):
    """(b): f64, vectorised over chunks of `chunk` samples (ragged tail zero-padded, its outputs dropped)"""
    b, a, sos, S = _prep(kind, b, a, nsos, normalised)
    dt = np.float64 if kind == "rrrf" else np.complex128
    x = np.asarray(x, dt)
    n = x.size
    T = chunk or max(1, int(np.sqrt(n)))
    nc = -(-n // T)
    X = np.zeros(nc * T, dt)
    X[:n] = x
    X = X.reshape(nc, T)
    s = [np.zeros(nc, dt) for _ in range(S)]
    for t in range(T):
        _, s = _step64(sos, b, a, s, X[:, t])
    z = np.array(s, dt).reshape(S, nc)
    # A^T: T zero-input steps from the unit states
    mt = np.complex128 if kind == "cccf" else np.float64
    u = [np.eye(S, dtype=mt)[i] for i in range(S)]
    for t in range(T):
        _, u = _step64(sos, b, a, u, np.zeros(S, mt))
    AT = np.array(u, mt).reshape(S, S)
    init = np.zeros((S, nc), dt)
    for c in range(1, nc):
        init[:, c] = AT @ init[:, c - 1] + z[:, c - 1]
    s = [init[i].copy() for i in range(S)]
    Y = np.empty((nc, T), dt)
    for t in range(T):
        Y[:, t], s = _step64(sos, b, a, s, X[:, t])
    return Y.reshape(-1)[:n] * scale
