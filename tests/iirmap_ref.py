"""Restatements of IirDecimationFilter, IirInterpolationFilter and IirHilbertFilter (src/filter/iir/iirdecim.rs,
iirinterp.rs, iirhilb.rs) line by line over iir_ref.Seq32, the reference's f32 recurrence in its own operation order.
The Hilbert transform holds two real filters, as the reference does: that it equals one complex filter is what the
library claims and the tests check."""
import numpy as np

from iir_ref import Seq32

f32 = np.float32
DT = {"rrrf": np.float32, "crcf": np.complex64, "cccf": np.complex64}


class IirDecimRef:
    def __init__(self, kind, M, b, a, nsos=None, scale=1.0):
        assert M >= 2
        self.kind, self.M = kind, M
        self.f = Seq32(kind, b, a, nsos=nsos, scale=scale)

    def clone(self):
        c = object.__new__(IirDecimRef)
        c.kind, c.M, c.f = self.kind, self.M, self.f.clone()
        return c

    def reset(self):
        self.f.reset()

    def execute(self, x):                                   # iirdecim.rs:128-137
        assert len(x) == self.M
        y = None
        for i, xi in enumerate(x):
            v = self.f.execute(xi)
            if i == 0:
                y = v
        return y

    def execute_block(self, x):                             # :145-149
        x = np.asarray(x)
        n = len(x) // self.M
        return np.array([self.execute(x[i * self.M:(i + 1) * self.M]) for i in range(n)], DT[self.kind])


class IirInterpRef:
    def __init__(self, kind, M, b, a, nsos=None, scale=1.0):
        assert M >= 2
        self.kind, self.M = kind, M
        self.f = Seq32(kind, b, a, nsos=nsos, scale=scale)

    def clone(self):
        c = object.__new__(IirInterpRef)
        c.kind, c.M, c.f = self.kind, self.M, self.f.clone()
        return c

    def reset(self):
        self.f.reset()

    def execute(self, x):                                   # iirinterp.rs:93-103
        return [self.f.execute(x if i == 0 else 0.0) for i in range(self.M)]

    def execute_block(self, x):                             # :106-115
        out = []
        for v in x:
            out += self.execute(v)
        return np.array(out, DT[self.kind])


class IirHilbRef:
    """two real filters with the same sections and the u8 state"""

    def __init__(self, b, a, nsos):
        self.f0 = Seq32("rrrf", b, a, nsos=nsos)
        self.f1 = Seq32("rrrf", b, a, nsos=nsos)
        self.state = 0

    def clone(self):
        c = object.__new__(IirHilbRef)
        c.f0, c.f1, c.state = self.f0.clone(), self.f1.clone(), self.state
        return c

    def reset(self):                                        # iirhilb.rs:49-53
        self.f0.reset()
        self.f1.reset()
        self.state = 0

    def r2c_execute(self, x):                               # :55-82
        x, s, two = f32(x), self.state, f32(2.0)
        if s == 0:
            yi, yq = f32(self.f0.execute(x)), f32(self.f1.execute(0.0))
            y = (two * yi, two * yq)
        elif s == 1:
            yi, yq = f32(self.f0.execute(0.0)), f32(self.f1.execute(-x))
            y = (two * -yq, two * yi)
        elif s == 2:
            yi, yq = f32(self.f0.execute(-x)), f32(self.f1.execute(0.0))
            y = (two * -yi, two * -yq)
        else:
            yi, yq = f32(self.f0.execute(0.0)), f32(self.f1.execute(x))
            y = (two * yq, two * -yi)
        self.state = (s + 1) & 3
        return np.complex64(complex(y[0], y[1]))

    def c2r_execute(self, x):                               # :90-117
        re, im, s = f32(np.real(x)), f32(np.imag(x)), self.state
        if s == 0:
            yi, _ = f32(self.f0.execute(re)), self.f1.execute(im)
            y = yi
        elif s == 1:
            _, yq = self.f0.execute(im), f32(self.f1.execute(-re))
            y = -yq
        elif s == 2:
            yi, _ = f32(self.f0.execute(-re)), self.f1.execute(-im)
            y = -yi
        else:
            _, yq = self.f0.execute(-im), f32(self.f1.execute(re))
            y = yq
        self.state = (s + 1) & 3
        return f32(y)

    def decim_execute(self, x):                             # :125-139
        assert self.state in (0, 1), "1 - state underflows the reference's u8"
        x0, x1 = f32(x[0]), f32(x[1])
        xi = -x0 if self.state else x0
        xq = x1 if self.state else -x1
        yi0 = f32(self.f0.execute(xi))
        self.f0.execute(0.0)
        yq0 = f32(self.f1.execute(0.0))
        self.f1.execute(xq)
        self.state = 1 - self.state
        return np.complex64(complex(f32(2.0) * yi0, f32(2.0) * yq0))

    def interp_execute(self, x):                            # :147-158
        assert self.state in (0, 1), "1 - state underflows the reference's u8"
        yi0 = f32(self.f0.execute(f32(np.real(x))))
        self.f0.execute(0.0)
        self.f1.execute(f32(np.imag(x)))
        yq1 = f32(self.f1.execute(0.0))
        y = (f32(-2.0) * yi0 if self.state else f32(2.0) * yi0, f32(2.0) * yq1 if self.state else f32(-2.0) * yq1)
        self.state = 1 - self.state
        return y

    def r2c_execute_block(self, x):
        return np.array([self.r2c_execute(v) for v in x], np.complex64)

    def c2r_execute_block(self, x):
        return np.array([self.c2r_execute(v) for v in x], np.float32)

    def decim_execute_block(self, x):
        return np.array([self.decim_execute(x[2 * i:2 * i + 2]) for i in range(len(x) // 2)], np.complex64)

    def interp_execute_block(self, x):
        out = []
        for v in x:
            out += list(self.interp_execute(v))
        return np.array(out, np.float32)


# ---- the virtual streams of DESIGN section 4, built explicitly (what a caller composes today) ---------------------
def zero_stuff(x, M):
    u = np.zeros(len(x) * M, x.dtype)
    u[::M] = x
    return u


def hilb_input(mode, x, state):
    """the complex stream u fed to one crcf filter; state = the 2-bit state at the start of the call"""
    if mode in ("r2c", "decim"):
        x = np.asarray(x, np.float32)
        k = ((2 * state if mode == "decim" else state) + np.arange(len(x))) & 3
        u = np.zeros(len(x), np.complex64)
        u.real = np.where(k == 0, x, np.where(k == 2, -x, np.float32(0)))
        u.imag = np.where(k == 1, -x, np.where(k == 3, x, np.float32(0)))
        return u
    x = np.asarray(x, np.complex64)
    if mode == "interp":
        return zero_stuff(x, 2)
    k = (state + np.arange(len(x))) & 3
    u = np.empty(len(x), np.complex64)
    u.real = np.choose(k, [x.real, x.imag, -x.real, -x.imag])
    u.imag = np.choose(k, [x.imag, -x.real, -x.imag, x.real])
    return u


def hilb_output(mode, v, state):
    v = np.asarray(v, np.complex64)
    two = np.float32(2.0)
    if mode == "decim":
        return (two * v[::2]).astype(np.complex64)
    k = ((2 * state if mode == "interp" else state) + np.arange(len(v))) & 3
    if mode == "r2c":
        y = np.empty(len(v), np.complex64)
        y.real = two * np.choose(k, [v.real, -v.imag, -v.real, v.imag])
        y.imag = two * np.choose(k, [v.imag, v.real, -v.imag, -v.real])
        return y
    y = np.choose(k, [v.real, -v.imag, -v.real, v.imag]).astype(np.float32)
    return two * y if mode == "interp" else y
