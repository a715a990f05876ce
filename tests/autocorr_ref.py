"""Autocorr (include/yagi_hip.h) restated twice (a helper, not a test module).

The definition: X = the stream since reset(), X[k] = 0 for k < 0.  After sample n, with w[i] = X[n-W+1+i] and
v[i] = conj(X[n-W+1+i-d]) for i = 0 .. W-1,

    rxx[n]    = dotprod(w, v)      the sequential sum from +0.0; every product and add rounded on its own; the complex
                                   product is num-complex's (a.re b.re - a.im b.im, a.re b.im + a.im b.re)
    energy[n] = sum_i fl(fl(w[i].re^2) + fl(w[i].im^2))      in the same order from +0.0 (rrrf: fl(w[i]^2))

Autocorr is the fast form: numpy float32, vectorised over n, a Python loop over i, real and imaginary parts as separate
float32 arrays so that numpy's complex multiply never decides a rounding.  SlowAutocorr is the same object made only of
oracle.Window and oracle.dotprod (the reference's buffer::Window and dotprod); tests/test_autocorr_ref_cpu.py pins the
fast form against it, and the GPU tests compare with the fast form."""
import numpy as np

WMAX = 1024          # YAGI_AUTOCORR_WMAX
DMAX = 65536         # YAGI_AUTOCORR_DMAX
TILE = 2048          # YAGI_AUTOCORR_TILE
DTYPES = {"cccf": np.complex64, "rrrf": np.float32}


def _parts(a):
    a = np.asarray(a)
    if a.dtype.kind == "c":
        return np.ascontiguousarray(a.real, np.float32), np.ascontiguousarray(a.imag, np.float32)
    return np.ascontiguousarray(a, np.float32), None


class Autocorr:
    def __init__(self, kind, window_size, delay):
        if not 1 <= window_size <= WMAX or not 0 <= delay <= DMAX:
            raise ValueError("window size or delay out of range")
        self.kind, self.T = kind, np.dtype(DTYPES[kind])
        self.W, self.d = int(window_size), int(delay)
        self.reset()

    window_size = property(lambda self: self.W)
    delay = property(lambda self: self.d)

    def reset(self):
        self.hist = np.zeros(self.W + self.d, self.T)            # the last W + d samples, oldest first

    def clone(self):
        new = Autocorr(self.kind, self.W, self.d)
        new.hist = self.hist.copy()
        return new

    def push(self, x):
        self.hist = np.concatenate([self.hist[1:], np.array([x], self.T)])

    def write(self, x):
        x = np.asarray(x, self.T)
        self.hist = np.concatenate([self.hist, x])[-(self.W + self.d):]

    def _sums(self, stream, n):
        """(rxx, energy) after each of the last n samples of stream, which holds W + d samples in front of them"""
        W, d = self.W, self.d
        first = stream.size - n - W + 1                            # w[0] of the first output
        assert first - d >= 0
        sr, si = _parts(stream)
        re, en = np.zeros(n, np.float32), np.zeros(n, np.float32)
        im = np.zeros(n, np.float32) if si is not None else None
        with np.errstate(all="ignore"):
            for i in range(W):
                a, b = slice(first + i, first + i + n), slice(first + i - d, first + i - d + n)
                if si is None:
                    re = re + sr[a] * sr[b]
                    en = en + sr[a] * sr[a]
                else:
                    ar, ai, vr, vi = sr[a], si[a], sr[b], -si[b]   # v = conj(X[.. - d])
                    re = re + (ar * vr - ai * vi)
                    im = im + (ar * vi + ai * vr)
                    en = en + (ar * ar + ai * ai)
        for v in (re, im, en):
            assert v is None or v.dtype == np.float32
        if si is None:
            return re, en
        out = np.empty(n, np.complex64)
        out.real, out.imag = re, im
        return out, en

    def execute(self):
        return self._sums(self.hist, 1)[0][0]

    def get_energy(self):
        return self._sums(self.hist, 1)[1][0]

    def execute_block(self, x, energy=False):
        x = np.asarray(x, self.T)
        stream = np.concatenate([self.hist, x])
        rxx, en = self._sums(stream, x.size)
        self.hist = stream[-(self.W + self.d):].copy()
        return (rxx, en) if energy else rxx


class SlowAutocorr:
    """the definition word for word: w = Window(W), wd = Window(W + d) fed conj(x); rxx = dotprod(w, wd[:W]); the
    energy is the real part of dotprod(w, conj(w)), whose terms are fl(re^2) - fl(im (-im)) = fl(fl(re^2) + fl(im^2))
    summed in the same order (rrrf: dotprod(w, w))"""

    def __init__(self, oracle, kind, window_size, delay):
        self.o, self.kind, self.T = oracle, kind, np.dtype(DTYPES[kind])
        self.W, self.d = int(window_size), int(delay)
        self.w = oracle.Window(self.W, self.T)
        self.wd = oracle.Window(self.W + self.d, self.T)
        self.dot = "ccc" if kind == "cccf" else "rrrf"

    def push(self, x):
        x = self.T.type(x)
        self.w.push(x)
        self.wd.push(np.conj(x))

    def execute(self):
        return self.T.type(self.o.dotprod(self.dot, self.w.read(), self.wd.read()[:self.W]))

    def get_energy(self):
        w = self.w.read()
        return np.float32(np.real(self.o.dotprod(self.dot, w, np.conj(w))))

    def execute_block(self, x):
        rxx, en = np.empty(len(x), self.T), np.empty(len(x), np.float32)
        for i, v in enumerate(np.asarray(x, self.T)):
            self.push(v)
            rxx[i], en[i] = self.execute(), self.get_energy()
        return rxx, en


def stream(rng, kind, n):
    """N(0, 1) samples, every 7th exactly 0 and some of those -0.0 (in either part of a complex sample)"""
    if kind == "cccf":
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        x[::7] = 0
        x[7::21] = np.complex64(complex(-0.0, 0.0))
        x[14::21] = np.complex64(complex(0.0, -0.0))
        x[3::35] = np.complex64(complex(-0.0, -0.0))
        return x
    x = rng.standard_normal(n).astype(np.float32)
    x[::7] = 0
    x[7::14] = np.float32(-0.0)
    return x
