"""Restatement of Fdelay (src/filter/fdelay.rs) for the tests: test infrastructure only.

FdelayRef is the reference's per-sample loop: a Window of nmax + 1 samples (push drops the oldest, index(w) counts from
the oldest) in front of the oracle's FirPfbFilter built as FirPfbFilter::default(npfb, m), with set_delay's arithmetic
in f32.  block() is a vectorised closed form for long inputs: with X the input stream and D[n], f[n] the lag and branch
in force at step n, the bank's input is V[n] = X[n - D[n]] and y[n] = (sum_k H[f[n]][k] V[n - (Ls - 1) + k]) * 1, summed
tap by tap over whole arrays, real and imaginary parts as separate f32 arrays (one rounding per product and per add, as
in the loop)."""
import numpy as np

f32 = np.float32
KINDS = {"rrrf": np.float32, "crcf": np.complex64, "cccf": np.complex64}


def lag(d, nmax, npfb):
    """set_delay :72-89 -> (w_index, f_index); ValueError where the reference returns Err"""
    d = f32(d)
    if d < 0 or not (d <= f32(nmax)):
        raise ValueError("delay out of range")
    offset = f32(f32(nmax) - d)
    ip = np.floor(offset)
    frac = f32(offset - ip)
    v = f32(f32(npfb) * frac)
    r = np.floor(v)                                   # f32::round: half away from zero, v >= 0
    if f32(v - r) >= f32(0.5):
        r = r + 1
    w, f = int(ip), int(r)
    while f >= npfb:
        w += 1
        f -= npfb
    assert w <= nmax
    return w, f


def lags(d, nmax, npfb):
    """lag() over an array -> (D = nmax - w, f) as int64 arrays"""
    d = np.asarray(d, f32)
    if d.size and (np.any(d < 0) or not np.all(d <= f32(nmax))):
        raise ValueError("delay out of range")
    offset = (f32(nmax) - d).astype(f32)
    ip = np.floor(offset)
    frac = (offset - ip).astype(f32)
    v = (f32(npfb) * frac).astype(f32)
    r = np.floor(v)
    r = r + ((v - r).astype(f32) >= f32(0.5))
    w, f = ip.astype(np.int64), r.astype(np.int64)
    wrap = f >= npfb                                  # frac < 1, so once at the most
    w, f = w + wrap, f - wrap * npfb
    return nmax - w, f


class Design:
    """FirPfbFilter::default(npfb, m) (firpfb.rs:79-114): the taps, the branch length and the rows against the window"""

    def __init__(self, oracle, kind, nmax, m, npfb):
        if nmax == 0 or m == 0 or npfb == 0:
            raise ValueError("config")
        self.kind, self.nmax, self.m, self.npfb = kind, nmax, m, npfb
        self.tdt = KINDS[kind]
        self.h_len = 2 * npfb * m + 1
        self.h = np.asarray(oracle.fir_design_kaiser(self.h_len, f32(0.5) / f32(npfb), 60.0), f32)
        self.Ls = self.h_len // npfb
        k = np.arange(self.Ls)
        self.H = np.stack([self.h[i + (self.Ls - 1 - k) * npfb] for i in range(npfb)]).astype(f32)   # oldest first


class FdelayRef:
    """the per-sample loop; state() = (last nmax inputs, last Ls bank inputs, delay, w_index, f_index)"""

    def __init__(self, oracle, design):
        self.d, self.oracle = design, oracle
        self.pfb = oracle.FirPfbFilter(design.kind, design.npfb, design.h, design.h_len)
        self.reset()

    def reset(self):                                  # :59-65
        d = self.d
        self.delay, self.w_index, self.f_index = f32(0.0), d.nmax - 1, 0
        self.win = np.zeros(d.nmax + 1, d.tdt)
        self.vh = np.zeros(d.Ls, d.tdt)
        self.pfb = self.oracle.FirPfbFilter(d.kind, d.npfb, d.h, d.h_len)

    def get_delay(self):
        return self.delay

    def set_delay(self, delay):                       # :71-97
        self.w_index, self.f_index = lag(delay, self.d.nmax, self.d.npfb)
        self.delay = f32(delay)

    def adjust_delay(self, delta):                    # :99-101
        self.set_delay(f32(self.delay + f32(delta)))

    def push(self, x):                                # :115-118
        self.win[:-1] = self.win[1:]
        self.win[-1] = x
        v = self.win[self.w_index]
        self.vh[:-1] = self.vh[1:]
        self.vh[-1] = v
        self.pfb.push(v)

    def write(self, xs):
        for v in xs:
            self.push(v)

    def execute(self):                                # :126-128
        return self.pfb.execute(self.f_index)

    def execute_block(self, x):                       # :130-136
        out = np.zeros(len(x), self.d.tdt)
        for i, v in enumerate(np.asarray(x, self.d.tdt)):
            self.push(v)
            out[i] = self.execute()
        return out

    def execute_track(self, delays, x):
        out = np.zeros(len(x), self.d.tdt)
        for i, v in enumerate(np.asarray(x, self.d.tdt)):
            self.set_delay(delays[i])
            self.push(v)
            out[i] = self.execute()
        return out

    def state(self):
        return self.win[1:].copy(), self.vh.copy(), self.delay, self.w_index, self.f_index


def reset_state(design):
    return (np.zeros(design.nmax, design.tdt), np.zeros(design.Ls, design.tdt), f32(0.0), design.nmax - 1, 0)


def _parts(a):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return a.real.astype(f32), a.imag.astype(f32)
    return a.astype(f32), None


def block(design, state, x, delays=None):
    """closed form of len(x) per-sample steps from `state`, at the state's fixed delay or with one delay per sample;
    returns (y, new state)"""
    d = design
    xh, vh, delay, w, f = state
    x = np.asarray(x, d.tdt)
    n = len(x)
    if n == 0:
        return np.zeros(0, d.tdt), state
    if delays is None:
        D = np.full(n, d.nmax - w, np.int64)
        fi = np.full(n, f, np.int64)
    else:
        D, fi = lags(delays, d.nmax, d.npfb)
        delay = f32(delays[-1])
        w, f = int(d.nmax - D[-1]), int(fi[-1])
    X = np.concatenate([np.asarray(xh, d.tdt), x])
    V = np.concatenate([np.asarray(vh, d.tdt), X[d.nmax + np.arange(n) - D]])
    vr, vi = _parts(V)
    zero = np.zeros(n, f32)
    sr, si = zero.copy(), zero.copy()
    for k in range(d.Ls):
        hk = d.H[fi, k]
        a = vr[1 + k: 1 + k + n]
        if d.kind == "rrrf":
            sr = sr + a * hk
        elif d.kind == "crcf":                        # Complex * f32, component-wise
            b = vi[1 + k: 1 + k + n]
            sr, si = sr + a * hk, si + b * hk
        else:                                         # Complex * Complex, the tap's imaginary part +0.0
            b = vi[1 + k: 1 + k + n]
            sr, si = sr + (a * hk - b * zero), si + (a * zero + b * hk)
    one = f32(1.0)                                    # the bank's unit scale, applied as the reference applies it
    if d.kind == "rrrf":
        y = sr * one
    else:
        y = np.empty(n, np.complex64)
        if d.kind == "crcf":
            y.real, y.imag = sr * one, si * one
        else:
            y.real, y.imag = sr * one - si * zero, sr * zero + si * one
    return y.astype(d.tdt), (X[-d.nmax:].copy(), V[-d.Ls:].copy(), delay, w, f)


def same_bits(a, b):
    a = np.ascontiguousarray(a).view(np.uint32)
    b = np.ascontiguousarray(b).view(np.uint32)
    return a.shape == b.shape and np.array_equal(a, b)


def delay_estimate(y, m):
    """the reference's estimator (fdelay.rs:170-177) for an impulse input, in f32 like the test"""
    n = len(y)
    fc = f32(0.1) / f32(n)
    i = np.arange(n, dtype=f32)
    ph = (f32(2.0) * f32(np.pi) * fc * i).astype(f32)
    v = np.sum(np.asarray(y).real.astype(f32) * (np.cos(ph) + 1j * np.sin(ph)).astype(np.complex64))
    return f32(np.angle(v) / (2.0 * np.pi * float(fc)) - m)
