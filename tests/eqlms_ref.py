"""Restatement of equalization::eqlms::Eqlms<Complex32> (src/equalization/eqlms.rs) for a bank of C independent channels
of one design, as yagi_amd.EqLms defines it (include/yagi_hip.h).

Two forms of the same sequential loop:
  EqLmsRef      numpy f32, vectorised ACROSS CHANNELS (and, for the products, across taps) only: every operation is an
                array operation, so each is rounded on its own; time is a Python loop, and the sum over the window is a
                strictly sequential np.add.accumulate from +0.0, oldest first.
  EqLmsScalar   one channel, statement by statement in np.float32 scalars, with the reference's explicit WDelay(h_len)
                for x2: that the library recomputes x2_0 from the sample leaving the window is proven by the two forms
                agreeing bit for bit.
Both carry the two stated deviations of the library: |z| = (float)sqrt((double)re^2 + (double)im^2) in step_blind
(abs_def), and DECISION's rule (decide): the first table entry at the least unfused squared distance, only a strictly
smaller value replacing the best.  decim_block runs decim_execute and THEN one update per symbol, as the reference's
testbench composes them."""
import numpy as np

LEN_MAX = 128            # YAGI_EQLMS_LEN_MAX
CHANNELS_MAX = 1 << 20   # YAGI_EQLMS_CHANNELS_MAX
TABLE_MAX = 256          # YAGI_EQLMS_TABLE_MAX
NONE, TRAIN, BLIND, DECISION = 0, 1, 2, 3

F = np.float32
D = np.float64


class ConfigError(ValueError):
    pass


def abs_def(re, im):
    """the library's |z|: the f64 products are exact, the sum and the root are rounded once each, then once to f32"""
    re, im = np.asarray(re, F).astype(D), np.asarray(im, F).astype(D)
    with np.errstate(all="ignore"):
        return np.sqrt(re * re + im * im).astype(F)


def initial_taps(h_len, h=None):
    """new (:25-49): h0"""
    if h_len == 0 or h_len > LEN_MAX:
        raise ConfigError("h_len")
    h0 = np.zeros(h_len, np.complex64)
    if h is None:
        h0[h_len // 2] = 1
    else:
        h = np.asarray(h, np.complex64)
        if h.shape != (h_len,):
            raise ConfigError("h")
        h0.real, h0.imag = h.real[::-1], -h.imag[::-1]
    return h0


def rnyquist_h(ftype, k, m, beta, dt):
    """new_rnyquist (:51-76); the prototype is the library's host design (no device needed)"""
    import yagi_amd as ya
    if k < 2 or m == 0 or not (0.0 <= beta <= 1.0) or not (-1.0 <= dt <= 1.0):
        raise ConfigError("config")
    h = np.asarray(ya.fir_design_prototype(ftype, k, m, beta, dt), F)
    out = np.zeros(h.size, np.complex64)
    out.real = h / F(k)
    return out


def lowpass_h(h_len, fc):
    """new_lowpass (:78-90): x * Complex(2, 0) * fc"""
    import yagi_amd as ya
    if h_len == 0 or not (0.0 <= fc <= 0.5):
        raise ConfigError("config")
    h = np.asarray(ya.fir_design_kaiser(h_len, fc, 40.0, 0.0), F)
    out = np.zeros(h.size, np.complex64)
    out.real, out.imag = (h * F(2.0)) * F(fc), (h * F(0.0)) * F(fc)
    return out


class EqLmsRef:
    def __init__(self, channels, h_len, h=None):
        if not 1 <= channels <= CHANNELS_MAX:
            raise ConfigError("channels")
        self.h0 = initial_taps(h_len, h)
        self.C, self.h_len, self.mu, self.table = int(channels), int(h_len), F(0.5), None
        self.reset()

    def reset(self):
        C, L = self.C, self.h_len
        self.wr = np.repeat(self.h0.real[:, None], C, axis=1).astype(F)      # w0, [h_len][C]
        self.wi = np.repeat(self.h0.imag[:, None], C, axis=1).astype(F)
        self.rr, self.ri = np.zeros((L, C), F), np.zeros((L, C), F)          # the window, oldest first
        self.x2_sum = np.zeros(C, F)
        self.count = np.zeros(C, np.uint64)

    def reset_channel(self, c):
        if not 0 <= c < self.C:
            raise ConfigError("channel")
        self.wr[:, c], self.wi[:, c] = self.h0.real, self.h0.imag
        self.rr[:, c] = self.ri[:, c] = 0
        self.x2_sum[c] = 0
        self.count[c] = 0

    def clone(self):
        new = EqLmsRef(self.C, self.h_len)
        new.h0, new.mu, new.table = self.h0.copy(), self.mu, None if self.table is None else self.table.copy()
        for name in ("wr", "wi", "rr", "ri", "x2_sum", "count"):
            setattr(new, name, getattr(self, name).copy())
        return new

    def set_bw(self, mu):
        if mu < 0:
            raise ConfigError("learning rate cannot be less than zero")
        self.mu = F(mu)

    def set_constellation(self, table):
        table = np.asarray(table, np.complex64).reshape(-1)
        if not 1 <= table.size <= TABLE_MAX:
            raise ConfigError("table")
        self.table = table.copy()

    def get_coefficients(self):
        """w0[channels][h_len]"""
        return _cplx(self.wr, self.wi).T.copy()

    def get_weights(self):
        return _cplx(self.wr[::-1], -self.wi[::-1]).T.copy()

    # -- the reference's per-sample calls, one array operation per rounding
    def push(self, x):
        xr, xi = np.asarray(x.real, F), np.asarray(x.imag, F)
        with np.errstate(all="ignore"):
            x2_n = xr * xr - xi * (-xi)
            x2_0 = self.rr[0] * self.rr[0] - self.ri[0] * (-self.ri[0])      # the sample that leaves the window
            self.x2_sum = self.x2_sum + (x2_n - x2_0)
        self.rr = np.concatenate([self.rr[1:], xr[None, :]])
        self.ri = np.concatenate([self.ri[1:], xi[None, :]])
        self.count = self.count + np.uint64(1)

    def execute(self):
        with np.errstate(all="ignore"):
            ar, ai = self.wr, -self.wi
            tr = ar * self.rr - ai * self.ri
            ti = ar * self.ri + ai * self.rr
            z = np.zeros((1, self.C), F)
            yr = np.add.accumulate(np.concatenate([z, tr]), axis=0)[-1]
            yi = np.add.accumulate(np.concatenate([z, ti]), axis=0)[-1]
        return _cplx(yr, yi)

    def step(self, d, y, only=None):
        """step(d, d_hat) on the channels of `only` (all by default) that have count >= h_len"""
        go = self.count >= np.uint64(self.h_len)
        if only is not None:
            go = go & only
        with np.errstate(all="ignore"):
            d, y = np.asarray(d, np.complex64), np.asarray(y, np.complex64)
            ar, ai = d.real - y.real, d.imag - y.imag
            sr, si = self.mu * ar, self.mu * (-ai)
            pr = sr * self.rr - si * self.ri
            pi = sr * self.ri + si * self.rr
            nr, ni = self.wr + pr / self.x2_sum, self.wi + pi / self.x2_sum
        self.wr, self.wi = np.where(go, nr, self.wr), np.where(go, ni, self.wi)

    def unit(self, y):
        a = abs_def(y.real, y.imag)
        with np.errstate(all="ignore"):
            return _cplx(y.real / a, y.imag / a)

    def decide(self, y):
        dmin, best = np.full(self.C, np.inf, F), np.zeros(self.C, np.int64)
        with np.errstate(all="ignore"):
            for j, t in enumerate(self.table):
                er, ei = y.real - t.real, y.imag - t.imag
                dd = er * er + ei * ei
                lt = dd < dmin
                dmin, best = np.where(lt, dd, dmin), np.where(lt, j, best)
        return self.table[best]

    # -- the block calls
    def execute_block(self, k, x):
        if k == 0:
            raise ConfigError("k")
        x = np.asarray(x, np.complex64)
        y = np.zeros_like(x)
        for i in range(x.shape[0]):
            self.push(x[i])
            y[i] = self.execute()
            due = (self.count + np.uint64(k - 1)) % np.uint64(k) == 0
            if due.any():
                self.step(self.unit(y[i]), y[i], due)
        return y

    def decim_block(self, k, mode, x, d=None):
        x = np.asarray(x, np.complex64)
        if k == 0 or x.shape[0] % k != 0 or mode not in (NONE, TRAIN, BLIND, DECISION):
            raise ConfigError("k, n or mode")
        n = x.shape[0] // k
        if mode == TRAIN and n and d is None:
            raise ConfigError("TRAIN needs d")
        if mode == DECISION and self.table is None:
            raise ConfigError("DECISION needs a table")
        y = np.zeros((n, self.C), np.complex64)
        for i in range(n):
            self.push(x[i * k])
            y[i] = self.execute()
            for j in range(1, k):
                self.push(x[i * k + j])
            if mode == TRAIN:
                self.step(np.asarray(d[i], np.complex64), y[i])
            elif mode == BLIND:
                self.step(self.unit(y[i]), y[i])
            elif mode == DECISION:
                self.step(self.decide(y[i]), y[i])
        return y


def _cplx(re, im):
    out = np.zeros(np.shape(re), np.complex64)
    out.real, out.imag = re, im
    return out


# ---- one channel, statement by statement ------------------------------------------------------------------------------
class WDelay:
    """buffer/wdelay.rs: read() after push() is the value pushed `delay` pushes earlier"""

    def __init__(self, delay):
        self.v, self.delay, self.read_index = [F(0)] * (delay + 1), delay, 0

    def push(self, value):
        self.v[self.read_index] = value
        self.read_index = (self.read_index + 1) % (self.delay + 1)

    def read(self):
        return self.v[self.read_index]


def _cmul(a, b):
    """num-complex's product of (re, im) pairs"""
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


class EqLmsScalar:
    def __init__(self, h_len, h=None):
        self.h0 = initial_taps(h_len, h)
        self.h_len, self.mu, self.table = int(h_len), F(0.5), None
        self.reset()

    def reset(self):
        self.w0 = [(F(v.real), F(v.imag)) for v in self.h0]
        self.buffer = [(F(0), F(0))] * self.h_len
        self.x2 = WDelay(self.h_len)
        self.count, self.buf_full, self.x2_sum = 0, False, F(0)

    def push(self, x):
        x = (F(x.real), F(x.imag))
        self.buffer = self.buffer[1:] + [x]
        x2_n = _cmul(x, (x[0], -x[1]))[0]
        self.x2.push(x2_n)
        x2_0 = self.x2.read()
        self.x2_sum = self.x2_sum + (x2_n - x2_0)
        self.count += 1

    def execute(self):
        acc = (F(0), F(0))
        for w, r in zip(self.w0, self.buffer):
            t = _cmul((w[0], -w[1]), r)
            acc = (acc[0] + t[0], acc[1] + t[1])
        return acc

    def step(self, d, d_hat):
        if not self.buf_full:
            if self.count < self.h_len:
                return
            self.buf_full = True
        alpha = (d[0] - d_hat[0], d[1] - d_hat[1])
        s = (self.mu * alpha[0], self.mu * (-alpha[1]))
        w1 = []
        for w, r in zip(self.w0, self.buffer):
            p = _cmul(s, r)
            w1.append((w[0] + p[0] / self.x2_sum, w[1] + p[1] / self.x2_sum))
        self.w0 = w1

    def step_blind(self, d_hat):
        a = abs_def(d_hat[0], d_hat[1])[()]
        self.step((d_hat[0] / a, d_hat[1] / a), d_hat)

    def decide(self, y):
        dmin, best = F(np.inf), 0
        for j, t in enumerate(self.table):
            er, ei = y[0] - F(t.real), y[1] - F(t.imag)
            dd = er * er + ei * ei
            if dd < dmin:
                dmin, best = dd, j
        t = self.table[best]
        return F(t.real), F(t.imag)

    def execute_block(self, k, x):
        y = np.zeros(len(x), np.complex64)
        with np.errstate(all="ignore"):
            for i, xi in enumerate(x):
                self.push(xi)
                d_hat = self.execute()
                y[i] = complex(*d_hat)
                if (self.count + k - 1) % k == 0:
                    self.step_blind(d_hat)
        return y

    def decim_block(self, k, mode, x, d=None):
        n = len(x) // k
        y = np.zeros(n, np.complex64)
        with np.errstate(all="ignore"):
            for i in range(n):
                self.push(x[i * k])                          # decim_execute
                sym = self.execute()
                for j in range(1, k):
                    self.push(x[i * k + j])
                y[i] = complex(*sym)
                if mode == TRAIN:
                    self.step((F(d[i].real), F(d[i].imag)), sym)
                elif mode == BLIND:
                    self.step_blind(sym)
                elif mode == DECISION:
                    self.step(self.decide(sym), sym)
        return y

    def get_coefficients(self):
        return np.array([complex(*w) for w in self.w0], np.complex64)


# ---- streams and comparisons the tests share ---------------------------------------------------------------------------
def same_words(a, b):
    """bit for bit, a NaN matching any NaN (sign and payload of a NaN differ between instruction sets)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "c":
        a, b = np.ascontiguousarray(a).view(np.float32), np.ascontiguousarray(b).view(np.float32)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


def noise(seed, n, channels, amp=0.5):
    """N(0, amp^2 / 2) per component; amp may be one value or one per channel"""
    r = np.random.default_rng(seed)
    x = (r.standard_normal((n, channels)) + 1j * r.standard_normal((n, channels))) * np.sqrt(0.5)
    return (x * np.asarray(amp)).astype(np.complex64)


CHANNEL = np.array([1.00, -0.01j, -0.11 + 0.02j, 0.02 + 0.01j, -0.09 - 0.04j])     # the testbench's fixed channel (:229-235)
QPSK_MAP = (np.array([1 + 1j, -1 + 1j, 1 - 1j, -1 - 1j]) * np.sqrt(0.5)).astype(np.complex64)
_Q = np.array([-3, -1, 1, 3]) / np.sqrt(10.0)
QAM16_MAP = (_Q[:, None] + 1j * _Q[None, :]).reshape(-1).astype(np.complex64)


def modulated(seed, cmap, nsym, k=2, m=7, beta=0.3):
    """(symbols[nsym], samples[nsym k]): seeded symbols of `cmap` through the Arkaiser interpolator
    FirInterpolationFilter::new_prototype designs and the testbench's channel"""
    import yagi_amd as ya
    r = np.random.default_rng(seed)
    s = np.asarray(cmap, np.complex64)[r.integers(0, len(cmap), nsym)]
    h = np.asarray(ya.fir_design_prototype(ya.FirFilterShape.Arkaiser, k, m, beta, 0.0), np.float64)
    up = np.zeros(nsym * k, np.complex128)
    up[::k] = s
    tx = np.convolve(up, h)[:nsym * k]
    return s, np.convolve(tx, CHANNEL)[:nsym * k].astype(np.complex64)


def streams(n, channels, seed, k=2):
    """n rows for `channels` channels: noise of amplitudes 0.5, 4, 0.02, 1 and 2 in turn, QPSK and QAM16 through the
    interpolator and the channel on every fifth channel, channel 1 (where there is one) all zero, and channel 3 with
    one NaN and, later, one Inf sample"""
    amps = np.array([0.5, 4.0, 0.02, 1.0, 2.0])[np.arange(channels) % 5]
    x = noise(seed, n, channels, amps)
    ks = max(k, 2)                                             # the interpolator needs two samples per symbol
    nsym = -(-n // ks)
    for c in range(0, channels, 5):
        cmap = QPSK_MAP if (c // 5) % 2 == 0 else QAM16_MAP
        x[:, c] = modulated(seed + c, cmap, nsym, k=ks, m=3)[1][:n]
    if channels > 1:
        x[:, 1] = 0
    if channels > 3 and n > 8:
        x[n // 3, 3] = np.nan
        x[(2 * n) // 3, 3] = np.inf
    return x


def symbols(n, channels, seed):
    """rows of known symbols for TRAIN: QPSK points, another draw per channel"""
    r = np.random.default_rng(seed)
    return QPSK_MAP[r.integers(0, 4, (n, channels))]


# ---- the GPU tests' shared plumbing --------------------------------------------------------------------------------------
def run_dev(ya, q, k, x, mode=None, d=None, pad=0):
    """EqLms.execute_block_devptr (mode None) or decim_block_devptr on plain device buffers whose pitches are C + pad;
    y starts as zeros and is returned whole, [rows][C + pad]"""
    x = np.asarray(x, np.complex64)
    n, C = x.shape
    pitch = C + pad
    rows = n if mode is None else n // k

    def up(a, r):
        wide = np.full((max(r, 1), pitch), 5 - 3j, np.complex64)
        wide[:r, :C] = a
        return ya.DeviceArray.from_numpy(wide)
    xd = up(x, n)
    dd = up(d, rows) if d is not None else None
    yd = ya.DeviceArray(max(rows, 1) * pitch, np.complex64)
    yd.zero()
    if mode is None:
        q.execute_block_devptr(k, xd.ptr, pitch, n, yd.ptr, pitch)
    else:
        q.decim_block_devptr(k, int(mode), xd.ptr, pitch, n, None if dd is None else dd.ptr, pitch, yd.ptr, pitch)
    ya.synchronize()
    y = yd.to_numpy()[:rows * pitch].reshape(rows, pitch).copy()
    for b in (xd, dd, yd):
        if b is not None:
            b.free()
    return y
