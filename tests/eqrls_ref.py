"""Restatement of equalization::eqrls::Eqrls<Complex32> (src/equalization/eqrls.rs) for a bank of C independent channels
of one design, as yagi_amd.EqRls defines it (include/yagi_hip.h).

Two forms of the same sequential loop:
  EqRlsRef      numpy f32, vectorised ACROSS CHANNELS and across matrix elements only: every operation is an array
                operation, so each is rounded on its own; time and every summation index are Python loops, and every sum
                starts from +0.0 and takes its terms in the reference's order.
  EqRlsScalar   one channel, statement by statement in np.float32 scalars, following eqrls.rs line for line with the
                explicit gxl, gxlp0, p1 and w1 temporaries.
Products and quotients are num-complex's (cmul, cquot).  DECISION's rule and table limits are EqLms's (eqlms_ref.decide).
step_block runs push, execute, the update and THEN the symbol's other k - 1 pushes."""
import numpy as np

import eqlms_ref as er
from eqlms_ref import ConfigError, same_words  # noqa: F401  (the tests take them from here)

LEN_MAX = 32             # YAGI_EQRLS_LEN_MAX
CHANNELS_MAX = 1 << 20   # YAGI_EQRLS_CHANNELS_MAX
MATRIX_MAX = 1 << 26     # YAGI_EQRLS_MATRIX_MAX
NONE, TRAIN, DECISION = 0, 1, 3

F = np.float32


def cmul(a, b):
    """num-complex's product of (re, im) pairs"""
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def cquot(a, b):
    """num-complex's quotient of (re, im) pairs"""
    n = b[0] * b[0] + b[1] * b[1]
    return (a[0] * b[0] + a[1] * b[1]) / n, (a[1] * b[0] - a[0] * b[1]) / n


def conj(a):
    return a[0], -a[1]


def check_design(channels, p):
    if not 1 <= channels <= CHANNELS_MAX or not 1 <= p <= LEN_MAX or channels * p * p > MATRIX_MAX:
        raise ConfigError("design")


def initial_taps(p, h=None):
    """new (:31-62): h0 = h as given"""
    h0 = np.zeros(p, np.complex64)
    if h is None:
        h0[p - 1] = 1
    else:
        h = np.asarray(h, np.complex64)
        if h.shape != (p,):
            raise ConfigError("h")
        h0[:] = h
    return h0


def check_bw(lam):
    if not (0.0 <= lam <= 1.0):
        raise ConfigError("learning rate must be in (0,1)")
    return F(lam)


class EqRlsRef:
    def __init__(self, channels, p, h=None):
        check_design(channels, p)
        self.C, self.p, self.lam, self.table = int(channels), int(p), F(0.99), None
        self.h0 = initial_taps(p, h)
        self.w1r, self.w1i = np.zeros((p, self.C), F), np.zeros((p, self.C), F)
        self.reset()

    def recreate(self, p, h=None):
        if p == self.p:
            if h is not None:
                self.h0 = initial_taps(p, h)
            return
        table = self.table
        self.__init__(self.C, p, h)
        self.table = table

    def _reset(self, c):
        """reset (:76-88) on the channels c (an index or a slice): w1 stays"""
        p = self.p
        self.Pr[:, :, c], self.Pi[:, :, c] = (np.eye(p, dtype=F) * (F(1.0) / F(0.1)))[:, :, None], 0
        self.w0r[:, c], self.w0i[:, c] = self.h0.real[:, None], self.h0.imag[:, None]
        self.rr[:, c] = self.ri[:, c] = 0

    def reset(self):
        p, C = self.p, self.C
        self.Pr, self.Pi = np.zeros((p, p, C), F), np.zeros((p, p, C), F)         # P0[r][c], [p][p][C]
        self.w0r, self.w0i = np.zeros((p, C), F), np.zeros((p, C), F)
        self.rr, self.ri = np.zeros((p, C), F), np.zeros((p, C), F)               # the window, oldest first
        self._reset(slice(None))

    def reset_channel(self, c):
        if not 0 <= c < self.C:
            raise ConfigError("channel")
        self._reset(slice(c, c + 1))

    def clone(self):
        new = EqRlsRef(self.C, self.p)
        new.h0, new.lam, new.table = self.h0.copy(), self.lam, None if self.table is None else self.table.copy()
        for name in ("Pr", "Pi", "w0r", "w0i", "w1r", "w1i", "rr", "ri"):
            setattr(new, name, getattr(self, name).copy())
        return new

    def set_bw(self, lam):
        self.lam = check_bw(lam)

    def set_constellation(self, table):
        table = np.asarray(table, np.complex64).reshape(-1)
        if not 1 <= table.size <= er.TABLE_MAX:
            raise ConfigError("table")
        self.table = table.copy()

    def get_coefficients(self):
        """w0[channels][p]"""
        return er._cplx(self.w0r, self.w0i).T.copy()

    def get_weights(self):
        """w1 reversed (:148-156)"""
        return er._cplx(self.w1r[::-1], self.w1i[::-1]).T.copy()

    def get_matrix(self):
        """P0[channels][p][p]"""
        return np.ascontiguousarray(er._cplx(self.Pr, self.Pi).transpose(2, 0, 1))

    # -- the reference's per-sample calls, one array operation per rounding
    def push(self, x):
        xr, xi = np.asarray(x.real, F), np.asarray(x.imag, F)
        self.rr = np.concatenate([self.rr[1:], xr[None, :]])
        self.ri = np.concatenate([self.ri[1:], xi[None, :]])

    def execute(self):
        with np.errstate(all="ignore"):
            tr, ti = cmul((self.w0r, self.w0i), (self.rr, self.ri))
            yr, yi = np.zeros(self.C, F), np.zeros(self.C, F)
            for i in range(self.p):
                yr, yi = yr + tr[i], yi + ti[i]
        return er._cplx(yr, yi)

    def step(self, d, y):
        p, C = self.p, self.C
        P, x = (self.Pr, self.Pi), (self.rr, self.ri)
        lam = (self.lam, F(0.0))
        with np.errstate(all="ignore"):
            d, y = np.asarray(d, np.complex64), np.asarray(y, np.complex64)
            alpha = (d.real - y.real, d.imag - y.imag)
            xp0 = (np.zeros((p, C), F), np.zeros((p, C), F))                       # [c]
            for r in range(p):
                t = cmul((x[0][r][None, :], x[1][r][None, :]), (P[0][r], P[1][r]))
                xp0 = (xp0[0] + t[0], xp0[1] + t[1])
            z = (np.zeros(C, F), np.zeros(C, F))
            for c in range(p):
                t = cmul((xp0[0][c], xp0[1][c]), conj((x[0][c], x[1][c])))
                z = (z[0] + t[0], z[1] + t[1])
            zeta = (z[0] + lam[0], z[1] + lam[1])
            g = (np.zeros((p, C), F), np.zeros((p, C), F))                         # [r]
            for c in range(p):
                t = cmul((P[0][:, c], P[1][:, c]), conj((x[0][c][None, :], x[1][c][None, :])))
                g = (g[0] + t[0], g[1] + t[1])
            g = cquot(g, (zeta[0][None, :], zeta[1][None, :]))
            gxl = cquot(cmul((g[0][:, None, :], g[1][:, None, :]), (x[0][None, :, :], x[1][None, :, :])), lam)   # [r][c]
            acc = (np.zeros((p, p, C), F), np.zeros((p, p, C), F))
            for i in range(p):
                t = cmul((gxl[0][:, i, None, :], gxl[1][:, i, None, :]), (P[0][None, i], P[1][None, i]))
                acc = (acc[0] + t[0], acc[1] + t[1])
            q = cquot(P, lam)
            self.Pr, self.Pi = q[0] - acc[0], q[1] - acc[1]
            t = cmul((alpha[0][None, :], alpha[1][None, :]), g)
            self.w1r, self.w1i = self.w0r + t[0], self.w0i + t[1]
            self.w0r, self.w0i = self.w1r.copy(), self.w1i.copy()

    def decide(self, y):
        return er.EqLmsRef.decide(self, y)

    # -- the block calls
    def step_block(self, k, mode, x, d=None):
        x = np.asarray(x, np.complex64)
        if k == 0 or x.shape[0] % k != 0 or mode not in (NONE, TRAIN, DECISION):
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
            if mode == TRAIN:
                self.step(np.asarray(d[i], np.complex64), y[i])
            elif mode == DECISION:
                self.step(self.decide(y[i]), y[i])
            for j in range(1, k):
                self.push(x[i * k + j])
        return y

    def train(self, w, x, d):
        """train (:158-176)"""
        w, x = np.asarray(w, np.complex64), np.asarray(x, np.complex64)
        if x.shape[0] < self.p:
            raise ConfigError("training sequence less than filter order")
        self.reset()
        self.w0r, self.w0i = w.real[:, ::-1].T.astype(F), w.imag[:, ::-1].T.astype(F)
        self.step_block(1, TRAIN, x, d)
        return self.get_weights()


# ---- one channel, statement by statement ------------------------------------------------------------------------------
class EqRlsScalar:
    def __init__(self, p, h=None):
        check_design(1, p)
        self.p, self.lam, self.delta, self.table = int(p), F(0.99), F(0.1), None
        self.h0 = [(F(v.real), F(v.imag)) for v in initial_taps(p, h)]
        self.w1 = [(F(0), F(0))] * p
        self.reset()

    def reset(self):
        p, z = self.p, (F(0), F(0))
        self.p0 = [(F(1.0) / self.delta, F(0)) if i == j else z for i in range(p) for j in range(p)]
        self.w0 = list(self.h0)
        self.buffer = [z] * p

    def set_bw(self, lam):
        self.lam = check_bw(lam)

    def push(self, x):
        self.buffer = self.buffer[1:] + [(F(x.real), F(x.imag))]

    def execute(self):
        acc = (F(0), F(0))
        for w, r in zip(self.w0, self.buffer):
            t = cmul(w, r)
            acc = (acc[0] + t[0], acc[1] + t[1])
        return acc

    def step(self, d, d_hat):
        p, x, p0 = self.p, self.buffer, self.p0
        lam = (self.lam, F(0))                                   # lambda.into()

        def csum(terms):
            acc = (F(0), F(0))
            for t in terms:
                acc = (acc[0] + t[0], acc[1] + t[1])
            return acc
        alpha = (d[0] - d_hat[0], d[1] - d_hat[1])
        xp0 = [csum(cmul(x[r], p0[r * p + c]) for r in range(p)) for c in range(p)]
        s = csum(cmul(xp, conj(xi)) for xp, xi in zip(xp0, x))
        zeta = (s[0] + lam[0], s[1] + lam[1])
        g = [cquot(csum(cmul(p0[r * p + c], conj(x[c])) for c in range(p)), zeta) for r in range(p)]
        gxl = [cquot(cmul(g[r], x[c]), lam) for r in range(p) for c in range(p)]
        gxlp0 = [None] * (p * p)
        for r in range(p):                                        # matrix_mul (matrix/math.rs:95-103)
            for c in range(p):
                acc = (F(0), F(0))
                for i in range(p):
                    t = cmul(gxl[r * p + i], p0[i * p + c])
                    acc = (acc[0] + t[0], acc[1] + t[1])
                gxlp0[r * p + c] = acc
        p1 = []
        for i in range(p * p):
            q = cquot(p0[i], lam)
            p1.append((q[0] - gxlp0[i][0], q[1] - gxlp0[i][1]))
        for i in range(p):
            t = cmul(alpha, g[i])
            self.w1[i] = (self.w0[i][0] + t[0], self.w0[i][1] + t[1])
        self.w0 = list(self.w1)
        self.p0 = p1

    def decide(self, y):
        return er.EqLmsScalar.decide(self, y)

    def step_block(self, k, mode, x, d=None):
        n = len(x) // k
        y = np.zeros(n, np.complex64)
        self.w1 = list(self.w1)
        with np.errstate(all="ignore"):
            for i in range(n):
                self.push(x[i * k])
                d_hat = self.execute()
                y[i] = complex(*d_hat)
                if mode == TRAIN:
                    self.step((F(d[i].real), F(d[i].imag)), d_hat)
                elif mode == DECISION:
                    self.step(self.decide(d_hat), d_hat)
                for j in range(1, k):
                    self.push(x[i * k + j])
        return y

    def get_coefficients(self):
        return np.array([complex(*w) for w in self.w0], np.complex64)

    def get_weights(self):
        return np.array([complex(*w) for w in self.w1[::-1]], np.complex64)

    def get_matrix(self):
        return np.array([complex(*v) for v in self.p0], np.complex64).reshape(self.p, self.p)


# ---- streams the tests share ---------------------------------------------------------------------------------------------
def streams(n, channels, seed, k=1):
    """n rows for `channels` channels: noise of amplitudes 0.5, 2, 0.05 and 1 in turn; channel 1 (where there is one) all
    zero, channel 3 with one NaN sample and channel 4 with one Inf sample, each on the first row of a symbol of k rows
    (at p < k a later row of the symbol leaves the window before any update sees it)"""
    amps = np.array([0.5, 2.0, 0.05, 1.0])[np.arange(channels) % 4]
    x = er.noise(seed, n, channels, amps)
    if channels > 1:
        x[:, 1] = 0
    if channels > 3 and n > 4:
        x[n // 3 // k * k, 3] = np.nan
    if channels > 4 and n > 4:
        x[n // 2 // k * k, 4] = np.inf
    return x


def lanes_around(L):
    """channel counts at the seams of a wave of 64 // L channels"""
    G = 64 // L
    return sorted({c for c in (G - 1, G, G + 1) if c >= 1})


def state_same(q, r):
    """get_coefficients, get_weights and get_matrix of the two agree bit for bit"""
    return (same_words(q.get_coefficients(), r.get_coefficients()) and same_words(q.get_weights(), r.get_weights())
            and same_words(q.get_matrix(), r.get_matrix()))
