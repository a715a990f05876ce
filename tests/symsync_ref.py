"""Restatement of filter::symsync::Symsync<Complex32> (src/filter/symsync.rs) for a bank of C independent channels of one
design, as yagi_amd.SymSync defines it (include/yagi_hip.h).

Two forms of the same sequential loop:
  SymSyncRef      numpy f32, vectorised ACROSS CHANNELS only: every operation is an array operation over [C], so each is
                  rounded on its own; time is a Python loop, one step after the other.
  SymSyncScalar   one channel, statement by statement: the matched sum through the oracle's FirPfbFilter.push / execute(i)
                  (the sum FirPfbFilter::execute pins), the derivative sum through oracle.dotprod("rcc") of the bank's row
                  against a window that reset() never clears.
Both carry the capacity rule of the library (absent from the reference, which panics instead): a channel may write at
most ycap outputs per call; an inner-loop iteration about to store output number ycap does not run, the channel becomes
stalled and ignores all input until reset() / reset_channel(c).  The sample of the stalling step has been pushed; the
step's closing statements (tau -= 1 ...) do not run."""
import numpy as np

NPFB_MAX = 128          # YAGI_SYMSYNC_NPFB_MAX
LS_MAX = 128            # YAGI_SYMSYNC_LS_MAX
CHANNELS_MAX = 1 << 20  # YAGI_SYMSYNC_CHANNELS_MAX

F = np.float32
_U64_MAX = np.uint64(2 ** 64 - 1)


class ConfigError(ValueError):
    pass


def design(k, npfb, h):
    """symsync.rs:37-79: the matched bank H and the derivative bank D, [npfb][Ls], rows against the window oldest first"""
    h = np.asarray(h, F)
    h_len = h.size
    if k < 2 or npfb == 0 or h_len == 0 or (h_len - 1) % npfb != 0:
        raise ConfigError("config")
    ls = h_len // npfb
    if npfb > NPFB_MAX or ls > LS_MAX or ls == 0 or h_len < 2:
        raise ConfigError("limits")
    dh = np.zeros(h_len, F)
    hdh_max = F(0.0)
    with np.errstate(all="ignore"):
        for i in range(h_len):
            if i == 0:
                dh[i] = h[i + 1] - h[h_len - 1]
            elif i == h_len - 1:
                dh[i] = h[0] - h[i - 1]
            else:
                dh[i] = h[i + 1] - h[i - 1]
            if abs(F(h[i] * dh[i])) > hdh_max or i == 0:
                hdh_max = abs(F(h[i] * dh[i]))
        if not np.isfinite(hdh_max) or hdh_max == 0:
            raise ConfigError("hdh_max")                      # deviation: the reference would build NaN taps
        s = F(0.06) / hdh_max
        for i in range(h_len):
            dh[i] = dh[i] * s

    def bank(t):                                              # firpfb.rs:42-52: the last tap of t is dropped
        out = np.zeros((npfb, ls), F)
        for i in range(npfb):
            for n in range(ls):
                out[i, ls - n - 1] = t[i + n * npfb]
        return out
    return bank(h), bank(dh)


def rnyquist_taps(ftype, k, m, beta, npfb):
    """symsync.rs:112-131; the prototype is the library's host design (no device needed)"""
    import yagi_amd as ya
    if k < 2 or m == 0 or not (0.0 <= beta <= 1.0) or npfb == 0:
        raise ConfigError("config")
    return np.asarray(ya.fir_design_prototype(ftype, k * npfb, m, beta, 0.0), F)


def kaiser_taps(k, m, beta, npfb):
    """symsync.rs:133-158"""
    import yagi_amd as ya
    if k < 2 or m == 0 or not (0.0 < beta <= 1.0) or npfb == 0:
        raise ConfigError("config")
    fc = F(0.75)
    h = np.asarray(ya.fir_design_kaiser(2 * npfb * k * m + 1, fc / (F(k) * F(npfb)), 40.0, 0.0), F)
    return (h * (F(2.0) * fc)).astype(F)


def lf_coefficients(bw):
    """set_lf_bw (:196-213) in f32, normalised by a0 as IirFilterSos::set_coefficients: (b[3], a[3], rate_adjustment)"""
    bw = F(bw)
    if not (bw >= 0.0 and bw <= 1.0):
        raise ConfigError("bandwidth must be in [0,1]")
    alpha = F(1.0) - bw
    beta = F(0.22) * bw
    a, b = F(0.5), F(0.495)
    bc = [beta, F(0.0), F(0.0)]
    ac = [F(1.0) - a * alpha, -b * alpha, F(0.0)]
    a0 = ac[0]
    with np.errstate(all="ignore"):
        return [F(v / a0) for v in bc], [F(v / a0) for v in ac], F(0.5) * bw


def _round_usize(bf):
    """`bf.round() as usize`: half away from zero, saturating, negative and NaN give 0; uint64 array"""
    d = np.asarray(bf, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.trunc(d + np.copysign(0.5, d))
        r = np.where(np.isnan(r) | (r < 0), 0.0, r)
        big = r >= 2.0 ** 64
        out = np.where(big, 0.0, r).astype(np.uint64)
    out[big] = _U64_MAX
    return out


class SymSyncRef:
    def __init__(self, channels, k, npfb, h):
        if not 1 <= channels <= CHANNELS_MAX:
            raise ConfigError("channels")
        self.H, self.D = design(k, npfb, h)
        self.C, self.k, self.npfb, self.ls = int(channels), int(k), int(npfb), self.H.shape[1]
        self.k_out = 1
        C_ = self.C
        self.wm = np.zeros((self.ls, C_), np.complex64)        # the matched filter's window, oldest first
        self.wd = np.zeros((self.ls, C_), np.complex64)        # the derivative filter's
        z = lambda: np.zeros(C_, F)
        self.tau, self.tau_decim, self.bf, self.rate, self.del_, self.q, self.q_hat = (z() for _ in range(7))
        self.v = [z(), z(), z()]
        self.b = np.zeros(C_, np.uint64)
        self.decim = np.zeros(C_, np.uint64)
        self.stalled = np.zeros(C_, bool)
        self.locked = False
        self.reset()
        self.set_lf_bw(0.01)

    @classmethod
    def rnyquist(cls, channels, ftype, k, m, beta, npfb):
        return cls(channels, k, npfb, rnyquist_taps(ftype, k, m, beta, npfb))

    @classmethod
    def kaiser(cls, channels, k, m, beta, npfb):
        return cls(channels, k, npfb, kaiser_taps(k, m, beta, npfb))

    def clone(self):
        import copy
        return copy.deepcopy(self)

    def reset(self):
        for c in range(self.C):
            self.reset_channel(c)

    def reset_channel(self, c):                                # :160-172: mf.reset() only; the derivative window stays
        self.wm[:, c] = 0
        self.rate[c] = F(self.k) / F(self.k_out)
        self.del_[c] = self.rate[c]
        self.b[c] = 0
        for a in (self.bf, self.tau, self.tau_decim, self.q, self.q_hat, *self.v):
            a[c] = 0
        self.decim[c] = 0
        self.stalled[c] = False

    def lock(self):
        self.locked = True

    def unlock(self):
        self.locked = False

    def set_output_rate(self, k_out):
        if k_out == 0:
            raise ConfigError("output rate must be greater than 0")
        self.k_out = int(k_out)
        self.rate[:] = F(self.k) / F(self.k_out)
        self.del_[:] = self.rate

    def set_lf_bw(self, bw):
        self.lb, self.la, self.rate_adjustment = lf_coefficients(bw)

    def get_tau(self):
        return self.tau_decim.copy()

    def _sum(self, bank, rows, w, run):
        """dotprod of row rows[c] of the bank against window column c, oldest first, from +0.0, unfused"""
        t = bank[rows]                                          # [C][Ls]
        re, im = np.zeros(self.C, F), np.zeros(self.C, F)
        for j in range(self.ls):
            re = re + t[:, j] * w[j].real
            im = im + t[:, j] * w[j].imag
        return re, im

    def execute(self, x, ycap):
        """x[n][C] -> (y[ycap][C], ny[C], stalled[C]); rows >= ny[c] of a column stay zero"""
        x = np.asarray(x, np.complex64).reshape(-1, self.C)
        n = x.shape[0]
        y = np.zeros((ycap, self.C), np.complex64)
        ny = np.zeros(self.C, np.int64)
        npfb = np.uint64(self.npfb)
        kf, zero = F(self.k), F(0.0)
        norm = kf * kf + zero * zero
        cols = np.arange(self.C)
        with np.errstate(all="ignore"):
            for s in range(n):
                live = ~self.stalled
                if not live.any():
                    break
                # self.mf.push(x); self.dmf.push(x)
                self.wm[:, live] = np.concatenate([self.wm[1:, live], x[s:s + 1, live]])
                self.wd[:, live] = np.concatenate([self.wd[1:, live], x[s:s + 1, live]])
                while True:
                    run = live & (self.b < npfb)               # while self.b < self.npfb
                    st = run & (ny >= ycap)                    # the capacity rule
                    self.stalled |= st
                    live = live & ~st
                    run = run & ~st
                    if not run.any():
                        break
                    rows = np.where(run, self.b, 0).astype(np.int64)
                    mr, mi = self._sum(self.H, rows, self.wm, run)   # mf = self.mf.execute(self.b)
                    # y[ny] = mf / Complex(k as f32, 0): num-complex's complex division
                    yr = (mr * kf + mi * zero) / norm
                    yi = (mi * kf - mr * zero) / norm
                    yv = np.empty(self.C, np.complex64)
                    yv.real, yv.imag = yr, yi
                    y[ny[run], cols[run]] = yv[run]
                    upd = run & (self.decim == np.uint64(self.k_out))
                    self.decim[upd] = 0
                    if self.locked:
                        adv = run & ~upd                       # `continue`: the iteration is repeated
                    else:
                        adv = run
                        if upd.any():
                            dr, di = self._sum(self.D, rows, self.wd, upd)   # dmf = self.dmf.execute(self.b)
                            # q = (mf.conj() * dmf).re(): a.re b.re - a.im b.im with a = (mr, -mi)
                            q = mr * dr - (-mi) * di
                            q = np.where(q < F(-1.0), F(-1.0), np.where(q > F(1.0), F(1.0), q))   # clamp passes NaN
                            # pll.execute(q): execute_df2
                            v2, v1 = self.v[1], self.v[0]
                            v0 = q - self.la[1] * v1 - self.la[2] * v2
                            qh = self.lb[0] * v0 + self.lb[1] * v1 + self.lb[2] * v2
                            rate = self.rate + self.rate_adjustment * qh
                            del_ = rate + qh
                            for dst, src in ((self.q, q), (self.q_hat, qh), (self.v[2], v2), (self.v[1], v1),
                                             (self.v[0], v0), (self.rate, rate), (self.del_, del_),
                                             (self.tau_decim, self.tau)):
                                dst[upd] = src[upd]
                    self.decim[adv] += np.uint64(1)
                    tau = self.tau + self.del_
                    bf = tau * F(self.npfb)
                    b = _round_usize(bf)
                    self.tau[adv], self.bf[adv], self.b[adv] = tau[adv], bf[adv], b[adv]
                    ny[adv] += 1
                self.tau[live] = (self.tau - F(1.0))[live]
                self.bf[live] = (self.bf - F(self.npfb))[live]
                self.b[live] -= npfb
        return y, ny.astype(np.uint32), self.stalled.astype(np.uint32)


class SymSyncScalar:
    """One channel, word for word, on the oracle's filter banks."""

    def __init__(self, k, npfb, h):
        from oracle import oracle
        self.H, self.D = design(k, npfb, h)
        h = np.asarray(h, F)
        self.k, self.npfb, self.k_out = int(k), int(npfb), 1
        ls = self.H.shape[1]
        self.mf = oracle.FirPfbFilter("crcf", npfb, h, h.size)
        self.oracle, self.wd = oracle, np.zeros(ls, np.complex64)
        self.locked, self.stalled = False, False
        self.v = [F(0), F(0), F(0)]
        self.reset()
        self.set_lf_bw(0.01)

    def reset(self):
        self.mf.reset()
        self.rate = F(self.k) / F(self.k_out)
        self.del_ = self.rate
        self.b = 0
        self.bf = self.tau = self.tau_decim = self.q = self.q_hat = F(0)
        self.decim = 0
        self.v = [F(0), F(0), F(0)]
        self.stalled = False

    def set_output_rate(self, k_out):
        self.k_out = int(k_out)
        self.rate = F(self.k) / F(self.k_out)
        self.del_ = self.rate

    def set_lf_bw(self, bw):
        self.lb, self.la, self.rate_adjustment = lf_coefficients(bw)

    def execute(self, x, ycap):
        y, ny = np.zeros(ycap, np.complex64), 0
        kf, zero = F(self.k), F(0.0)
        norm = kf * kf + zero * zero
        with np.errstate(all="ignore"):
            for xi in np.asarray(x, np.complex64):
                if self.stalled:
                    break
                self.mf.push(xi)
                self.wd = np.append(self.wd[1:], xi)              # dmf.push
                while self.b < self.npfb:
                    if ny >= ycap:
                        self.stalled = True
                        break
                    mf = self.mf.execute(self.b)
                    mr, mi = F(mf.real), F(mf.imag)
                    y[ny] = complex(F(F(mr * kf) + F(mi * zero)) / norm, F(F(mi * kf) - F(mr * zero)) / norm)
                    if self.decim == self.k_out:
                        self.decim = 0
                        if self.locked:
                            continue
                        dmf = self.oracle.dotprod("rcc", self.D[self.b], self.wd)
                        dr, di = F(dmf.real), F(dmf.imag)
                        q = F(F(mr * dr) - F(F(-mi) * di))
                        q = F(-1.0) if q < F(-1.0) else F(1.0) if q > F(1.0) else q
                        self.q = q
                        self.v[2] = self.v[1]
                        self.v[1] = self.v[0]
                        self.v[0] = F(F(q - F(self.la[1] * self.v[1])) - F(self.la[2] * self.v[2]))
                        self.q_hat = F(F(F(self.lb[0] * self.v[0]) + F(self.lb[1] * self.v[1])) + F(self.lb[2] * self.v[2]))
                        self.rate = F(self.rate + F(self.rate_adjustment * self.q_hat))
                        self.del_ = F(self.rate + self.q_hat)
                        self.tau_decim = self.tau
                    self.decim += 1
                    self.tau = F(self.tau + self.del_)
                    self.bf = F(self.tau * F(self.npfb))
                    self.b = int(_round_usize(np.array([self.bf]))[0])
                    ny += 1
                if self.stalled:
                    break
                self.tau = F(self.tau - F(1.0))
                self.bf = F(self.bf - F(self.npfb))
                self.b -= self.npfb
        return y, ny, self.stalled


def default_ycap(n, k, k_out):
    """the Python package's default capacity: a default, not a bound"""
    return 2 * -(-n * k_out // k) + 8


# ---- streams and comparisons the tests share ---------------------------------------------------------------------------
def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize in (4, 8) and a.dtype.kind in "fc" else a


def same_words(a, b):
    """bit for bit, a NaN matching any NaN (sign and payload of a NaN differ between instruction sets)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "c":
        a, b = np.ascontiguousarray(a).view(np.float32), np.ascontiguousarray(b).view(np.float32)
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (words(a) == words(b))))


def below(y, ny):
    """the words a call defines: y[j, c] for j < ny[c], as a list of columns"""
    return [np.asarray(y)[:int(ny[c]), c].copy() for c in range(len(ny))]


def same_outputs(a, b):
    """(y, ny, stalled) of two forms: the same counts, flags and words below ny"""
    (ya_, na, sa), (yb, nb, sb) = a[:3], b[:3]
    return (np.array_equal(na, nb) and np.array_equal(sa, sb)
            and all(same_words(u, v) for u, v in zip(below(ya_, na), below(yb, nb))))


def noise(seed, n, channels, amp=0.5):
    """N(0, amp^2 / 2) per component; amp may be one value or one per channel"""
    r = np.random.default_rng(seed)
    x = (r.standard_normal((n, channels)) + 1j * r.standard_normal((n, channels))) * np.sqrt(0.5)
    return (x * np.asarray(amp)).astype(np.complex64)


def qpsk_symbols(nsym):
    """symsync.rs:419-427: QPSK from MSequence::create_default(10)"""
    from sequence_ref import MSequence
    ms = MSequence(10, 0x240, 1)
    s = np.zeros(nsym, np.complex64)
    r = F(np.sqrt(0.5))
    for i in range(nsym):
        si = ms.generate_symbol(1)
        sq = ms.generate_symbol(1)
        s[i] = complex(r if si == 0 else -r, r if sq == 0 else -r)
    return s


def interp_dt(k, tau):
    """symsync.rs:401-408: the interpolator's fractional sample offset for a fractional symbol offset tau"""
    while tau < 0.0:
        tau += 1.0
    g = k * tau
    dt = g - np.floor(g)
    return dt - 1.0 if dt > 0.5 else dt


def qpsk_stream(nsym, tau, k=2, m=7, beta=0.35):
    """(symbols, samples): the symbols through the Arkaiser interpolator FirInterpolationFilter::new_prototype designs
    (k branches of the 2km + 1 prototype at offset dt), no resampler"""
    import yagi_amd as ya
    s = qpsk_symbols(nsym)
    h = np.asarray(ya.fir_design_prototype(ya.FirFilterShape.Arkaiser, k, m, beta, interp_dt(k, tau)), np.float64)
    up = np.zeros(nsym * k, np.complex128)
    up[::k] = s
    return s, np.convolve(up, h)[:nsym * k].astype(np.complex64)


LOCK_TAUS = (0.0, -0.25, 0.1, 0.4)
LOCK_TOL = 0.2           # symsync.rs:376


def lock_errors(z, nz, s, m=7, ntest=100):
    """|z[i] - s[i - 2m]| over the last ntest outputs"""
    i = np.arange(nz - ntest, nz)
    return np.abs(z[i] - s[i - 2 * m])


# ---- the GPU tests' shared plumbing --------------------------------------------------------------------------------------
def run_dev(ya, q, x, ycap, x_pitch=None, y_pitch=None):
    """SymSync.execute_devptr on plain device buffers: x[n][C] -> (y[ycap][C], ny, stalled); y starts as zeros"""
    x = np.asarray(x, np.complex64)
    n, C = x.shape
    xp, yp = x_pitch or C, y_pitch or C
    wide = np.zeros((n, xp), np.complex64)
    wide[:, :C] = x
    xd = ya.DeviceArray.from_numpy(wide) if n else ya.DeviceArray(1, np.complex64)
    yd = ya.DeviceArray(max(ycap * yp, 1), np.complex64)
    yd.zero()
    sd = ya.DeviceArray(2 * C, np.uint32)
    q.execute_devptr(xd.ptr, xp, n, yd.ptr, yp, ycap, sd.ptr)
    ya.synchronize()
    st = sd.to_numpy()
    y = yd.to_numpy()[:ycap * yp].reshape(ycap, yp)[:, :C].copy()
    for d in (xd, yd, sd):
        d.free()
    return y, st[:C].copy(), st[C:].copy()


def streams(k, n, channels, seed):
    """n steps for `channels` channels that pull the lanes of a wave apart: noise of amplitudes 0.5, 4 (q clamps, del
    wanders), 0.2, 1 and 2 in turn, and on every fifth channel QPSK at one of four timing offsets"""
    amps = np.array([0.5, 4.0, 0.2, 1.0, 2.0])[np.arange(channels) % 5]
    x = noise(seed, n, channels, amps)
    nsym = -(-n // k)
    for i, tau in enumerate(LOCK_TAUS):
        cols = np.arange(channels)[(np.arange(channels) % 5 == 0) & ((np.arange(channels) // 5) % 4 == i)]
        if cols.size:
            x[:, cols] = qpsk_stream(nsym, tau, k=k, m=3)[1][:n, None]
    return x


def concat(parts, channels):
    """the per-channel output streams of consecutive calls [(y, ny, stalled), ...]"""
    return [np.concatenate([y[:int(ny[c]), c] for y, ny, _ in parts]) for c in range(channels)]
