"""SymTrack's definition (include/yagi_hip.h, "SymTrack: the definition") restated as a per-channel loop over the scalar
restatements of its parts: AgcScalar, SymSyncScalar, OscRef, EqLmsScalar and RefModem, imported as they are (a helper,
not a conftest).  The order of the statements is the definition's, including the two stall rules; nothing here is
shared with the library's source."""
import numpy as np

import agc_ref
import eqlms_ref
import modem_ref
import osc_ref
import symsync_ref
from symsync_ref import same_words                      # bit for bit, a NaN matching any NaN

F = np.float32
OFF, CM, DD = 0, 1, 2                                   # YAGI_SYMTRACK_EQ_*
STALL_CAPACITY, STALL_PLL = 1, 2                        # YAGI_SYMTRACK_STALL_*
PLL_ARG_MAX = F(256.0)                                  # YAGI_SYMTRACK_PLL_ARG_MAX
CHANNELS_MAX = 1 << 20
LDS_MAX = 160 * 1024
# an 8-point table whose balancing and scaling are exact (mean 0, energy 98 / 8 = 3.5^2), so that the f32 design of
# modem_ref.py and the library's f64 design give the same words
ARB8 = np.array([3 + 3j, -3 + 3j, 3 - 3j, -3 - 3j, 2.5 + 0.5j, -2.5 + 0.5j, 2.5 - 0.5j, -2.5 - 0.5j], np.complex64)


class ConfigError(ValueError):
    pass


def modem_design(scheme):
    """scheme: a ModulationScheme name such as "Qpsk", or a table of points"""
    if isinstance(scheme, str):
        kind, bps = modem_ref.SCHEMES[scheme]
        if kind in (modem_ref.PSK, modem_ref.DPSK):
            raise ConfigError("PSK and DPSK are not built")
        return modem_ref.design(kind, bps)
    t = np.asarray(scheme, np.complex64)
    bps = int(t.size).bit_length() - 1
    if t.ndim != 1 or t.size < 2 or t.size > 256 or (1 << bps) != t.size:
        raise ConfigError("table size must be a power of 2 in 2..256")
    return modem_ref.design(modem_ref.ARB, bps, t)


def lds_bytes(ls, eq_len, vco, M):
    """the lane-strided tiles (64 lanes of 8 bytes per slot), the 16 staged rows, the oscillator table, the constellation
    and reference[]"""
    return 512 * ls + 2 * 512 * eq_len + 16 * 512 + 1024 * (16 if vco else 8) + 8 * M + 32


class SymTrackScalar:
    """one channel"""

    def __init__(self, h, k, npfb, eq_h, D, vco):
        self.h, self.k, self.npfb = np.asarray(h, F), k, npfb
        self.agc = agc_ref.AgcScalar(True)
        self.sync = symsync_ref.SymSyncScalar(k, npfb, h)
        self.sync.set_output_rate(2)
        self.nco = osc_ref.OscRef(vco)
        self.eq = eqlms_ref.EqLmsScalar(len(eq_h), eq_h)
        self.demod = modem_ref.RefModem(D)
        self.strategy, self.holdoff = CM, 200
        self.index = self.num_syms = self.stall = 0
        self.hist = []                                      # what the matched filter's window holds besides zeros

    def reset(self):
        self.agc.reset()
        self.sync.reset()
        self.nco.reset()
        self.eq.reset()
        self.demod.reset()
        self.index = self.num_syms = self.stall = 0
        self.hist = []

    def set_bandwidths(self, agc, sync, eq, pll):
        self.agc.set_bandwidth(agc)
        self.sync.set_lf_bw(sync)
        self.eq.mu = F(eq)
        self.nco.pll_set_bandwidth(pll)

    # The oracle's filter bank is a C object without a copy: its window is zeros and then self.hist, so a copy is a fresh
    # bank with those samples pushed.
    _SYNC_SHARED = ("mf", "oracle", "H", "D")

    def _sync_snapshot(self):
        import copy
        return ({k: copy.deepcopy(v) for k, v in self.sync.__dict__.items() if k not in self._SYNC_SHARED}, list(self.hist))

    def _sync_restore(self, snap):
        import copy
        fields, hist = snap
        self.sync.__dict__.update(copy.deepcopy(fields))
        self.sync.mf.reset()
        for v in hist:
            self.sync.mf.push(v)
        self.hist = list(hist)

    def clone(self):
        import copy
        new = copy.copy(self)
        for name in ("agc", "nco", "eq", "demod"):
            setattr(new, name, copy.deepcopy(getattr(self, name)))
        new.sync = symsync_ref.SymSyncScalar(self.k, self.npfb, self.h)
        new._sync_restore(self._sync_snapshot())
        return new

    def _push_and_sync(self, v, room):
        self.hist = (self.hist + [v])[-self.sync.H.shape[1]:]
        return self.sync.execute(np.array([v], np.complex64), room)

    def execute(self, x, ycap):
        """-> (d_hat[ny], sym[ny]) of this call"""
        y, sym = [], []
        with np.errstate(all="ignore"):
            for xi in np.asarray(x, np.complex64):
                if self.stall:
                    break
                v = np.complex64(self.agc.execute(xi))
                # the synchroniser's own capacity rule, counted in its outputs: the iteration that would emit symbol
                # number ycap is the next even-numbered output once ycap symbols are out
                room = 2 * (ycap - len(y)) + (self.index & 1)
                before = self._sync_snapshot()
                s, ns, full = self._push_and_sync(v, room)
                for i, si in enumerate(s[:ns]):
                    u = self.nco.mix_down(si)
                    self.nco.step()
                    self.eq.push(u)
                    j = self.index
                    self.index += 1
                    if j & 1:
                        continue
                    d_hat = self.eq.execute()
                    dc = np.complex64(complex(*d_hat))
                    sy = self.demod.demodulate(dc)
                    xh = self.demod.get_demodulator_sample()
                    e = self.demod.get_demodulator_phase_error()
                    fa, fb = F(e) * self.nco.alpha, F(e) * self.nco.beta
                    if abs(fa) >= PLL_ARG_MAX or abs(fb) >= PLL_ARG_MAX:
                        # the synchroniser's iterations behind this one have not run: again, with room for i + 1 only
                        self.stall = STALL_PLL
                        self._sync_restore(before)
                        self._push_and_sync(v, i + 1)
                        break
                    self.nco.pll_step(e)
                    if self.num_syms > self.holdoff and self.strategy != OFF:
                        if self.strategy == CM:
                            self.eq.step_blind(d_hat)
                        else:
                            self.eq.step((F(xh.real), F(xh.imag)), d_hat)
                    self.num_syms += 1
                    y.append(dc)
                    sym.append(sy)
                if full and not self.stall:
                    self.stall = STALL_CAPACITY
        return np.array(y, np.complex64), np.array(sym, np.uint8)


class SymTrackRef:
    """the bank: `channels` SymTrackScalar objects of one design, with the object's setters and getters"""

    def __init__(self, channels, ftype, k, m, beta, scheme, vco=False, npfb=16, eq_len=9):
        if not 1 <= channels <= CHANNELS_MAX:
            raise ConfigError("channels")
        D = modem_design(scheme)
        if k < 2:
            raise ConfigError("k")
        if not 1 <= eq_len <= eqlms_ref.LEN_MAX:
            raise ConfigError("eq_len")
        try:
            h = symsync_ref.rnyquist_taps(ftype, k, m, beta, npfb)
        except symsync_ref.ConfigError as e:
            raise ConfigError(str(e))
        if lds_bytes(2 * k * m, eq_len, vco, D.M) > LDS_MAX:
            raise ConfigError("LDS")
        eq_h = eqlms_ref.lowpass_h(eq_len, 0.45)
        self.channels, self.k, self.eq_len = channels, k, eq_len
        self.ch = [SymTrackScalar(h, k, npfb, eq_h, D, vco) for _ in range(channels)]
        self.set_bandwidth(0.9)

    def set_bandwidth(self, bw):
        if not bw >= 0:
            raise ConfigError("bw")
        bw = F(bw)
        self.set_bandwidths(F(0.02) * bw, F(0.001) * bw, F(0.02) * bw, F(0.001) * bw)

    def set_bandwidths(self, agc, sync, eq, pll):
        for c in self.ch:
            c.set_bandwidths(agc, sync, eq, pll)

    def set_eq_strategy(self, s):
        for c in self.ch:
            c.strategy = int(s)

    def set_eq_holdoff(self, n):
        for c in self.ch:
            c.holdoff = int(n)

    def set_nco(self, c, frequency, phase=0.0):
        w = osc_ref.constrain(frequency), osc_ref.constrain(phase)
        if None in w:
            raise ConfigError("constrain")
        self.ch[c].nco.d_theta, self.ch[c].nco.theta = w

    def set_nco_all(self, frequency, phase=None):
        for c in range(self.channels):
            self.set_nco(c, frequency[c], 0.0 if phase is None else phase[c])

    def reset(self):
        for c in self.ch:
            c.reset()

    def reset_channel(self, c):
        self.ch[c].reset()

    def clone(self):
        import copy
        new = copy.copy(self)
        new.ch = [c.clone() for c in self.ch]
        return new

    def execute(self, x, ycap):
        """x[n, channels] -> (y[ycap, channels], sym[ycap, channels], ny, stalled)"""
        x = np.asarray(x, np.complex64)
        y, sym = np.zeros((ycap, self.channels), np.complex64), np.zeros((ycap, self.channels), np.uint8)
        ny, st = np.zeros(self.channels, np.uint32), np.zeros(self.channels, np.uint32)
        for c, ch in enumerate(self.ch):
            if not ch.stall:
                yc, sc = ch.execute(x[:, c], ycap)
                ny[c] = len(yc)
                y[:len(yc), c], sym[:len(sc), c] = yc, sc
            st[c] = ch.stall
        return y, sym, ny, st

    # -- getters, as the object's
    def get_tau(self):
        return np.array([c.sync.tau_decim for c in self.ch], F)

    def get_gain(self):
        return np.array([c.agc.g for c in self.ch], F)

    def get_rssi(self):
        return np.array([c.agc.get_rssi() for c in self.ch], F)

    def get_nco_frequency(self):
        return np.array([c.nco.get_frequency() for c in self.ch], F)

    def get_nco_phase(self):
        return np.array([c.nco.get_phase() for c in self.ch], F)

    def get_nco_state(self):
        return (np.array([c.nco.theta for c in self.ch], np.uint32), np.array([c.nco.d_theta for c in self.ch], np.uint32))

    def get_weights(self):
        """Eqlms::get_weights (:121-123): conj(w0) reversed"""
        return np.array([np.conj(c.eq.get_coefficients()[::-1]) for c in self.ch], np.complex64)

    def get_num_syms(self):
        return np.array([c.num_syms for c in self.ch], np.uint64)

    def get_stalled(self):
        return np.array([c.stall for c in self.ch], np.uint32)


GETTERS = ("get_tau", "get_gain", "get_rssi", "get_nco_frequency", "get_nco_phase", "get_weights", "get_num_syms",
           "get_stalled")


def same_getters(q, r):
    """every getter of the object q against the restatement r, word for word; returns the names that differ"""
    bad = [g for g in GETTERS if not same_words(getattr(q, g)(), getattr(r, g)())]
    (th, dth), (rth, rdth) = q.get_nco_state(), r.get_nco_state()
    if not (np.array_equal(th, rth) and np.array_equal(dth, rdth)):
        bad.append("get_nco_state")
    return bad


def same_outputs(a, b):
    """(y, sym, ny, stalled) of two forms: the same counts, reasons and words below ny; returns what differs"""
    (ya_, sa, na, ta), (yb, sb, nb, tb) = a, b
    bad = []
    if not np.array_equal(na, nb):
        bad.append(("ny", na.tolist(), nb.tolist()))
    if not np.array_equal(ta, tb):
        bad.append(("stalled", ta.tolist(), tb.tolist()))
    for c in range(len(na)):
        n = int(min(na[c], nb[c]))
        if not same_words(np.asarray(ya_)[:n, c].copy(), np.asarray(yb)[:n, c].copy()):
            bad.append(("y", c))
        if sa is not None and sb is not None and not np.array_equal(np.asarray(sa)[:n, c], np.asarray(sb)[:n, c]):
            bad.append(("sym", c))
    return bad


# ---- stimuli the tests share ----------------------------------------------------------------------------------------------
FT = 6                                                   # FirFilterShape.Arkaiser
BETA = 0.3
SCHEMES = {"Bpsk": "Bpsk", "Qpsk": "Qpsk", "Ook": "Ook", "Ask4": "Ask4", "Qam16": "Qam16", "Qam64": "Qam64",
           "Qam32": "Qam32", "Arb8": ARB8}
#        C    k  m  npfb  eq_len  vco    n
SHAPES = [(1, 2, 2, 8, 9, False, 260),
          (63, 3, 2, 8, 2, True, 120),
          (64, 4, 3, 16, 9, False, 120),
          (65, 2, 2, 8, 9, True, 120),
          (200, 3, 2, 8, 2, False, 60),
          (3, 2, 7, 16, 9, False, 220),
          (2, 4, 8, 16, 64, True, 80),             # 112 KiB of LDS: past the 64 KiB a launch gets unasked
          (2, 8, 8, 128, 9, False, 120),           # 128 KiB of branch taps do not fit beside the tiles: they stay global
          (2, 2, 2, 8, 1, False, 60)]              # eq_len = 1: new_lowpass(1, .) is one NaN tap (a Kaiser window of one
                                                   # tap is 0 / 0), so every output is a NaN; the counts and states remain
#        scheme  vco   strategy  eq_len
KINDS = [("Bpsk", False, CM, 9), ("Qpsk", True, DD, 2), ("Ook", False, OFF, 9), ("Ask4", True, DD, 9),
         ("Qam16", False, DD, 9), ("Qam64", True, CM, 2), ("Qam32", False, DD, 9), ("Arb8", True, DD, 9)]


def pll_stimulus(C, k, m, n, victim, row):
    """ordinary streams with one sample of 1e30 in channel `victim`"""
    x = streams(51, "Qpsk", n, C, k, m, BETA)
    x[row, victim] = np.complex64(1e30)
    return x


def constellation(scheme):
    return modem_design(scheme).map


def modulated(seed, scheme, nsym, k, m=7, beta=0.3, ftype=None, tau=0.0, dphi=0.0, gain=1.0, snr_db=30.0, phase=0.0):
    """nsym symbols of `scheme` through the transmit pulse (the same root-Nyquist shape, delayed by tau of a symbol), a
    carrier offset of dphi radians per sample, a gain and noise at snr_db: (samples[nsym k], symbols[nsym])"""
    import yagi_amd as ya
    rng = np.random.default_rng(seed)
    cmap = constellation(scheme)
    s = rng.integers(0, cmap.size, nsym)
    ftype = FT if ftype is None else ftype
    h = np.asarray(ya.fir_design_prototype(ftype, k, m, beta, tau), np.float64)
    up = np.zeros(nsym * k, np.complex128)
    up[::k] = cmap[s]
    x = np.convolve(up, h)[:nsym * k]
    x = x * np.exp(1j * (dphi * np.arange(x.size) + phase)) * gain
    sigma = gain * np.sqrt(np.mean(np.abs(cmap) ** 2)) * 10.0 ** (-snr_db / 20.0)
    x = x + sigma * np.sqrt(0.5) * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return x.astype(np.complex64), s


def streams(seed, scheme, n, channels, k, m=3, beta=0.3):
    """x[n, channels]: every channel its own symbols, timing offset, carrier offset and gain"""
    x = np.zeros((n, channels), np.complex64)
    nsym = -(-n // k) + 1
    for c in range(channels):
        xc, _ = modulated(seed * 1000 + c, scheme, nsym, k, m, beta, tau=((c * 7) % 11 - 5) / 11.0,
                          dphi=0.03 * (((c * 5) % 9) - 4) / 4.0, gain=(0.05, 0.7, 2.5)[c % 3], snr_db=25.0, phase=0.4 * c)
        x[:, c] = xc[:n]
    return x


def cuts(n, sizes=(0, 1, 3, 17, 0, 45, 2, 91)):
    """row ranges that cut [0, n) into calls of the given sizes, cycling"""
    out, at, i = [], 0, 0
    while at < n:
        e = min(n, at + sizes[i % len(sizes)])
        out.append((at, e))
        at, i = e, i + 1
    return out


def run_dev(ya, q, x, ycap, pad=0, symbols=True):
    """SymTrack.execute_devptr on plain device buffers at pitch C + pad: x[n][C] -> (y[ycap][C], sym[ycap][C] or None, ny,
    stalled); y and sym start as zeros.  The third status plane, the low word of num_syms, is checked against the getter"""
    x = np.asarray(x, np.complex64)
    n, C = x.shape
    p = C + pad
    wide = np.zeros((n, p), np.complex64)
    wide[:, :C] = x
    xd = ya.DeviceArray.from_numpy(wide) if n else ya.DeviceArray(1, np.complex64)
    yd = ya.DeviceArray(max(ycap * p, 1), np.complex64)
    yd.zero()
    bd = ya.DeviceArray(max(ycap * p, 1), np.uint8)
    bd.zero()
    sd = ya.DeviceArray(3 * C, np.uint32)
    q.execute_devptr(xd.ptr, p, n, yd.ptr, p, bd.ptr if symbols else None, p, ycap, sd.ptr)
    ya.synchronize()
    st = sd.to_numpy()
    y = yd.to_numpy()[:ycap * p].reshape(ycap, p)[:, :C].copy()
    sym = bd.to_numpy()[:ycap * p].reshape(ycap, p)[:, :C].copy() if symbols else None
    for d in (xd, yd, bd, sd):
        d.free()
    assert np.array_equal(st[2 * C:], (q.get_num_syms() & 0xFFFFFFFF).astype(np.uint32))
    return y, sym, st[:C].copy(), st[C:2 * C].copy()
