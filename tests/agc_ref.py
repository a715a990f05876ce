"""Restatement of agc::Agc (src/agc/agc.rs) for a bank of C independent channels, as yagi_amd.Agc defines it
(include/yagi_hip.h), written independently of the C source: the loop in np.float32 scalars, statement by statement, and
the library's three words (ln, exp, log10) in plain Python floats (IEEE f64, every operation rounded on its own) with
math.frexp / math.ldexp for the exponent.  `words` selects the three functions, so the same loop also runs on the
platform's logf / expf / log10f (libm_words) for the comparison of DESIGN.md section 6."""
import ctypes
import ctypes.util
import math

import numpy as np

F = np.float32
CHANNELS_MAX = 1 << 20   # YAGI_AGC_CHANNELS_MAX
DISABLED, ENABLED, RISE, SIGNALHI, FALL, SIGNALLO, TIMEOUT = range(7)

LN2 = float.fromhex("0x1.62e42fefa39efp-1")
INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42feep-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
LN10 = float.fromhex("0x1.26bb1bbb55516p+1")
INV_LN10 = float.fromhex("0x1.bcb7b1526e50ep-2")
SQRT2 = float.fromhex("0x1.6a09e667f3bcdp+0")
LN_COEF = [1.0 / k for k in range(23, 0, -2)]                       # 1/23 .. 1/3, 1
EXP_COEF = [1.0 / math.factorial(k) for k in range(14, -1, -1)]     # 1/14! .. 1/1!, 1/0!


class ConfigError(ValueError):
    pass


# ---- the words ---------------------------------------------------------------------------------------------------------
def ln64(x):
    """x a positive finite float: x = 2^e m, m in [sqrt 1/2, sqrt 2); s = (m - 1) / (m + 1); e LN2 + 2 s p(s^2)"""
    m, e = math.frexp(x)                                            # m in [0.5, 1)
    m, e = m * 2.0, e - 1                                           # [1, 2)
    if m >= SQRT2:
        m, e = m * 0.5, e + 1
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = LN_COEF[0]
    for c in LN_COEF[1:]:
        p = p * z + c
    return float(e) * LN2 + (2.0 * s) * p


def exp64(x):
    """x not a NaN, clamped to [-110, 95]: k = floor(x / ln 2 + 1/2), r = (x - k HI) - k LO, Taylor to r^14 / 14!, 2^k"""
    x = -110.0 if x < -110.0 else x
    x = 95.0 if x > 95.0 else x
    k = math.floor(x * INV_LN2 + 0.5)
    kd = float(k)
    r = (x - kd * LN2_HI) - kd * LN2_LO
    p = EXP_COEF[0]
    for c in EXP_COEF[1:]:
        p = p * r + c
    return math.ldexp(p, k)


def _ln_special(x):
    if x != x or x < 0:
        return F(np.nan)
    if x == 0:
        return F(-np.inf)
    if x == np.inf:
        return F(np.inf)
    return None


def _f32(v):
    with np.errstate(all="ignore"):
        return F(v)


def lnf(x):
    x = F(x)
    sp = _ln_special(x)
    return sp if sp is not None else _f32(ln64(float(x)))


def log10f(x):
    x = F(x)
    sp = _ln_special(x)
    return sp if sp is not None else _f32(ln64(float(x)) * INV_LN10)


def expf(x):
    x = F(x)
    if x != x:
        return x
    return _f32(exp64(float(x)))


def exp10_rssi(rssi):
    """set_rssi's 10^(-rssi / 20)"""
    with np.errstate(all="ignore"):
        t = -F(rssi) / F(20.0)
    if t != t:
        return t
    with np.errstate(all="ignore"):
        return _f32(exp64(float(t) * LN10))


class Words:
    def __init__(self, ln, exp, log10):
        self.ln, self.exp, self.log10 = ln, exp, log10


OWN = Words(lnf, expf, log10f)


def libm_words():
    """the platform's logf / expf / log10f"""
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    out = []
    for name in ("logf", "expf", "log10f"):
        fn = getattr(m, name)
        fn.argtypes, fn.restype = [ctypes.c_float], ctypes.c_float
        out.append(lambda x, fn=fn: F(fn(float(F(x)))))
    return Words(*out)


# ---- one channel, statement by statement ----------------------------------------------------------------------------------
class AgcScalar:
    """agc.rs:37-248 for one channel; T is complex (crcf) or real (rrrf)"""

    def __init__(self, cplx=True, words=OWN):
        self.cplx, self.w = cplx, words
        self.g = self.y2_prime = F(0)
        self.is_locked = False
        self.squelch_mode = DISABLED
        self.squelch_timer = 0
        self.set_bandwidth(1e-2)
        self.reset()
        self.squelch_threshold, self.squelch_timeout = F(0), 100
        self.scale = F(1)

    def reset(self):
        self.g, self.y2_prime, self.is_locked = F(1), F(1), False
        self.squelch_mode = DISABLED if self.squelch_mode == DISABLED else ENABLED

    def set_bandwidth(self, bt):
        if not 0.0 <= bt <= 1.0:
            raise ConfigError("bandwidth must be in [0, 1]")
        self.alpha = F(bt)

    def set_scale(self, scale):
        if not scale > 0:
            raise ConfigError("scale must be greater than zero")
        self.scale = F(scale)

    def set_gain(self, gain):
        if not gain > 0:
            raise ConfigError("gain must be greater than zero")
        self.g = F(gain)

    def set_signal_level(self, x2):
        if not x2 > 0:
            raise ConfigError("signal level must be greater than zero")
        self._set_level(F(x2))

    def _set_level(self, x2):
        with np.errstate(all="ignore"):
            self.g = F(1) / x2
        self.y2_prime = F(1)

    def set_rssi(self, rssi):
        g = exp10_rssi(rssi)
        self.g = g if g >= F(1e-16) else F(1e-16)                   # f32::max: a NaN becomes 1e-16
        self.y2_prime = F(1)

    def get_signal_level(self):
        with np.errstate(all="ignore"):
            return F(1) / self.g

    def get_rssi(self):
        with np.errstate(all="ignore"):
            return F(-20.0) * self.w.log10(self.g)

    def squelch_enable(self):
        self.squelch_mode = ENABLED

    def squelch_disable(self):
        self.squelch_mode = DISABLED

    def squelch_set_timeout(self, timeout):
        if not 1 <= timeout < 1 << 32:
            raise ConfigError("timeout")
        self.squelch_timeout = int(timeout)

    def init(self, x):
        if len(x) == 0:
            raise ConfigError("number of samples must be greater than zero")
        acc = F(0)
        with np.errstate(all="ignore"):
            for v in x:
                acc = acc + self._norm(*self._parts(v))
            x2 = np.sqrt(acc / F(len(x))) + F(1e-16)
        self._set_level(F(x2))

    def _parts(self, x):
        return (F(x.real), F(x.imag)) if self.cplx else (F(x), F(0))

    def _norm(self, re, im):
        return re * re - im * (-im) if self.cplx else re * re

    def execute(self, x):
        with np.errstate(all="ignore"):
            re, im = self._parts(x)
            re, im = re * self.g, im * self.g
            y2 = self._norm(re, im)
            self.y2_prime = (F(1) - self.alpha) * self.y2_prime + self.alpha * y2
            if self.is_locked:
                return self._out(re, im)
            if self.y2_prime > F(1e-6):
                self.g = self.g * self.w.exp(F(-0.5) * self.alpha * self.w.ln(self.y2_prime))
            self.g = self.g if self.g < F(1e6) else F(1e6)          # f32::min: a NaN becomes 1e6
            self._squelch_update()
            return self._out(re * self.scale, im * self.scale)

    def _out(self, re, im):
        return complex(re, im) if self.cplx else re

    def _squelch_update(self):
        hi = bool(self.get_rssi() > self.squelch_threshold)
        m = self.squelch_mode
        if m == ENABLED:
            m = RISE if hi else ENABLED
        elif m == RISE:
            m = SIGNALHI if hi else FALL
        elif m == SIGNALHI:
            m = SIGNALHI if hi else FALL
        elif m == FALL:
            self.squelch_timer = self.squelch_timeout
            m = SIGNALHI if hi else SIGNALLO
        elif m == SIGNALLO:
            self.squelch_timer -= 1
            m = TIMEOUT if self.squelch_timer == 0 else SIGNALHI if hi else SIGNALLO
        elif m == TIMEOUT:
            m = ENABLED
        self.squelch_mode = m


# ---- the bank ------------------------------------------------------------------------------------------------------------
class AgcRef:
    """C AgcScalar objects behind the interface of yagi_amd.Agc"""

    def __init__(self, channels, kind="crcf", words=OWN):
        if not 1 <= channels <= CHANNELS_MAX:
            raise ConfigError("channels")
        if kind not in ("crcf", "rrrf"):
            raise ConfigError("kind")
        self.C, self.kind, self.cplx = int(channels), kind, kind == "crcf"
        self.T = np.complex64 if self.cplx else np.float32
        self.q = [AgcScalar(self.cplx, words) for _ in range(self.C)]

    def clone(self):
        import copy
        return copy.deepcopy(self)

    def _all(self, name, *args):
        for q in self.q:
            getattr(q, name)(*args)

    def reset(self):
        self._all("reset")

    def reset_channel(self, c):
        if not 0 <= c < self.C:
            raise ConfigError("channel")
        self.q[c].reset()

    def lock(self):
        self.set_locked(np.ones(self.C, np.uint8))

    def unlock(self):
        self.set_locked(np.zeros(self.C, np.uint8))

    def is_locked(self):
        return all(q.is_locked for q in self.q)

    def set_locked(self, locked):
        for q, v in zip(self.q, locked):
            q.is_locked = bool(v)

    def get_locked(self):
        return np.array([q.is_locked for q in self.q], np.uint8)

    def set_bandwidth(self, bt):
        self._all("set_bandwidth", bt)

    def set_scale(self, scale):
        self._all("set_scale", scale)

    def set_gain(self, g):
        self._all("set_gain", g)

    def set_gains(self, g):
        if not all(v > 0 for v in g):
            raise ConfigError("gain must be greater than zero")
        for q, v in zip(self.q, g):
            q.set_gain(v)

    def set_signal_level(self, x2):
        self._all("set_signal_level", x2)

    def set_rssi(self, rssi):
        self._all("set_rssi", rssi)

    def get_gain(self):
        return np.array([q.g for q in self.q], F)

    def get_signal_level(self):
        return np.array([q.get_signal_level() for q in self.q], F)

    def get_rssi(self):
        return np.array([q.get_rssi() for q in self.q], F)

    def squelch_enable(self):
        self._all("squelch_enable")

    def squelch_disable(self):
        self._all("squelch_disable")

    def squelch_set_threshold(self, t):
        for q in self.q:
            q.squelch_threshold = F(t)

    def squelch_set_timeout(self, t):
        self._all("squelch_set_timeout", t)

    def squelch_get_status(self):
        return np.array([q.squelch_mode for q in self.q], np.uint8)

    def init(self, x):
        x = np.asarray(x, self.T)
        for c, q in enumerate(self.q):
            q.init(x[:, c])

    def execute_block(self, x, edges=None):
        """x[n, C] -> (y[n, C], status[n, C]); edges, a set, collects the (mode before, mode after) pairs"""
        x = np.asarray(x, self.T)
        y, st = np.zeros_like(x), np.zeros(x.shape, np.uint8)
        for c, q in enumerate(self.q):
            for i in range(x.shape[0]):
                before = q.squelch_mode
                y[i, c] = q.execute(x[i, c])
                st[i, c] = q.squelch_mode
                if edges is not None and not q.is_locked:
                    edges.add((before, q.squelch_mode))
        return y, st


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


def noise(seed, n, channels, amp=1.0, kind="crcf"):
    """unit-power noise times amp (one value or one per channel)"""
    r = np.random.default_rng(seed)
    if kind == "crcf":
        x = (r.standard_normal((n, channels)) + 1j * r.standard_normal((n, channels))) * np.sqrt(0.5)
        return (x * np.asarray(amp)).astype(np.complex64)
    return (r.standard_normal((n, channels)) * np.asarray(amp)).astype(np.float32)


def amplitudes(channels):
    """per-channel levels spread over 1e-4 .. 1e2"""
    return 10.0 ** (-4.0 + 6.0 * ((np.arange(channels) * 7) % 13) / 12.0)


def squelch_stimulus(n=2000, kind="crcf"):
    """the reference's squelch test signal (:432-446) in f32"""
    out = np.zeros(n, np.complex64)
    pi = F(np.pi)
    for i in range(n):
        if i < 500:
            gamma = F(1e-3)
        elif i < 550:
            gamma = F(1e-3) + (F(1e-2) - F(1e-3)) * (F(0.5) - F(0.5) * np.cos((pi * F(i - 500)) / F(50.0), dtype=F))
        elif i < 1450:
            gamma = F(1e-2)
        elif i < 1500:
            gamma = F(1e-3) + (F(1e-2) - F(1e-3)) * (F(0.5) + F(0.5) * np.cos((pi * F(i - 1450)) / F(50.0), dtype=F))
        else:
            gamma = F(1e-3)
        ph = F(2.0) * pi * F(0.0193) * F(i)
        out[i] = complex(gamma * np.cos(ph, dtype=F), gamma * np.sin(ph, dtype=F))
    return out if kind == "crcf" else np.ascontiguousarray(out.real)


def hopping(seed, n, channels, kind="crcf"):
    """levels that hop about a squelch threshold from row to row: runs of 1 to 6 rows at one of two levels 40 dB apart,
    another draw per channel, times the per-channel amplitudes"""
    r = np.random.default_rng(seed)
    lvl = np.zeros((n, channels))
    for c in range(channels):
        i = 0
        hi = bool(r.integers(0, 2))
        while i < n:
            run = int(r.integers(1, 7))
            lvl[i:i + run, c] = 1.0 if hi else 1e-2
            hi, i = not hi, i + run
    return _tone(n, channels, kind) * (lvl * amplitudes(channels)).astype(F)


def _tone(n, channels, kind):
    ph = 0.37 * np.arange(n)[:, None] + 0.11 * np.arange(channels)[None, :]
    if kind == "crcf":
        return np.exp(1j * ph).astype(np.complex64)
    return (np.sign(np.cos(ph)) + (np.cos(ph) == 0)).astype(np.float32)


def streams(n, channels, seed, kind="crcf"):
    """n rows for `channels` channels: noise on the even and hopping tones on the odd channels at amplitudes spread over
    1e-4 .. 1e2; channel 1 (where there is one) all zero, channel 3 with one NaN, channel 4 with one Inf sample"""
    x = noise(seed, n, channels, amplitudes(channels), kind)
    h = hopping(seed + 7, n, channels, kind)
    x[:, 1::2] = h[:, 1::2]
    if channels > 1:
        x[:, 1] = 0
    if channels > 3 and n > 8:
        x[n // 3, 3] = np.nan
    if channels > 4 and n > 8:
        x[n // 2, 4] = np.inf
    return x


# ---- the GPU tests' shared plumbing --------------------------------------------------------------------------------------
def run_dev(ya, q, x, status=False, pad=0):
    """Agc.execute_block_devptr on plain device buffers whose pitches are C + pad; y and the status plane start as zeros
    and are returned whole, [n][C + pad]"""
    x = np.asarray(x, q.T)
    n, C = x.shape
    pitch = C + pad
    wide = np.full((max(n, 1), pitch), 5, q.T)
    wide[:n, :C] = x
    xd = ya.DeviceArray.from_numpy(wide)
    yd = ya.DeviceArray(max(n, 1) * pitch, q.T)
    yd.zero()
    sd = None
    if status:
        sd = ya.DeviceArray(max(n, 1) * pitch, np.uint8)
        sd.zero()
    q.execute_block_devptr(xd.ptr, pitch, n, yd.ptr, pitch, None if sd is None else sd.ptr, pitch)
    ya.synchronize()
    y = yd.to_numpy()[:n * pitch].reshape(n, pitch).copy()
    st = None if sd is None else sd.to_numpy()[:n * pitch].reshape(n, pitch).copy()
    for b in (xd, yd, sd):
        if b is not None:
            b.free()
    return y, st
