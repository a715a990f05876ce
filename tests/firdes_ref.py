"""fir_design_prototype (include/yagi_hip.h; src/filter/fir/design/mod.rs:392-451) restated in numpy (a helper, not a test
module): the four shapes the library builds, every formula once, evaluated in the dtype it is asked for.  With
D = np.float32 it is the f32 restatement (operation by operation what the C code does, libm and rounding of fused
operations aside); with D = np.float64 the same formulas on the same f32 inputs give the reference value.  The branch
decisions (Kaiser beta ranges, the sinc's small-argument form, the special branches of Rcos and Rrcos, the bisection of
the stop-band estimate) are taken in the dtype of the evaluation."""
import functools

import numpy as np

KAISER, RCOS, ARKAISER, RRCOS = 0, 2, 6, 8
SHAPES = {"Kaiser": KAISER, "Rcos": RCOS, "Arkaiser": ARKAISER, "Rrcos": RRCOS}
UNSUPPORTED = {"Pm": 1, "Fexp": 3, "Fsech": 4, "Farcsech": 5, "Rkaiser": 7, "Hm3": 9, "Gmsktx": 10, "Gmskrx": 11,
               "Rfexp": 12, "Rfsech": 13, "Rfarcsech": 14}


class ConfigError(Exception):
    pass


def _pi(D):
    return D(np.pi)


@functools.lru_cache(maxsize=None)
def _lngamma_table(D):
    """ln Gamma(k + 1), k = 0 .. 63 (math/gamma.rs:7-22): recursion below 10, Stirling-type series above"""
    out = []
    for k in range(64):
        z = D(k + 1)
        logs = []
        while z < D(10) and len(logs) < 16:
            logs.append(np.log(z))
            z = z + D(1)
        g = D(0.5) * (np.log(D(2) * _pi(D)) - np.log(z))
        g = g + z * (np.log(z + D(1) / (D(12) * z - D(0.1) / z)) - D(1))
        for v in reversed(logs):
            g = g - v
        out.append(g)
    return np.array(out, D)


def bessel_i0(z, D):
    """math/bessel.rs:9-67, the log-domain series of 64 terms; z an array"""
    z = np.asarray(z, D)
    lg = _lngamma_table(D)
    out = np.ones(z.shape, D)
    small = (z != 0) & (z < D(1e-3))
    out[small] = D(1) / np.exp(lg[0])
    big = z >= D(1e-3)
    if big.any():
        lhz = np.log(D(0.5) * z[big])
        acc = np.zeros(lhz.shape, D)
        for k in range(64):
            acc = acc + np.exp(D(2) * D(k) * lhz - lg[k] - lg[k])
        out[big] = np.exp(D(0) + np.log(acc))
    return out


def sinc(x, D):
    """math/mod.rs:63-69"""
    x = np.asarray(x, D)
    pi = _pi(D)
    small = np.abs(x) < D(0.01)
    xs = np.where(small, D(1), x)
    a = np.cos(pi * x / D(2)) * np.cos(pi * x / D(4)) * np.cos(pi * x / D(8))
    b = np.sin(pi * xs) / (pi * xs)
    return np.where(small, a, b).astype(D)


def kaiser_beta(as_, D):
    """kaiser.rs:62-72"""
    a = abs(D(as_))
    if a > D(50):
        return D(0.1102) * (a - D(8.7))
    if a > D(21):
        return D(0.5842) * np.power(a - D(21), D(0.4)) + D(0.07886) * (a - D(21))
    return D(0)


def design_kaiser(n, fc, as_, mu, D):
    """kaiser.rs:16-51 with windows::kaiser (math/windows.rs:76-90)"""
    fc, as_, mu = D(fc), D(as_), D(mu)
    if mu <= D(-0.5) or mu > D(0.5):
        raise ConfigError("mu")
    if fc <= 0 or fc > D(0.5):
        raise ConfigError("fc")
    if n == 0:
        raise ConfigError("n")
    if as_ <= 0:
        raise ConfigError("as")
    beta = kaiser_beta(as_, D)
    i = np.arange(n).astype(D)
    t = i - (D(n) - D(1)) / D(2) + mu
    proto = sinc(D(2) * fc * t, D)
    tw = i - D(n - 1) / D(2)
    r = D(2) * tw / D(n - 1)
    win = bessel_i0(beta * np.sqrt(D(1) - r * r), D) / bessel_i0(np.array([beta], D), D)[0]
    return (proto * win).astype(D)


def filter_len_kaiser(df, as_, D):
    """design/mod.rs:228-238"""
    if df > D(0.5) or df <= 0:
        raise ConfigError("df")
    if as_ <= 0:
        raise ConfigError("as")
    return (as_ - D(7.95)) / (D(14.26) * df)


def estimate_stopband_attenuation(df, n, D):
    """design/mod.rs:161-184"""
    df = D(df)
    as0, as1, as_hat = D(0.01), D(200), D(0)
    for _ in range(20):
        as_hat = D(0.5) * (as1 + as0)
        if filter_len_kaiser(df, as_hat, D) < D(n):
            as0 = as_hat
        else:
            as1 = as_hat
    return as_hat


def _z(k, m, dt, D):
    n = np.arange(2 * k * m + 1).astype(D)
    return (n + D(dt)) / D(k) - D(m)


def design_rcos(k, m, beta, dt, D):
    """rcos.rs:17-51"""
    if k < 1 or m < 1 or beta < 0 or beta > 1:
        raise ConfigError("rcos")
    beta, pi = D(beta), _pi(D)
    z = _z(k, m, dt, D)
    t1 = np.cos(beta * pi * z)
    t2 = sinc(z, D)
    t3 = D(1) - D(4) * beta * beta * z * z
    special = np.abs(t3) < D(1e-3)
    with np.errstate(divide="ignore", invalid="ignore"):
        lim = np.sin(pi / (D(2) * beta)) * beta * D(0.5) if beta != 0 else D(0)
        return np.where(special, lim, t1 * t2 / np.where(special, D(1), t3)).astype(D)


def rcos_branch_distance(k, m, beta, dt):
    """f64: min over the taps of | |1 - 4 beta^2 z^2| - 1e-3 |, the compared quantity's distance from its threshold"""
    z = _z(k, m, dt, np.float64)
    b = np.float64(np.float32(beta))
    return np.min(np.abs(np.abs(1 - 4 * b * b * z * z) - 1e-3))


def design_rrcos(k, m, beta, dt, D):
    """rrcos.rs:15-63"""
    if k < 1 or m < 1 or beta < 0 or beta > 1:
        raise ConfigError("rrcos")
    beta, pi = D(beta), _pi(D)
    z = _z(k, m, dt, D)
    centre = np.abs(z) < D(1e-5)
    g = D(1) - D(16) * beta * beta * z * z
    g = g * g
    special = ~centre & (np.abs(g) < D(1e-5))
    zs = np.where(centre | special, D(1), z)       # keeps the general form finite where it is not taken
    h0 = D(1) - beta + D(4) * beta / pi
    g1, g2 = D(1) + D(2) / pi, np.sin(D(0.25) * pi / beta)
    g3, g4 = D(1) - D(2) / pi, np.cos(D(0.25) * pi / beta)
    h1 = beta / np.sqrt(D(2)) * (g1 * g2 + g3 * g4)
    t1 = np.cos((D(1) + beta) * pi * zs)
    t2 = np.sin((D(1) - beta) * pi * zs)
    t3 = D(1) / (D(4) * beta * zs)
    with np.errstate(divide="ignore", invalid="ignore"):
        t4 = D(4) * beta / (pi * (D(1) - (D(16) * beta * beta * zs * zs)))
        gen = t4 * (t1 + (t2 * t3))
    return np.where(centre, h0, np.where(special, h1, gen)).astype(D)


def rrcos_branch_distances(k, m, beta, dt):
    """f64, over the taps other than an exact z = 0: (min | |z| - 1e-5 |, min | |1 - 16 beta^2 z^2| - sqrt(1e-5) |), the
    distances of the two compared quantities from their thresholds (g = (1 - 16 beta^2 z^2)^2 < 1e-5)"""
    z = _z(k, m, dt, np.float64)
    z = z[z != 0]
    b = np.float64(np.float32(beta))
    return (np.min(np.abs(np.abs(z) - 1e-5)), np.min(np.abs(np.abs(1 - 16 * b * b * z * z) - np.sqrt(1e-5))))


def arkaiser_rho(m, beta, D):
    """rkaiser.rs:65-69, the closed form only"""
    mf, beta = D(m), D(beta)
    c0 = D(0.762886) + D(0.067663) * np.log(mf)
    c1 = D(0.065515)
    c2 = np.log(D(1) - D(0.088) * np.power(mf, D(-1.6)))
    lb = np.log(beta)
    return c0 + c1 * lb + c2 * lb * lb


def design_arkaiser(k, m, beta, dt, D):
    """rkaiser.rs:49-93; rho_hat outside (0, 1) is an error here (no fallback table)"""
    if k < 2 or m < 1 or beta <= 0 or beta >= 1 or dt < -1 or dt > 1:
        raise ConfigError("arkaiser")
    rho = arkaiser_rho(m, beta, D)
    if not (0 < rho < 1):
        raise ConfigError("rho")
    beta = D(beta)
    n = 2 * k * m + 1
    kf = D(k)
    delta = beta * rho / kf
    as_ = estimate_stopband_attenuation(delta, n, D)
    fc = D(0.5) * (D(1) + beta * (D(1) - rho)) / kf
    h = design_kaiser(n, fc, as_, dt, D)
    e2 = D(0)
    for v in h:                                     # the sequential f32 sum
        e2 = e2 + v * v
    return (h * np.sqrt(kf / e2)).astype(D)


def design_prototype(ftype, k, m, beta, dt, D):
    """design/mod.rs:392-451.  beta and dt are taken as the f32 values the C ABI receives."""
    beta, dt = D(np.float32(beta)), D(np.float32(dt))
    if k < 1 or m < 1:
        raise ConfigError("k, m")
    h_len = 2 * k * m + 1
    fc = D(0.5) / D(k)
    df = beta / D(k)
    as_ = estimate_stopband_attenuation(df, h_len, D)
    if ftype == KAISER:
        return design_kaiser(h_len, fc, as_, dt, D)
    if ftype == RCOS:
        return design_rcos(k, m, beta, dt, D)
    if ftype == RRCOS:
        return design_rrcos(k, m, beta, dt, D)
    if ftype == ARKAISER:
        return design_arkaiser(k, m, beta, dt, D)
    raise ConfigError("shape")
