"""tests/chanr_ref.py (the complex128 firpfbchr reference of the GPU tests) pinned without a GPU to

  * the relations that fix its conventions: at P = M/2 both directions equal FirPfbCh2Ref (and the oracle's FirPfbCh2),
    at P = M the synthesizer equals FirPfbChRef with p = 2m and FirPfbChRef's analyzer is M exp(+j 2 pi k / M) times this
    one (and the oracle's FirPfbCh),
  * a brute-force evaluation of the down-converter bank (analyzer) and of the up-converter bank (synthesizer), and
  * a sequential restatement of the analyzer with M windows and a commutator counting down, which equals the closed form
    times exp(-j 2 pi k P / M),

on blocks cut into 1, 2 and 3 calls whose cuts leave the step count off every multiple of Q = M / gcd(M, P).  Then the
designed prototypes: analyzer followed by synthesizer returns the input delayed by 2Mm - P + 1 samples, with the
reconstruction error measured in f64 (Kaiser, As = 60, 300 steps of noise) pinned to 1 dB.  Argument errors are
ConfigErrors decided before a device is needed."""
import math

import numpy as np
import pytest
import torch

from chan_ref import FirPfbCh2Ref, FirPfbChRef, FrameCheck
from chanr_ref import CHANR_FRAME_TAU, FirPfbChrRef
from gpu_util import SEED

TAU64 = 3e-12            # two complex128 evaluations of the same sums
TAU32 = 1e-6             # against the oracle, which computes in f32 (tests/test_chan_ref_cpu.py)

SHAPES = [(2, 1, 1), (6, 1, 2), (8, 3, 2), (10, 7, 3), (12, 9, 8), (16, 12, 4), (22, 6, 2), (64, 48, 8), (100, 75, 5),
          (256, 192, 4)]


def _proto(oracle, M, m, fc):
    h = oracle.fir_design_kaiser(2 * M * m + 1, fc, 60.0).astype(np.float64)     # the last tap must be ignored
    return h * M / h.sum()


def _nsteps(M, P, m):
    return -(-2 * M * m // P) + 2 * (M // math.gcd(M, P)) + 5


def _cuts(n, ncalls, Q):
    """call boundaries; every inner one is moved off the multiples of Q"""
    inner = [n // 3 + 1, (2 * n) // 3 + 2][: ncalls - 1]
    inner = [c + 1 if Q > 1 and c % Q == 0 else c for c in inner]
    assert all(0 < c < n and (Q == 1 or c % Q) for c in inner)
    c = [0] + inner + [n]
    return list(zip(c, c[1:]))


def _run(fn, x, unit, n, ncalls, Q, chunk):
    x = torch.from_numpy(np.ascontiguousarray(x))
    return torch.cat([fn(x[a * unit: b * unit], chunk=chunk) for a, b in _cuts(n, ncalls, Q)])


def _close(got, want, tau, what=""):
    want = torch.as_tensor(np.ascontiguousarray(want)) if not torch.is_tensor(want) else want
    want = want.reshape(got.shape[0], -1)
    fc = FrameCheck(got.shape[0])
    fc.add(0, got, want)
    worst, f, rel = fc.worst()
    assert worst <= tau, f"{what}: worst step {f}: ratio {worst:.3e} (rel L2 {rel:.3e})"


def _brute_analyzer(h, x, M, P, m, ns):
    """y_s[k] = (1/M) sum_l h[l] x[(s+1)P - 1 - l] exp(+j 2 pi k (l - sP) / M): M down-converters"""
    L = 2 * M * m
    k = np.arange(M)[:, None]
    l = np.arange(L)[None, :]
    y = np.zeros((ns, M), np.complex128)
    for s in range(ns):
        t = (s + 1) * P - 1 - l
        xs = np.where(t >= 0, x[np.maximum(t, 0)], 0)
        y[s] = (np.exp(2j * np.pi * ((k * (l - s * P)) % M) / M) * (h[:L] * xs)).sum(axis=1) / M
    return y


def _brute_synthesizer(h, X, M, P, m, ns):
    """y[t] = (P/M) sum_k exp(+j 2 pi k t / M) sum_s h[t - sP] X_s[k]: every channel upsampled by P, filtered, mixed up"""
    L = 2 * M * m
    k = np.arange(M)
    y = np.zeros(ns * P, np.complex128)
    for t in range(ns * P):
        s = np.arange(max(0, -(-(t - L + 1) // P)), t // P + 1)
        f = h[t - s * P] @ X[s]                                       # [M]: the filtered channels at time t
        y[t] = (np.exp(2j * np.pi * ((k * t) % M) / M) * f).sum() * P / M
    return y.reshape(ns, P)


def _sequential_analyzer(h, x, M, P, m, ns):
    """M windows of 2m samples, a commutator counting down from M - 1; after a step's P pushes branch i reads window
    (base_index + i + 1) mod M and its dot product goes to that window's slot of the transform; IDFT divided by M"""
    win = [[0j] * (2 * m) for _ in range(M)]                          # newest first
    base = M - 1
    y = np.zeros((ns, M), np.complex128)
    for s in range(ns):
        for v in x[s * P: (s + 1) * P]:
            win[base] = [complex(v)] + win[base][:-1]
            base = M - 1 if base == 0 else base - 1
        X = np.zeros(M, np.complex128)
        for i in range(M):
            off = (base + i + 1) % M
            X[off] = sum(h[i + n * M] * win[off][n] for n in range(2 * m))
        y[s] = np.fft.ifft(X)
    return y


@pytest.mark.parametrize("M,P,m", SHAPES)
@pytest.mark.parametrize("ncalls", [1, 2, 3])
def test_analyzer_ref_vs_brute_force_and_commutator(oracle, M, P, m, ncalls):
    Q = M // math.gcd(M, P)
    ns = _nsteps(M, P, m)
    h = _proto(oracle, M, m, 0.5 / P)
    x = oracle.gen_complex(SEED + 60 + M + P, ns * P).astype(np.complex128)
    ref = FirPfbChrRef(M, P, m, h)
    got = _run(ref.analyzer_execute, x, P, ns, ncalls, Q, chunk=3 * 2 * M * m)
    assert got.shape == (ns, M)
    _close(got, _brute_analyzer(h, x, M, P, m, ns), TAU64, "down-converter bank")
    if ncalls == 1:
        seq = _sequential_analyzer(h, x, M, P, m, ns) * np.exp(2j * np.pi * np.arange(M) * P / M)
        _close(got, seq, TAU64, "commutator")


@pytest.mark.parametrize("M,P,m", SHAPES)
@pytest.mark.parametrize("ncalls", [1, 2, 3])
def test_synthesizer_ref_vs_brute_force(oracle, M, P, m, ncalls):
    Q = M // math.gcd(M, P)
    ns = _nsteps(M, P, m)
    h = _proto(oracle, M, m, 0.5 / M)
    X = oracle.gen_complex(SEED + 61 + M + P, ns * M).astype(np.complex128)
    ref = FirPfbChrRef(M, P, m, h)
    got = _run(ref.synthesizer_execute, X, M, ns, ncalls, Q, chunk=3 * M)
    assert got.shape == (ns, P)
    _close(got, _brute_synthesizer(h, X.reshape(ns, M), M, P, m, ns), TAU64, "up-converter bank")


@pytest.mark.parametrize("M,m", [(2, 1), (6, 2), (16, 4), (64, 4), (100, 3)])
@pytest.mark.parametrize("ncalls", [1, 2, 3])
def test_half_rate_equals_firpfbch2(oracle, M, m, ncalls):
    P = M // 2
    ns = 8 * m + 13                                                   # odd, as in tests/test_chan_ref_cpu.py
    ha = _proto(oracle, M, m, 1.0 / M).astype(np.float32)
    hs = _proto(oracle, M, m, 0.5 / M).astype(np.float32)
    x = oracle.gen_complex(SEED + 62 + M, ns * P)
    X = oracle.gen_complex(SEED + 63 + M, ns * M)
    got = _run(FirPfbChrRef(M, P, m, ha).analyzer_execute, x, P, ns, ncalls, 2, chunk=5 * 2 * M * m)
    _close(got, FirPfbCh2Ref(M, m, ha).analyzer_execute(torch.from_numpy(x)), TAU64, "FirPfbCh2Ref analyzer")
    _close(got, oracle.FirPfbCh2(M, m, ha).analyzer_execute(x), TAU32, "oracle FirPfbCh2 analyzer")
    got = _run(FirPfbChrRef(M, P, m, hs).synthesizer_execute, X, M, ns, ncalls, 2, chunk=3 * M)
    _close(got, FirPfbCh2Ref(M, m, hs).synthesizer_execute(torch.from_numpy(X)), TAU64, "FirPfbCh2Ref synthesizer")
    _close(got, oracle.FirPfbCh2(M, m, hs).synthesizer_execute(X), TAU32, "oracle FirPfbCh2 synthesizer")


@pytest.mark.parametrize("M,m", [(2, 1), (6, 2), (16, 8), (64, 3), (100, 2)])
@pytest.mark.parametrize("ncalls", [1, 3])
def test_full_rate_equals_firpfbch(oracle, M, m, ncalls):
    P, p = M, 2 * m
    ns = 3 * p + 11
    h = oracle.fir_design_kaiser(M * p + 1, 0.5 / M, 60.0)
    x = oracle.gen_complex(SEED + 64 + M, ns * M)
    X = oracle.gen_complex(SEED + 65 + M, ns * M)
    got = _run(FirPfbChrRef(M, P, m, h).synthesizer_execute, X, M, ns, ncalls, 1, chunk=3 * M)
    _close(got, FirPfbChRef(M, p, h).synthesizer_execute(torch.from_numpy(X)), TAU64, "FirPfbChRef synthesizer")
    _close(got, oracle.FirPfbCh(M, p, h).synthesizer_execute(X), TAU32, "oracle FirPfbCh synthesizer")
    got = _run(FirPfbChrRef(M, P, m, h).analyzer_execute, x, P, ns, ncalls, 1, chunk=5 * M * p)
    got = got * (M * torch.exp(2j * math.pi * torch.arange(M, dtype=torch.float64) / M))
    _close(got, FirPfbChRef(M, p, h).analyzer_execute(torch.from_numpy(x)), TAU64, "FirPfbChRef analyzer")
    _close(got, oracle.FirPfbCh(M, p, h).analyzer_execute(x), TAU32, "oracle FirPfbCh analyzer")


def reconstruction_db(x, y, delay):
    """error of y against x delayed by `delay`, over the samples both cover, in dB"""
    x, y = np.asarray(x, np.complex128).reshape(-1), np.asarray(y, np.complex128).reshape(-1)
    e = y[delay:] - x[: x.size - delay]
    return 10 * math.log10(np.sum(np.abs(e) ** 2) / np.sum(np.abs(x[: x.size - delay]) ** 2))


# (M, P, m) -> reconstruction error in dB measured in f64 (As = 60, 300 steps of noise); the margin of 1 dB is for the
# noise realisation.  (16, 12, 4): the transition band is too wide for m = 4; (16, 16, 8): critical sampling, no guard band
RECONSTRUCTION = [((16, 12, 8), -63.2), ((64, 48, 8), -62.9), ((12, 9, 8), -63.4), ((16, 8, 4), -62.2),
                  ((16, 12, 4), -31.9), ((16, 16, 8), -15.1)]


@pytest.mark.parametrize("shape,db", RECONSTRUCTION, ids=[str(s) for s, _ in RECONSTRUCTION])
def test_designed_prototypes_reconstruct_with_the_stated_delay(oracle, shape, db):
    M, P, m = shape
    ns = 300
    ha, hs = _proto(oracle, M, m, 0.5 / P), _proto(oracle, M, m, 0.5 / M)
    x = oracle.gen_complex(SEED + 66 + M + P, ns * P).astype(np.complex128)
    Y = FirPfbChrRef(M, P, m, ha).analyzer_execute(torch.from_numpy(x))
    y = FirPfbChrRef(M, P, m, hs).synthesizer_execute(Y).reshape(-1).numpy()
    delay = 2 * M * m - P + 1
    n = x.size
    corr = np.fft.ifft(np.fft.fft(y, 2 * n) * np.conj(np.fft.fft(x, 2 * n)))[:n]     # corr[d] = sum_t y[t + d] conj(x[t])
    assert int(np.argmax(np.abs(corr))) == delay
    got = reconstruction_db(x, y, delay)
    print(f"firpfbchr {shape}: reconstruction {got:.2f} dB at delay {delay}")
    assert abs(got - db) <= 1.0, (shape, got, db)


def test_step_check_catches_one_step_off_by_one_percent(oracle):
    M, P, m = 64, 48, 8
    ns = 2048
    h = _proto(oracle, M, m, 0.5 / P)
    x = torch.from_numpy(oracle.gen_complex(SEED + 67, ns * P))
    want = FirPfbChrRef(M, P, m, h).analyzer_execute(x)
    bad = want.clone()
    bad[777] *= 1.01
    fc = FrameCheck(ns)
    fc.add(0, want, bad)
    worst, f, _ = fc.worst()
    assert f == 777 and worst > 100 * CHANR_FRAME_TAU


BAD_ARGS = [(1, 1, 1), (0, 1, 1), (4, 0, 1), (4, 5, 1), (4, 2, 0), (8194, 2, 1), (4, 2, 2049),
            (8192, 4096, 1)]           # M*m beyond the LDS of the general kernels


@pytest.mark.parametrize("M,P,m", BAD_ARGS)
def test_argument_errors_are_config_errors_without_a_device(M, P, m):
    import yagi_amd as ya
    h = np.ones(max(1, 2 * M * m), np.float32)
    with pytest.raises(ya.ConfigError):
        ya.FirPfbChr(M, P, m, h)
    with pytest.raises(ya.ConfigError):
        ya.FirPfbChr.new_kaiser(M, P, m, 60.0)
    with pytest.raises(ya.ConfigError):
        ya.FirPfbChr.new_kaiser_synthesizer(M, P, m, 60.0)
