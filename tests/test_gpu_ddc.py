"""Ddc and Duc: the oscillator mix fused into the FIR decimator and interpolator (ddc_kernels.hip).

The reference's src/filter/dds.rs is empty, so the objects are defined as compositions of two objects of this library
that are pinned to the reference elsewhere (tests/test_gpu_osc.py, tests/test_gpu_fir.py, tests/test_gpu_firinterp.py):

    Ddc = Osc.mix_block_down, then FirDecimationFilter.execute_block
    Duc = FirInterpolationFilter.execute_block, then Osc.mix_block_up

and the parity bar is np.array_equal on the raw words against that composition, run through an intermediate buffer with
the same taps, scale, frequency, phase and call lengths.  A second, independent check goes through tests/osc_ref.py and
the oracle's f64 FIR sum under the a-priori bound of tests/gpu_util.py."""
import ctypes

import numpy as np
import pytest

import osc_ref
from gpu_util import fir_bound, rand_samples, rand_taps

pytestmark = pytest.mark.gpu

KINDS = ["crcf", "cccf"]
SCHEMES = [0, 1]                                   # OscScheme.Nco, OscScheme.Vco
CUTS = np.cumsum([0, 4096, 2048, 513, 700, 512, 2049, 100])       # test_firdecim_register_window_kernel's
DUC_CUTS = np.cumsum([0, 1, 511, 512, 513, 2049, 100])
FREQS = ["ordinary", "odd word above 2^31", "zero"]
# a fused kernel serves none of these: M = 1 (no decimation), and 4096 taps at M = 64, whose phase-split span does not
# fit the LDS at any tile, so launch_fir_block streams it through fir_block_kernel<K, false>
UNSERVED = [(1, 33), (64, 4096)]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def words(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def same_words(a, b):
    return np.array_equal(words(a), words(b))


def tune(o, freq):
    """the same calls on a Ddc / Duc and on an Osc: the same constrain() makes the same words.  The phase word starts
    about 56000 below 2^32, so with a frequency it wraps within the first steps of the first call"""
    o.set_phase(6.2831)
    o.adjust_phase(3.0e-6)
    if freq == "ordinary":
        o.set_frequency(0.3713)
    elif freq == "odd word above 2^31":
        o.set_frequency(4.0)                       # above pi: the word is above 2^31, a multiple of 256 in f32
        o.adjust_frequency(1.0e-5)                 # a small word, exact in f32: makes the sum odd
    else:
        o.set_frequency(0.0)


def check_tuning(o, freq):
    theta, d = o.get_state()
    assert 0 < (1 << 32) - theta < 1 << 16, hex(theta)
    if freq == "odd word above 2^31":
        assert d > 1 << 31 and d & 1, hex(d)
    if freq == "zero":
        assert d == 0
    elif d:
        assert ((1 << 32) - theta) // d < 1000     # the phase wraps within 1000 steps


class DdcParts:
    """the composition: separate Osc and FirDecimationFilter through an intermediate buffer"""

    def __init__(self, ya, kind, scheme, M, h, scale):
        self.osc, self.fir, self.M = ya.Osc(scheme), ya.FirDecimationFilter(kind, M, h), M
        self.fir.set_scale(scale)

    def execute_block(self, x, n):
        mixed = self.osc.mix_block_down(x[:n * self.M])
        return self.fir.execute_block(mixed, n)


class DucParts:
    def __init__(self, ya, kind, scheme, interp, h, scale):
        self.osc, self.fir = ya.Osc(scheme), ya.FirInterpolationFilter(kind, interp, h)
        self.fir.set_scale(scale)

    def execute_block(self, x):
        return self.osc.mix_block_up(self.fir.execute_block(x))


def scale_of(kind):
    return 0.5 if kind == "crcf" else 0.5 - 0.25j


# ---- 1. Ddc: fused equals composition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES, ids=["nco", "vco"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,L", [(2, 65), (8, 129), (8, 257), (3, 64), (12, 200), (16, 33), (5, 7), (9, 300), (12, 400),
                                 (16, 513)])
def test_ddc_fused_equals_composition(ya, kind, scheme, M, L):
    """set_kernel(2), every call ran the fused kernel, every output word equals Osc + FirDecimationFilter.  Both paths
    see the same cuts, so launch_fir_block and the fused dispatch pick the same kernel per call, and every call after
    the first starts on a window of mixed samples.  With complex samples (8 bytes, fir_block_plan) the shapes reach:
      (2, 65)    32 taps per phase: fir_decim_consec<256, 8>, power-of-two descriptor staging in the interior tiles
      (8, 129)   16 per phase: <128, 4> (<256, 4> does not fit the 48 KiB span budget), power-of-two staging
      (8, 257)   32 per phase: <256, 8> and <256, 4> do not fit, <128, 4> does; power-of-two staging
      (3, 64)    21 per phase: <256, 4>, the any-M descriptor staging
      (9, 300)   33 per phase: <64, 8>, any-M staging;  (12, 400): <64, 4>, any-M;  (16, 513): <64, 4>, power of two
      (12, 200)  16 per phase, but neither <256, 4> nor <128, 4> fits: the general staged kernel
      (16, 33), (5, 7)     fewer than 8 taps per phase: the general staged kernel fir_block_kernel<K, true>
    so all five register-window instantiations and the general kernel run fused.  In every shape the first tile of a
    call (it reaches into the carried window) and the last (it ends with the block) take the guarded staging; the
    100-output call is below the 512-output threshold of the register-window kernels (general staged kernel), the
    513-output call just above it."""
    rng = np.random.default_rng(4100 + 37 * M + L)
    n = int(CUTS[-1])
    h, x = rand_taps(rng, kind, L), rand_samples(rng, "crcf", n * M)
    for freq in FREQS:
        q, ref = ya.Ddc(kind, scheme, M, h), DdcParts(ya, kind, scheme, M, h, scale_of(kind))
        q.set_scale(scale_of(kind))
        q.set_kernel(2)
        tune(q, freq)
        tune(ref.osc, freq)
        check_tuning(q, freq)
        for i, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
            if i == 3:
                q.adjust_frequency(0.01)
                ref.osc.adjust_frequency(0.01)
            got = q.execute_block(x[a * M:b * M], int(b - a))
            assert q.get_last_kernel() == 2, (freq, i)
            want = ref.execute_block(x[a * M:b * M], int(b - a))
            assert same_words(got, want), (freq, i, int(np.flatnonzero(words(got) != words(want))[0]))
            assert q.get_state() == ref.osc.get_state(), (freq, i)


# ---- 2. Duc: fused equals composition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES, ids=["nco", "vco"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("interp,hl", [(2, 9), (4, 65), (5, 101), (8, 257), (16, 33), (20, 100), (32, 12800)])
def test_duc_fused_equals_composition(ya, kind, scheme, interp, hl):
    """launch_firpfb_all picks firpfb_fewbranch_kernel for up to 16 branches whose 256-sample span fits the LDS: the
    five shapes of the issue, (2, 9) .. (16, 33), all reach it ((2, 9), (4, 65), (5, 101), (8, 257) and (16, 33) are no
    multiples of the rate, so their banks are zero-padded; 5 branches also run the loop over the last nf % 4).  Above
    16 branches it picks firpfb_all_kernel: (20, 100) with the transposed taps in LDS (TAPS_LDS), (32, 12800) with 400
    taps per branch, 51200 bytes (crcf) of taps that do not fit beside the span, so they stay in global memory."""
    rng = np.random.default_rng(4200 + 37 * interp + hl)
    n = int(DUC_CUTS[-1])
    h, x = rand_taps(rng, kind, hl), rand_samples(rng, "crcf", n)
    for freq in FREQS:
        q, ref = ya.Duc(kind, scheme, interp, h), DucParts(ya, kind, scheme, interp, h, scale_of(kind))
        q.set_scale(scale_of(kind))
        q.set_kernel(2)
        tune(q, freq)
        tune(ref.osc, freq)
        check_tuning(q, freq)
        for i, (a, b) in enumerate(zip(DUC_CUTS[:-1], DUC_CUTS[1:])):
            if i == 3:
                q.adjust_frequency(0.01)
                ref.osc.adjust_frequency(0.01)
            got = q.execute_block(x[a:b])
            assert q.get_last_kernel() == 2, (freq, i)
            want = ref.execute_block(x[a:b])
            assert same_words(got, want), (freq, i, int(np.flatnonzero(words(got) != words(want))[0]))
            assert q.get_state() == ref.osc.get_state(), (freq, i)


# ---- 3. the two-launch route -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES, ids=["nco", "vco"])
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_choices_give_the_same_words(ya, kind, scheme):
    """on a served shape choices 0 and 2 run the fused kernel and 1 the two launches; on shapes no fused kernel serves
    every choice runs two launches; the words are the composition's every time"""
    rng = np.random.default_rng(4300)
    cuts = CUTS[:4]
    for M, L, served in [(8, 129, True)] + [(m, l, False) for m, l in UNSERVED]:
        n = int(cuts[-1])
        h, x = rand_taps(rng, kind, L), rand_samples(rng, "crcf", n * M)
        ref = DdcParts(ya, kind, scheme, M, h, scale_of(kind))
        tune(ref.osc, "ordinary")
        want = [ref.execute_block(x[a * M:b * M], int(b - a)) for a, b in zip(cuts[:-1], cuts[1:])]
        for choice in (0, 1, 2):
            q = ya.Ddc(kind, scheme, M, h)
            q.set_scale(scale_of(kind))
            q.set_kernel(choice)
            tune(q, "ordinary")
            for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                got = q.execute_block(x[a * M:b * M], int(b - a))
                assert q.get_last_kernel() == (2 if served and choice != 1 else 1), (M, L, choice, i)
                assert same_words(got, want[i]), (M, L, choice, i)
            assert q.get_state() == ref.osc.get_state()
    # Duc: every shape launch_firpfb_all accepts is served; choice 1 is the two launches
    interp, hl = 5, 101
    h, x = rand_taps(rng, kind, hl), rand_samples(rng, "crcf", 1200)
    ref = DucParts(ya, kind, scheme, interp, h, scale_of(kind))
    tune(ref.osc, "ordinary")
    want = [ref.execute_block(x[:700]), ref.execute_block(x[700:])]
    for choice in (0, 1, 2):
        q = ya.Duc(kind, scheme, interp, h)
        q.set_scale(scale_of(kind))
        q.set_kernel(choice)
        tune(q, "ordinary")
        for i, part in enumerate((x[:700], x[700:])):
            got = q.execute_block(part)
            assert q.get_last_kernel() == (1 if choice == 1 else 2)
            assert same_words(got, want[i]), (choice, i)


# ---- 4. independent of the library's own parts --------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES, ids=["nco", "vco"])
def test_ddc_against_oscref_and_f64(ya, oracle, scheme):
    """mixed samples from OscRef (exact f32), the FIR sum from the oracle in f64, the bound of
    test_firdecim_random_vs_f64"""
    rng = np.random.default_rng(4400 + scheme)
    kind, M, L, n = "crcf", 8, 129, 3000
    h, x = rand_taps(rng, kind, L), rand_samples(rng, kind, n * M)
    q, o = ya.Ddc(kind, scheme, M, h), osc_ref.OscRef(scheme)
    q.set_scale(0.5)
    tune(q, "ordinary")
    tune(o, "ordinary")
    assert q.get_state() == (o.theta, o.d_theta)
    k = 1700
    got = np.concatenate([q.execute_block(x[:k * M], k), q.execute_block(x[k * M:], n - k)])
    assert q.get_last_kernel() == 2
    mixed = o.mix_block(x, True)
    truth = oracle.fir_block_f64(kind, h, mixed, M=M, n=n, scale=0.5)
    err, bound = float(np.max(np.abs(got - truth))), fir_bound(kind, h, mixed)
    print(f"Ddc scheme {scheme}: max |err| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert q.get_state() == (o.theta, o.d_theta)


@pytest.mark.parametrize("scheme", SCHEMES, ids=["nco", "vco"])
def test_duc_against_f64_and_oscref(ya, oracle, scheme):
    """the f64 interpolation (the FIR sum over the zero-stuffed input) rounded to f32 and mixed up by OscRef; the same
    bound, scaled by max |table| = 1"""
    rng = np.random.default_rng(4450 + scheme)
    kind, interp, hl, n = "crcf", 5, 101, 1500
    h, x = rand_taps(rng, kind, hl), rand_samples(rng, kind, n)
    q, o = ya.Duc(kind, scheme, interp, h), osc_ref.OscRef(scheme)
    q.set_scale(0.5)
    tune(q, "ordinary")
    tune(o, "ordinary")
    got = np.concatenate([q.execute_block(x[:700]), q.execute_block(x[700:])])
    assert q.get_last_kernel() == 2
    up = np.zeros(n * interp, np.complex64)
    up[::interp] = x
    y64 = oracle.fir_block_f64(kind, h, up, scale=0.5)
    truth = o.mix_block(y64.astype(np.complex64), False)
    err, bound = float(np.max(np.abs(got - truth))), fir_bound(kind, h, x)
    print(f"Duc scheme {scheme}: max |err| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert q.get_state() == (o.theta, o.d_theta)


# ---- 5. state -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES, ids=["nco", "vco"])
@pytest.mark.parametrize("kind", KINDS)
def test_clone_and_reset(ya, kind, scheme):
    rng = np.random.default_rng(4500)
    M, L, n = 8, 129, 1500
    h, x = rand_taps(rng, kind, L), rand_samples(rng, "crcf", 2 * n * M)
    q = ya.Ddc(kind, scheme, M, h)
    q.set_scale(scale_of(kind))
    tune(q, "ordinary")
    q.execute_block(x[:n * M], n)
    c = q.clone()
    assert c.get_state() == q.get_state() and c.get_scale() == q.get_scale() and c.get_decim_rate() == M
    assert same_words(q.execute_block(x[n * M:], n), c.execute_block(x[n * M:], n))
    # reset clears the window and keeps the phase: the next block is a fresh object's at the same words
    words_before = q.get_state()
    q.reset()
    assert q.get_state() == words_before
    f = ya.Ddc(kind, scheme, M, h)
    f.set_scale(scale_of(kind))
    f.set_state(*words_before)
    assert same_words(q.execute_block(x[:n * M], n), f.execute_block(x[:n * M], n))

    interp, hl = 5, 101
    hi = rand_taps(rng, kind, hl)
    u = ya.Duc(kind, scheme, interp, hi)
    u.set_scale(scale_of(kind))
    tune(u, "ordinary")
    u.execute_block(x[:700])
    cu = u.clone()
    assert cu.get_state() == u.get_state() and cu.get_interp_rate() == interp
    assert same_words(u.execute_block(x[700:1500]), cu.execute_block(x[700:1500]))
    words_before = u.get_state()
    u.reset()
    assert u.get_state() == words_before
    fu = ya.Duc(kind, scheme, interp, hi)
    fu.set_scale(scale_of(kind))
    fu.set_state(*words_before)
    assert same_words(u.execute_block(x[:700]), fu.execute_block(x[:700]))


@pytest.mark.parametrize("scheme", SCHEMES, ids=["nco", "vco"])
@pytest.mark.parametrize("kind", KINDS)
def test_per_sample_calls_interleave_with_block_calls(ya, kind, scheme):
    """execute() runs on the host mirror with Osc's per-sample mix and the parts' sequential, unfused sums, the block
    calls on the device with fused multiply-adds: equal to 1e-5, the tolerance between the two forms in
    test_per_sample_firpfb_and_firdecim_on_the_host_mirror; the phase word is exact"""
    rng = np.random.default_rng(4600)
    M, L = 4, 23
    h, x = rand_taps(rng, kind, L), rand_samples(rng, "crcf", 700 * M)
    whole, q = ya.Ddc(kind, scheme, M, h), ya.Ddc(kind, scheme, M, h)
    for o in (whole, q):
        tune(o, "ordinary")
    want = whole.execute_block(x, 700)
    got = [q.execute_block(x[:300 * M], 300)]
    got.append(np.array([q.execute(x[k * M:(k + 1) * M]) for k in range(300, 340)], np.complex64))
    got.append(q.execute_block(x[340 * M:690 * M], 350))
    got.append(np.array([q.execute(x[k * M:(k + 1) * M]) for k in range(690, 700)], np.complex64))
    assert np.max(np.abs(np.concatenate(got) - want)) <= 1e-5
    assert q.get_state() == whole.get_state()
    with pytest.raises(ya.ConfigError):
        q.execute(x[:M - 1])

    interp, hl = 4, 37
    hi = rand_taps(rng, kind, hl)
    whole, u = ya.Duc(kind, scheme, interp, hi), ya.Duc(kind, scheme, interp, hi)
    for o in (whole, u):
        tune(o, "ordinary")
    want = whole.execute_block(x[:700])
    got = [u.execute_block(x[:300])]
    got.append(np.concatenate([u.execute(x[k]) for k in range(300, 340)]))
    got.append(u.execute_block(x[340:690]))
    got.append(np.concatenate([u.execute(x[k]) for k in range(690, 700)]))
    assert np.max(np.abs(np.concatenate(got) - want)) <= 1e-5
    assert u.get_state() == whole.get_state()


# ---- 6. edges and non-finite input -------------------------------------------------------------------------------------
def test_edges_and_config_errors(ya):
    h = np.ones(16, np.float32)
    q, u = ya.Ddc("crcf", 0, 4, h), ya.Duc("crcf", 1, 4, h)
    for o in (q, u):
        tune(o, "ordinary")
    before = q.get_state(), u.get_state()
    assert q.execute_block(np.zeros(0, np.complex64), 0).size == 0 and u.execute_block(np.zeros(0, np.complex64)).size == 0
    buf = ya.DeviceArray(64, np.complex64)
    q.execute_block_devptr(buf, 0, buf)               # n = 0 returns before the overlap check
    u.execute_block_devptr(buf, 0, buf)
    assert (q.get_state(), u.get_state()) == before and q.get_last_kernel() == 0 and u.get_last_kernel() == 0
    with pytest.raises(ya.ConfigError, match="overlap"):
        q.execute_block_devptr(buf, 4, buf.ptr + 8)
    with pytest.raises(ya.ConfigError, match="overlap"):
        u.execute_block_devptr(buf, 4, buf.ptr + 8)
    for cls in (ya.Ddc, ya.Duc):
        with pytest.raises(ya.ConfigError):
            cls("rrrf", 0, 4, h)                   # real samples cannot be mixed
        with pytest.raises(ValueError):
            cls("crcf", 2, 4, h)                   # no such OscScheme
        with pytest.raises(ya.ConfigError, match="unknown scheme"):
            hd = ctypes.c_void_p()
            ya._check(getattr(ya.lib, f"yagi_hip_{cls._obj}_crcf_create")(7, 4, h.ctypes.data, h.size, ctypes.byref(hd)))
        with pytest.raises(ya.ConfigError, match="filter length"):
            cls("crcf", 0, 4, np.zeros(0, np.float32))
        with pytest.raises(ya.ConfigError, match="greater than 1"):
            cls.new_kaiser("crcf", 0, 1, 4, 60.0)
        with pytest.raises(ya.ConfigError, match="filter delay"):
            cls.new_kaiser("crcf", 0, 4, 0, 60.0)
    with pytest.raises(ya.ConfigError, match="decimation factor"):
        ya.Ddc("crcf", 0, 0, h)
    with pytest.raises(ya.ConfigError, match="interp factor"):
        ya.Duc("crcf", 0, 1, h)
    with pytest.raises(ya.ConfigError, match="kernel choice"):
        q.set_kernel(3)
    with pytest.raises(ya.ConfigError):
        q.set_frequency(float("inf"))
    # the Kaiser prototypes are the parts' own
    k, kp = ya.Ddc.new_kaiser("crcf", 0, 4, 5, 60.0), ya.FirDecimationFilter.new_kaiser("crcf", 4, 5, 60.0)
    x = rand_samples(np.random.default_rng(1), "crcf", 4000)
    assert same_words(k.execute_block(x, 1000), kp.execute_block(x, 1000))         # frequency and phase 0: the mix is x
    k, kp = ya.Duc.new_kaiser("crcf", 0, 4, 5, 60.0), ya.FirInterpolationFilter.new_kaiser("crcf", 4, 5, 60.0)
    assert same_words(k.execute_block(x[:1000]), kp.execute_block(x[:1000]))


def nan_at(y):
    return np.flatnonzero(np.isnan(y.real) | np.isnan(y.imag))


@pytest.mark.parametrize("scheme", SCHEMES, ids=["nco", "vco"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_nan_poisons_the_window_that_holds_it(ya, kind, scheme):
    """DESIGN.md's non-finite table: Ddc -- the decimator's outputs o with M o - (L-1) <= s <= M o (the mixed NaN is a
    NaN in both parts whatever the table entry); Duc -- ceil(h_len / I) inputs, every branch.  The other outputs are the
    clean run's bit for bit.  The NaN sits in the second call for half of the cases, so it crosses the carried window."""
    rng = np.random.default_rng(4700)
    M, L, n1, n2 = 8, 129, 1300, 700
    h, x = rand_taps(rng, kind, L), rand_samples(rng, "crcf", (n1 + n2) * M)

    def run(v):
        q = ya.Ddc(kind, scheme, M, h)
        tune(q, "ordinary")
        return np.concatenate([q.execute_block(v[:n1 * M], n1), q.execute_block(v[n1 * M:], n2)])
    clean = run(x)
    assert nan_at(clean).size == 0
    o = np.arange(n1 + n2)
    for s in (5, 600 * M + 3, n1 * M - 2, n1 * M, (n1 + 300) * M + 7):
        xn = x.copy()
        xn[s] = complex(np.nan, 1.0)
        got = run(xn)
        want = np.flatnonzero((M * o >= s) & (M * o - (L - 1) <= s))
        assert np.array_equal(nan_at(got), want), s
        keep = np.setdiff1d(o, want)
        assert same_words(got[keep], clean[keep]), s

    interp, hl, m1, m2 = 5, 37, 700, 300
    hi, xi = rand_taps(rng, kind, hl), x[:m1 + m2]
    Ls = -(-hl // interp)

    def run_up(v):
        q = ya.Duc(kind, scheme, interp, hi)
        tune(q, "ordinary")
        return np.concatenate([q.execute_block(v[:m1]), q.execute_block(v[m1:])])
    clean = run_up(xi)
    j = np.arange((m1 + m2) * interp)
    for s in (0, 255, 256, m1 - 3, m1, m1 + 100):
        xn = xi.copy()
        xn[s] = complex(1.0, np.nan)
        got = run_up(xn)
        want = np.flatnonzero((j // interp >= s) & (j // interp < s + Ls))
        assert np.array_equal(nan_at(got), want), s
        keep = np.setdiff1d(j, want)
        assert same_words(got[keep], clean[keep]), s
