"""IirDecimationFilter, IirInterpolationFilter and IirHilbertFilter through the C ABI (src/filter/iir/iirdecim.rs,
iirinterp.rs, iirhilb.rs) and the mapped chunk kernels of iir_kernels.hip.

Each wrapper is IirFilter's recurrence over a virtual stream, so for the same coefficients and the
same cuts of the stream into calls the fused output equals, word for word, IirFilter.execute_block_dev over the
explicitly built stream mapped on the host: chunks, start states and operation order are identical, and any difference
is a wrong index map, a skipped zero step or a misplaced sign.  Integer data with poles on the unit circle and
single-chunk float blocks are compared with the line-by-line restatements of iirmap_ref (two real filters for Hilbert).
Shapes are given in filter steps N; with one section a chunk is 64 steps and a workgroup covers 4096."""
import numpy as np
import pytest

from gpu_util import rand_samples
from iir_ref import iir64
from iirmap_ref import (IirDecimRef, IirHilbRef, IirInterpRef, hilb_input, hilb_output, zero_stuff)
from psd_util import validate_psd_signal

pytestmark = pytest.mark.gpu
KINDS = ["rrrf", "crcf", "cccf"]
DT = {"rrrf": np.float32, "crcf": np.complex64, "cccf": np.complex64}
CDT = {"rrrf": np.float32, "crcf": np.float32, "cccf": np.complex64}
# the host / device switch, one chunk, one workgroup, several aggregates, G - 1 > 64 (phase B: two per lane, partial)
STEPS = [1, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5, 65 * 4096 + 7]
SHORT = [1, 33, 65, 4097, 3 * 4096 + 5]
RATES = [2, 3, 5, 17]
HMODES = ["r2c", "c2r", "decim", "interp"]
H_IN = {"r2c": ("rrrf", 1), "c2r": ("crcf", 1), "decim": ("rrrf", 2), "interp": ("crcf", 1)}     # kind, inputs per unit
H_OUT = {"r2c": (np.complex64, 1), "c2r": (np.float32, 1), "decim": (np.complex64, 1), "interp": (np.float32, 2)}
H_STEPS = {"r2c": 1, "c2r": 1, "decim": 2, "interp": 2}


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(ya, x):
    return ya.DeviceArray.from_numpy(np.ascontiguousarray(x))


def filt_dev(ya, q, x):
    xd, yd = dev(ya, x), ya.DeviceArray(max(len(x), 1), x.dtype)
    q.execute_block_dev(xd, len(x), yd)
    ya.synchronize()
    return yd.to_numpy(len(x))


def rate_dev(ya, q, x, interp):
    M = q.get_rate()
    n = len(x) if interp else len(x) // M
    xd, yd = dev(ya, x), ya.DeviceArray(max(n * M if interp else n, 1), x.dtype)
    q.execute_block_dev(xd, n, yd)
    ya.synchronize()
    return yd.to_numpy(n * M if interp else n)


def hilb_dev(ya, q, mode, x):
    n = len(x) // H_IN[mode][1]
    ydt, per = H_OUT[mode]
    xd, yd = dev(ya, x), ya.DeviceArray(max(n * per, 1), ydt)
    getattr(q, mode + "_execute_block_dev")(xd, n, yd)
    ya.synchronize()
    return yd.to_numpy(n * per)


def stable_sos(rng, kind, nsos, rmax=0.95):
    b, a = [], []
    for k in range(nsos):
        r, th = rng.uniform(0.5, rmax), rng.uniform(0.02, 3.0)
        a += [1.0, -r * np.exp(1j * th), 0.0] if kind == "cccf" else [1.0, -2 * r * np.cos(th), r * r]
        b += list(rng.standard_normal(3) * (1 - r) + [1.0, 0, 0])
    return np.array(b, CDT[kind]), np.array(a, CDT[kind])


def stable_tf(rng, kind, n):
    a = rand_samples(rng, "cccf" if kind == "cccf" else "rrrf", n).astype(CDT[kind])
    a[0] = 1.0
    a[1:] *= np.float32(0.9) / np.float32(np.sum(np.abs(a[1:])))          # sum |a[1:]| < 1: stable (Rouche)
    return rand_samples(rng, "cccf" if kind == "cccf" else "rrrf", n).astype(CDT[kind]), a


def unit_counts(steps, per):
    """units per call so that the filter steps land on, just below or just above every value of `steps`"""
    out = []
    for N in steps:
        out += sorted({max(1, N // per), -(-N // per)})
    return out


# ---- check 1: fused == composed, bit for bit, on random float data ------------------------------------------------
def check_rate_composed(ya, kind, interp, M, mk_wrap, mk_filt, steps, seed):
    rng = np.random.default_rng(seed)
    q, f = mk_wrap(), mk_filt()
    for n in unit_counts(steps, M):
        x = rand_samples(rng, kind, n if interp else n * M)
        got = rate_dev(ya, q, x, interp)
        want = filt_dev(ya, f, zero_stuff(x, M)) if interp else filt_dev(ya, f, x)[::M]
        assert np.array_equal(bits(got), bits(want)), (n, M)
    # the carried state: per-sample calls on the host mirror continue identically
    x = rand_samples(rng, kind, 3 if interp else 3 * M)
    got = np.concatenate([q.execute(v) for v in x]) if interp else np.array([q.execute(x[i * M:(i + 1) * M]) for i in range(3)])
    u = zero_stuff(x, M) if interp else x
    want = np.array([f.execute(v) for v in u], DT[kind])
    assert np.array_equal(got.astype(DT[kind]), want if interp else want[::M])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", RATES)
@pytest.mark.parametrize("interp", [False, True], ids=["decim", "interp"])
def test_rate_fused_equals_composed(ya, kind, M, interp):
    b, a = stable_sos(np.random.default_rng(10 + M), kind, 1)
    W = ya.IirInterpolationFilter if interp else ya.IirDecimationFilter
    check_rate_composed(ya, kind, interp, M, lambda: W.new_sos(kind, M, b, a, 1), lambda: ya.IirFilter.new_sos(kind, b, a, 1),
                        STEPS, 1000 + M)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("interp", [False, True], ids=["decim", "interp"])
def test_rate_fused_equals_composed_tf(ya, kind, n, interp):
    """the transfer-function form: the deque head advances by the number of filter steps (M = 3 and 5 are coprime
    to n = 2 and 8, so every head position starts a call)"""
    b, a = stable_tf(np.random.default_rng(20 + n), kind, n)
    W = ya.IirInterpolationFilter if interp else ya.IirDecimationFilter
    for M in (3, 5):
        check_rate_composed(ya, kind, interp, M, lambda: W(kind, M, b, a), lambda: ya.IirFilter(kind, b, a), SHORT, 2000 + n + M)


@pytest.mark.parametrize("interp", [False, True], ids=["decim", "interp"])
def test_rate_set_scale(ya, interp):
    """set_scale / get_scale (extensions: the reference's wrappers keep their filter private) act as IirFilter's"""
    b, a = stable_sos(np.random.default_rng(25), "cccf", 2)
    W = ya.IirInterpolationFilter if interp else ya.IirDecimationFilter

    def mk_wrap():
        q = W.new_sos("cccf", 3, b, a, 2)
        q.set_scale(0.25 - 1.5j)
        assert q.get_scale() == np.complex64(0.25 - 1.5j)
        return q

    def mk_filt():
        f = ya.IirFilter.new_sos("cccf", b, a, 2)
        f.set_scale(0.25 - 1.5j)
        return f
    check_rate_composed(ya, "cccf", interp, 3, mk_wrap, mk_filt, SHORT, 2500)


@pytest.mark.parametrize("interp", [False, True], ids=["decim", "interp"])
def test_rate_grouped_cascade(ya, interp):
    """17 sections run as two kernel passes: the input map belongs to the first, the output map to the last"""
    b, a = stable_sos(np.random.default_rng(30), "crcf", 17, rmax=0.9)
    W = ya.IirInterpolationFilter if interp else ya.IirDecimationFilter
    check_rate_composed(ya, "crcf", interp, 3, lambda: W.new_sos("crcf", 3, b, a, 17),
                        lambda: ya.IirFilter.new_sos("crcf", b, a, 17), SHORT, 3000)


def hilb_composed(ya, f, mode, x, state):
    v = filt_dev(ya, f, hilb_input(mode, x, state))
    return hilb_output(mode, v, state)


@pytest.mark.parametrize("mode", HMODES)
@pytest.mark.parametrize("nsos", [1, 3, 17])
def test_hilbert_fused_equals_composed(ya, mode, nsos):
    rng = np.random.default_rng(40 + nsos)
    b, a = stable_sos(rng, "rrrf", nsos, rmax=0.9)
    q, f = ya.IirHilbertFilter.new_sos(b, a, nsos), ya.IirFilter.new_sos("crcf", b, a, nsos)
    kind, per = H_IN[mode]
    state = 0
    for n in unit_counts(STEPS if nsos == 1 else SHORT, H_STEPS[mode]):
        assert q.get_state() == state
        x = rand_samples(rng, kind, n * per)
        got, want = hilb_dev(ya, q, mode, x), hilb_composed(ya, f, mode, x, state)
        assert np.array_equal(bits(got), bits(want)), (mode, n, state)
        state = (state ^ (n & 1)) if H_STEPS[mode] == 2 else (state + n) & 3
    x = rand_samples(rng, kind, 5 * per)
    got = getattr(q, mode + "_execute_block")(x)                       # 5 or 10 steps: the host mirror
    want = hilb_output(mode, np.array([f.execute(v) for v in hilb_input(mode, x, state)], np.complex64), state)
    assert np.array_equal(bits(got), bits(want))


# ---- check 2: == the reference's loop, bit for bit ----------------------------------------------------------------
SOS_A = [[1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [1.0, 0.0, 1.0], [1.0, 0.0, -1.0]]


def sos_int(nsos):
    a = np.array([SOS_A[k % 4] for k in range(nsos)], np.float32)
    b = a.copy()                       # b = a: unit gain per section, the states still carry the sums
    b[-1] = [1.0, 1.0, 0.0]            # the last section keeps a pole: the output carries state too
    return b.ravel(), a.ravel()


def int_signal(rng, kind, n):
    if kind == "rrrf":
        return rng.integers(-1, 2, n).astype(np.float32)
    return (rng.integers(-1, 2, n) + 1j * rng.integers(-1, 2, n)).astype(np.complex64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [2, 5])
@pytest.mark.parametrize("interp", [False, True], ids=["decim", "interp"])
def test_rate_bitwise_vs_reference_loop(ya, kind, M, interp):
    rng = np.random.default_rng(50 + M)
    b, a = sos_int(2)
    bc, ac = b.astype(CDT[kind]), a.astype(CDT[kind])
    W, R = (ya.IirInterpolationFilter, IirInterpRef) if interp else (ya.IirDecimationFilter, IirDecimRef)
    q, r = W.new_sos(kind, M, bc, ac, 2), R(kind, M, b, a, nsos=2)
    units, pin = 4500 // M, (1 if interp else M)
    x = int_signal(rng, kind, units * pin)
    cuts = [0, 3, 3 + 40 // M, 700 // M, 701 // M + 9, 2800 // M, 2800 // M + 2, units]    # units; odd points
    got = []
    for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        xs = x[lo * pin:hi * pin]
        if i % 3 == 0:
            got.append(q.execute_block(xs) if interp else q.execute_block(xs, hi - lo))   # host data (mirror or staged)
        elif i % 3 == 1:
            got.append(rate_dev(ya, q, xs, interp))
        else:
            got.append(np.concatenate([np.atleast_1d(q.execute(xs[j] if interp else xs[j * M:(j + 1) * M]))
                                       for j in range(hi - lo)]).astype(DT[kind]))
    assert np.array_equal(np.concatenate(got), r.execute_block(x))


@pytest.mark.parametrize("mode", HMODES)
def test_hilbert_bitwise_vs_two_real_filters(ya, mode):
    """integer data over a whole stream cut at odd points, host and device calls mixed: one crcf filter equals the
    reference's two real ones"""
    rng = np.random.default_rng(60)
    b, a = sos_int(3)
    q, r = ya.IirHilbertFilter.new_sos(b, a, 3), IirHilbRef(b, a, 3)
    kind, per = H_IN[mode]
    units = 2400 // H_STEPS[mode]
    x = int_signal(rng, kind, units * per)
    cuts = [0, 5, 16, 600, 607, 1100, units]
    got = []
    for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        xs = x[lo * per:hi * per]
        if i % 3 == 0:
            got.append(getattr(q, mode + "_execute_block")(xs))
        elif i % 3 == 1:
            got.append(hilb_dev(ya, q, mode, xs))
        else:
            one = getattr(q, mode + "_execute")
            got.append(np.concatenate([np.atleast_1d(one(xs[j * per:(j + 1) * per] if per == 2 else xs[j]))
                                       for j in range(hi - lo)]))
    want = getattr(r, mode + "_execute_block")(x)
    assert np.array_equal(np.concatenate(got).astype(want.dtype), want)


@pytest.mark.parametrize("mode", HMODES)
def test_hilbert_first_chunk_bitwise_on_float_data(ya, mode):
    """float data on the designed filter: a device block that fits one chunk starts from the exactly carried state, so
    every word is the reference's two-filter arithmetic"""
    rng = np.random.default_rng(70)
    b, a = ya.iir_design_lowpass_sos(ya.IirFilterShape.Butter, 5, 0.25, 0.1, 60.0)
    q, r = ya.IirHilbertFilter.new_default(5), IirHilbRef(b.ravel(), a.ravel(), 3)
    kind, per = H_IN[mode]
    for n in (7, 64 // H_STEPS[mode], 20):                   # <= 64 steps each: 6 state entries -> chunks of 64
        x = rand_samples(rng, kind, n * per)
        got = hilb_dev(ya, q, mode, x)
        want = getattr(r, mode + "_execute_block")(x)
        assert np.array_equal(bits(got), bits(want)), n


@pytest.mark.parametrize("interp", [False, True], ids=["decim", "interp"])
def test_rate_first_chunk_bitwise_on_float_data(ya, interp):
    rng = np.random.default_rng(71)
    b, a = ya.iir_design_lowpass_sos(ya.IirFilterShape.Cheby2 if interp else ya.IirFilterShape.Butter, 7, 0.5 / 3, 0.1, 60.0)
    W, R = (ya.IirInterpolationFilter, IirInterpRef) if interp else (ya.IirDecimationFilter, IirDecimRef)
    q, r = W.new_default("crcf", 3, 7), R("crcf", 3, b.ravel(), a.ravel(), nsos=4, scale=3.0 if interp else 1.0)
    for n in (5, 21, 11):                                    # <= 64 steps: 8 state entries -> chunks of 64
        x = rand_samples(rng, "crcf", n if interp else 3 * n)
        assert np.array_equal(rate_dev(ya, q, x, interp), r.execute_block(x))


# ---- check 3: the Hilbert state -------------------------------------------------------------------------------------
def test_hilbert_state_interleaved(ya):
    rng = np.random.default_rng(80)
    b, a = sos_int(2)
    q, r = ya.IirHilbertFilter.new_sos(b, a, 2), IirHilbRef(b, a, 2)
    # (mode, units): r2c / c2r start at every state 0..3, decim / interp at both toggles; device sizes above 32 steps
    plan = [("decim", 35), ("interp", 33), ("interp", 40), ("decim", 3), ("decim", 50), ("r2c", 41), ("c2r", 45),
            ("r2c", 34), ("c2r", 3), ("c2r", 37), ("r2c", 33), ("r2c", 41), ("c2r", 40), ("decim", 37), ("r2c", 2),
            ("interp", 34)]
    seen = {m: set() for m in HMODES}
    for mode, n in plan:
        assert q.get_state() == r.state
        if mode in ("decim", "interp") and r.state > 1:
            with pytest.raises(ya.ModeError, match="reset first"):
                hilb_dev(ya, q, mode, int_signal(rng, H_IN[mode][0], n * H_IN[mode][1]))
            with pytest.raises(ya.ModeError):
                getattr(q, mode + "_execute_block")(int_signal(rng, H_IN[mode][0], H_IN[mode][1]))
            assert q.get_state() == r.state
            mode = "r2c"                                     # walk on to a state the reference accepts
        seen[mode].add(r.state)
        x = int_signal(rng, H_IN[mode][0], n * H_IN[mode][1])
        got = hilb_dev(ya, q, mode, x)
        want = getattr(r, mode + "_execute_block")(x)
        assert np.array_equal(got.astype(want.dtype), want), (mode, n)
    assert seen["r2c"] == seen["c2r"] == {0, 1, 2, 3} and seen["decim"] == seen["interp"] == {0, 1}, seen
    for st in (2, 3):                                        # the error at state 2 and at state 3
        q.reset()
        hilb_dev(ya, q, "r2c", int_signal(rng, "rrrf", 32 + st))
        assert q.get_state() == st
        for mode in ("decim", "interp"):
            with pytest.raises(ya.ModeError, match="reset first"):
                hilb_dev(ya, q, mode, int_signal(rng, H_IN[mode][0], 40 * H_IN[mode][1]))


@pytest.mark.parametrize("mode", ["decim", "interp"])
def test_hilbert_clone_and_reset(ya, mode):                  # iirhilb.rs:331-380
    rng = np.random.default_rng(81)
    q0 = ya.IirHilbertFilter(ya.IirFilterShape.Cheby2, 7, 0.1, 80.0)
    kind, per = H_IN[mode]
    x0 = rand_samples(rng, kind, 81 * per)
    first = hilb_dev(ya, q0, mode, x0)
    q1 = q0.clone()
    assert q1.get_state() == q0.get_state() == 1
    x = rand_samples(rng, kind, 80 * per)
    y0 = hilb_dev(ya, q0, mode, x)
    assert np.array_equal(y0, hilb_dev(ya, q1, mode, x))
    one = getattr(q0, mode + "_execute"), getattr(q1, mode + "_execute")
    for j in range(4):
        v = x[j * per:(j + 1) * per] if per == 2 else x[j]
        assert np.array_equal(np.atleast_1d(one[0](v)), np.atleast_1d(one[1](v)))
    q0.reset()
    assert q0.get_state() == 0
    assert np.array_equal(hilb_dev(ya, q0, mode, x0), first)


@pytest.mark.parametrize("interp", [False, True], ids=["decim", "interp"])
def test_rate_clone_and_reset(ya, interp):                   # iirinterp.rs:195-218
    rng = np.random.default_rng(82)
    W = ya.IirInterpolationFilter if interp else ya.IirDecimationFilter
    q0 = W.new_default("crcf", 3, 7)
    x0 = rand_samples(rng, "crcf", 50 * (1 if interp else 3))
    first = rate_dev(ya, q0, x0, interp)
    q1 = q0.clone()
    assert q1.get_rate() == 3 and q1.get_scale() == q0.get_scale()
    x = rand_samples(rng, "crcf", 64 * (1 if interp else 3))
    assert np.array_equal(rate_dev(ya, q0, x, interp), rate_dev(ya, q1, x, interp))
    q0.reset()
    assert np.array_equal(rate_dev(ya, q0, x0, interp), first)


# ---- check 4: accuracy on designed filters ---------------------------------------------------------------------------
TAU = 2e-7          # the device error is at most twice the sequential f32 error + 2e-7 ||y||


def assert_accuracy(y_dev, y_seq, y64, what):
    e_dev, e_seq = np.linalg.norm(y_dev - y64), np.linalg.norm(y_seq - y64)
    print(f"{what}: dev {e_dev / np.linalg.norm(y64):.3e} seq {e_seq / np.linalg.norm(y64):.3e}")
    assert e_dev <= 2 * e_seq + TAU * np.linalg.norm(y64), (what, e_dev, e_seq)


@pytest.mark.parametrize("interp", [False, True], ids=["decim", "interp"])
def test_rate_accuracy_designed(ya, interp):
    rng = np.random.default_rng(90)
    M, steps = 3, 1 << 18
    units = steps // M
    S = ya.IirFilterShape
    b, a = ya.iir_design_lowpass_sos(S.Cheby2 if interp else S.Butter, 7, 0.5 / M, 0.1, 60.0)
    W = ya.IirInterpolationFilter if interp else ya.IirDecimationFilter
    x = rand_samples(rng, "crcf", units if interp else units * M)
    u = zero_stuff(x, M) if interp else x
    y64 = iir64("crcf", b.ravel(), a.ravel(), u, nsos=4, scale=3.0 if interp else 1.0, chunk=1024)
    y64 = y64 if interp else y64[::M]
    y_dev = rate_dev(ya, W.new_default("crcf", M, 7), x, interp)
    q, per = W.new_default("crcf", M, 7), (1 if interp else M)
    y_seq = np.concatenate([q.execute_block(x[i * per:(i + 10) * per]) if interp else q.execute_block(x[i * per:(i + 10) * per], min(10, units - i))
                            for i in range(0, units, 10)])              # 30 steps per call: the host mirror
    assert_accuracy(y_dev, y_seq, y64, "interp" if interp else "decim")


@pytest.mark.parametrize("mode", HMODES)
def test_hilbert_accuracy_designed(ya, mode):
    rng = np.random.default_rng(91)
    b, a = ya.iir_design_lowpass_sos(ya.IirFilterShape.Butter, 5, 0.25, 0.1, 60.0)
    kind, per = H_IN[mode]
    units = (1 << 18) // H_STEPS[mode]
    x = rand_samples(rng, kind, units * per)
    v64 = iir64("crcf", b.ravel(), a.ravel(), hilb_input(mode, x, 0), nsos=3, chunk=1024)
    k = np.arange(len(v64)) & 3
    if mode == "r2c":
        y64 = 2 * v64 * np.choose(k, [1, 1j, -1, -1j])
    elif mode == "decim":
        y64 = 2 * v64[::2]
    else:
        y64 = np.choose(k, [v64.real, -v64.imag, -v64.real, v64.imag]) * (2 if mode == "interp" else 1)
    y_dev = hilb_dev(ya, ya.IirHilbertFilter.new_default(5), mode, x)
    q, nb = ya.IirHilbertFilter.new_default(5), 32 // H_STEPS[mode]
    y_seq = np.concatenate([getattr(q, mode + "_execute_block")(x[i * per:(i + nb) * per]) for i in range(0, units, nb)])
    assert_accuracy(y_dev, y_seq, y64, mode)


# ---- check 5: the reference's Hilbert spectral tests through the device path ----------------------------------------
def test_iirhilbf_interp_decim_masks(ya):                    # iirhilb.rs:175-231
    tol, bw, as_, p, m = 1.0, 0.4, 60.0, 40, 5
    q = ya.IirHilbertFilter.new_default(m)
    h_len = 2 * p + 1
    n = h_len + 2 * m + 8
    w = np.float32(0.36 * bw)
    h = ya.fir_design_kaiser(h_len, float(w), 80.0, 0.0)
    buf0 = np.zeros(n, np.complex64)
    buf0[:h_len] = np.float32(2.0) * w * h
    buf1 = hilb_dev(ya, q, "interp", buf0)
    q.reset()
    buf2 = hilb_dev(ya, q, "decim", buf1)
    orig = [(-0.5, -0.5 * bw, 0.0, -as_ + tol, False, True), (-0.3 * bw, 0.3 * bw, -1.0, 1.0, True, True),
            (0.5 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    interp = [(-0.5, -0.25 - 0.25 * bw, 0.0, -as_ + tol, False, True), (-0.25 - 0.15 * bw, -0.25 + 0.15 * bw, -1.0, 1.0, True, True),
              (-0.25 + 0.25 * bw, 0.25 - 0.25 * bw, 0.0, -as_ + tol, False, True),
              (0.25 - 0.15 * bw, 0.25 + 0.15 * bw, -1.0, 1.0, True, True), (0.25 + 0.25 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    assert validate_psd_signal(buf0, orig)[0]
    assert validate_psd_signal(buf1, interp)[0]
    assert validate_psd_signal(buf2, orig)[0]


def test_iirhilbf_filter_masks(ya):                          # iirhilb.rs:233-317
    tol, bw, f0, ft, as_, p, m = 1.0, 0.2, 0.3, -0.3, 60.0, 50, 7
    q = ya.IirHilbertFilter.new_default(m)
    h_len = 2 * p + 1
    n = h_len + 2 * m + 8
    w = 0.36 * bw
    h = ya.fir_design_kaiser(h_len, w, 80.0, 0.0).astype(np.float64)
    i = np.arange(h_len)
    buf0 = np.zeros(n, np.complex128)
    buf0[:h_len] = 2.0 * w * h * np.exp(2j * np.pi * f0 * i) + 1e-3 * np.kaiser(n, 10.0)[:h_len] * np.exp(2j * np.pi * ft * i)
    buf0 = buf0.astype(np.complex64)
    buf1 = hilb_dev(ya, q, "c2r", buf0) * np.float32(2.0)
    q.reset()
    buf2 = hilb_dev(ya, q, "r2c", buf1) * np.float32(0.5)
    orig = [(-0.5, ft - 0.03, 0.0, -as_ + tol, False, True), (ft - 0.01, ft + 0.01, -40.0, 0.0, True, False),
            (ft + 0.03, f0 - 0.5 * bw, 0.0, -as_ + tol, False, True), (f0 - 0.3 * bw, f0 + 0.3 * bw, -1.0, 1.0, True, True),
            (f0 + 0.5 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    c2r = [(-0.5, -f0 - 0.5 * bw, 0.0, -as_ + tol, False, True), (-f0 - 0.3 * bw, -f0 + 0.3 * bw, -1.0, 1.0, True, True),
           (-f0 + 0.5 * bw, f0 - 0.5 * bw, 0.0, -as_ + tol, False, True), (f0 - 0.3 * bw, f0 + 0.3 * bw, -1.0, 1.0, True, True),
           (f0 + 0.5 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    r2c = [(-0.5, f0 - 0.5 * bw, 0.0, -as_ + tol, False, True), (f0 - 0.3 * bw, f0 + 0.3 * bw, -1.0, 1.0, True, True),
           (f0 + 0.5 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    assert validate_psd_signal(buf0, orig)[0]
    assert validate_psd_signal(buf1, c2r)[0]
    assert validate_psd_signal(buf2, r2c)[0]


def welch_psd(y, nfft):
    """the reference's Spgram(nfft, Hann, nfft / 2, nfft / 4).get_psd() as an independent numpy Welch estimate (Hann
    window of nfft / 2, hop nfft / 4, white unit-variance noise -> 0 dB), no project code on the measuring side"""
    wl, hop = nfft // 2, nfft // 4
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(wl) / (wl - 1))
    segs = np.lib.stride_tricks.sliding_window_view(np.asarray(y, np.complex128), wl)[::hop]
    psd = np.mean(np.abs(np.fft.fft(segs * w, nfft, axis=1)) ** 2, axis=0) / np.sum(w * w)
    return 10 * np.log10(np.fft.fftshift(psd))


def check_mask(psd, regions):
    f = np.arange(len(psd)) / len(psd) - 0.5
    for fmin, fmax, pmin, pmax, lo, hi in regions:
        sel = (f >= fmin) & (f <= fmax)
        if lo:
            assert psd[sel].min() >= pmin, (fmin, fmax, psd[sel].min())
        if hi:
            assert psd[sel].max() <= pmax, (fmin, fmax, psd[sel].max())


def symstream_standin(ya, rng, n, B, gain):
    """stand-in for SymStreamR(Kaiser, bandwidth B, m 25, beta 0.2, QPSK) with set_gain(gain): complex white noise
    shaped by a 241-tap Kaiser low-pass (80 dB) whose transition lies inside the 20 % excess bandwidth of the
    reference's pulse, 0.4 B .. 0.55 B.  Power gain^2 spread flat over B: PSD level gain^2 / B."""
    h = ya.fir_design_kaiser(241, 0.475 * B, 80.0, 0.0).astype(np.float64)
    w = (rng.standard_normal(n + 240) + 1j * rng.standard_normal(n + 240)) * np.sqrt(0.5)
    x = np.convolve(w, h, mode="valid")[:n] / abs(h.sum())
    return (x * gain / np.sqrt(B)).astype(np.complex64), h / abs(h.sum())


@pytest.mark.parametrize("M", [2, 3, 4])
def test_iirinterp_crcf_O9_masks(ya, M):                     # iirinterp.rs:135-193, autotest_iirinterp_crcf_M{2,3,4}_O9
    n, bw, nfft, as_, tol, order = 800000, 0.2, 800, 60.0, 0.5, 9
    rng = np.random.default_rng(110 + M)
    B = bw * M
    x, h = symstream_standin(ya, rng, n // M + 1, B, np.sqrt(bw))
    # the stand-in meets the mask on its own, at the input rate (level 1 / M: the interpolator brings it to 0 dB):
    # exactly, by its shaping filter, and as measured
    f = np.arange(nfft) / nfft - 0.5
    resp = 20 * np.log10(np.abs(np.exp(-2j * np.pi * np.outer(f, np.arange(len(h)))) @ h) + 1e-300)
    assert np.max(np.abs(resp[np.abs(f) <= 0.4 * B])) < 0.01 and np.max(resp[np.abs(f) >= 0.6 * B]) < -as_ - 15.0
    check_mask(welch_psd(x, nfft) + 10 * np.log10(M), [(-0.5, -0.6 * B, 0.0, -as_ + tol, False, True),
                                                        (-0.4 * B, 0.4 * B, -tol, tol, True, True),
                                                        (0.6 * B, 0.5, 0.0, -as_ + tol, False, True)])
    q = ya.IirInterpolationFilter.new_default("crcf", M, order)
    out, blk = [], 36001                                     # device blocks, cut at an odd length
    for o in range(0, len(x), blk):
        out.append(rate_dev(ya, q, x[o:o + blk], True))
    y = np.concatenate(out)[:n + nfft // 2]
    assert len(y) >= n
    psd = welch_psd(y, nfft)
    f0 = np.abs(f) <= 0.4 * bw
    print(f"M={M}: pass-band {psd[f0].min():+.3f} .. {psd[f0].max():+.3f} dB, stop-band max {psd[np.abs(f) >= 0.6 * bw].max():.2f} dB")
    check_mask(psd, [(-0.5, -0.6 * bw, 0.0, -as_ + tol, False, True), (-0.4 * bw, 0.4 * bw, 0.0 - tol, 0.0 + tol, True, True),
                     (0.6 * bw, 0.5, 0.0, -as_ + tol, False, True)])


# ---- check 6: config errors and group delay ------------------------------------------------------------------------
def test_config_errors_and_groupdelay(ya):
    S = ya.IirFilterShape
    b, a = ya.iir_design_lowpass_sos(S.Butter, 4, 0.2)
    for W in (ya.IirDecimationFilter, ya.IirInterpolationFilter):
        for M in (0, 1):
            with pytest.raises(ya.ConfigError):
                W("crcf", M, [1.0, 0.5], [1.0, -0.5])
            with pytest.raises(ya.ConfigError):
                W.new_sos("crcf", M, b, a, 2)
            with pytest.raises(ya.ConfigError):
                W.new_default("crcf", M, 5)
            with pytest.raises(ya.ConfigError):
                W.new_prototype("crcf", M, S.Butter, 5, 0.2, 0.1, 60.0)
        with pytest.raises(ya.ConfigError):
            W.new_default("crcf", 2, 0)
        with pytest.raises(ya.ConfigError, match="65536"):   # the kernels' 32-bit index split
            W.new_sos("crcf", 65537, b, a, 2)
        with pytest.raises(ya.ConfigError, match="65536"):
            W("crcf", 65537, [1.0, 0.5], [1.0, -0.5])
        assert W.new_sos("crcf", 65536, b, a, 2).get_rate() == 65536
        with pytest.raises(ya.ConfigError):
            W("rrrf", 2, [], [1.0])
        with pytest.raises(ya.ConfigError):
            W("rrrf", 2, [1.0], [])
        with pytest.raises(ya.ConfigError):
            W.new_sos("rrrf", 2, [], [], 0)
        for shape in (S.Cheby1, S.Ellip, S.Bessel):
            with pytest.raises(ya.ConfigError, match="not built"):
                W.new_prototype("crcf", 2, shape, 5, 0.2, 0.1, 60.0)
    with pytest.raises(ya.ConfigError, match="decimation factor"):
        ya.IirDecimationFilter.new_default("crcf", 1, 5)
    with pytest.raises(ya.ConfigError, match="interp factor"):
        ya.IirInterpolationFilter.new_default("crcf", 1, 5)
    with pytest.raises(ya.ConfigError):                      # iirhilb.rs:319-324
        ya.IirHilbertFilter(S.Butter, 0, 0.1, 60.0)
    with pytest.raises(ya.ConfigError):
        ya.IirHilbertFilter.new_default(0)
    with pytest.raises(ya.ConfigError, match="not built"):
        ya.IirHilbertFilter(S.Ellip, 7, 0.1, 80.0)
    with pytest.raises(ya.ConfigError):
        ya.IirHilbertFilter.new_sos([], [], 0)
    with pytest.raises(ya.ConfigError):
        ya.IirFilter.new_lowpass("crcf", 0, 0.2)
    with pytest.raises(ya.ConfigError):
        ya.IirFilter.new_prototype("crcf", S.Butter, 5, 0.5, 0.1, 60.0)
    f = ya.IirFilter.new_lowpass("crcf", 7, 0.5 / 3)
    assert f.get_length() == 8
    d, i = ya.IirDecimationFilter.new_default("crcf", 3, 7), ya.IirInterpolationFilter.new_prototype("crcf", 3, S.Butter, 7, 0.5 / 3, 0.1, 60.0)
    assert d.get_decim() == 3 and i.get_interp() == 3
    assert d.get_scale() == np.float32(1.0) and i.get_scale() == np.float32(3.0)
    assert ya.IirInterpolationFilter.new_sos("crcf", 3, b, a, 2).get_scale() == np.float32(1.0)
    for fc in (0.0, 0.05, 0.1):
        assert d.groupdelay(fc) == f.groupdelay(fc)
        assert i.groupdelay(fc) == np.float32(f.groupdelay(fc) / np.float32(3.0))


# ---- check 7: execution -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["decim", "interp"])
def test_hilbert_in_place(ya, mode):
    """decim and interp move the same bytes per unit (2 floats <-> 1 complex): x_dev == y_dev is allowed"""
    rng = np.random.default_rng(100)
    kind, per = H_IN[mode]
    n = (3 * 4096 + 6) // 2
    x = rand_samples(rng, kind, n * per)
    want = hilb_dev(ya, ya.IirHilbertFilter.new_default(5), mode, x)
    q, xd = ya.IirHilbertFilter.new_default(5), dev(ya, x)
    getattr(q, mode + "_execute_block_dev")(xd, n, xd)
    ya.synchronize()
    got = np.frombuffer(xd.to_numpy().tobytes(), want.dtype)
    assert np.array_equal(got, want)
    yd = ya.DeviceArray(n * 2, np.float32)
    with pytest.raises(ya.ConfigError, match="overlap"):     # r2c / c2r change the element size: no overlap at all
        q.r2c_execute_block_dev(yd, n, yd)


def test_set_stream(ya):
    import torch
    rng = np.random.default_rng(101)
    s = torch.cuda.Stream()
    n = 3 * 4096 + 5
    for mk, run, x in [(lambda: ya.IirDecimationFilter.new_default("crcf", 3, 7), lambda q, x: rate_dev(ya, q, x, False), rand_samples(rng, "crcf", n // 3 * 3)),
                       (lambda: ya.IirInterpolationFilter.new_default("crcf", 3, 7), lambda q, x: rate_dev(ya, q, x, True), rand_samples(rng, "crcf", n // 3)),
                       (lambda: ya.IirHilbertFilter.new_default(5), lambda q, x: hilb_dev(ya, q, "r2c", x), rand_samples(rng, "rrrf", n))]:
        want = run(mk(), x)
        q = mk()
        q.set_stream(s.cuda_stream)
        got = run(q, x)
        assert np.array_equal(got, want)
        q.set_stream(0)
