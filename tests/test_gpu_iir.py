"""IirFilter through the C ABI -- src/filter/iir/iirfilt.rs and iirfiltsos.rs, their tests (iirfilt.rs:483-986,
iirfiltsos.rs:130-282) and the chunked state scan of iir_kernels.hip.

Integer taps and inputs with poles on the unit circle keep every value an exact integer in f32 and f64, so the
device path, the host path and the restatement iir_ref.Seq32 agree bit for bit.  Float data is checked against the
f64 references of iir_ref: the device path must be no less accurate than the reference's own f32 arithmetic."""
import numpy as np
import pytest

from pathlib import Path

from gpu_util import rand_samples, rel_l2
from iir_ref import Seq32, iir64

pytestmark = pytest.mark.gpu
KINDS = ["rrrf", "crcf", "cccf"]
GOLD = np.load(Path(__file__).resolve().parent / "golden" / "iirfilt.npz")
DT = {"rrrf": np.float32, "crcf": np.complex64, "cccf": np.complex64}
CDT = {"rrrf": np.float32, "crcf": np.float32, "cccf": np.complex64}
WG = 64                    # chunks per workgroup (kernels.hpp kIirWg)


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


def run_dev(ya, q, x):
    xd = ya.DeviceArray.from_numpy(np.ascontiguousarray(x))
    yd = ya.DeviceArray(max(len(x), 1), x.dtype)
    q.execute_block_dev(xd, len(x), yd)
    return yd.to_numpy(len(x))


def run_host(q, x):
    """the library's host path: 32-sample host blocks run on the host mirror in the reference's order"""
    y = np.empty_like(x)
    for i in range(0, len(x), 32):
        y[i:i + 32] = q.execute_block(x[i:i + 32])
    return y


# ---- golden vectors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h", [3, 5, 7])
@pytest.mark.parametrize("path", ["execute", "execute_block", "execute_block_dev"])
def test_kat(ya, kind, h, path):
    b, a, x, y = (GOLD[f"{kind}_h{h}_{p}"] for p in "baxy")
    q = ya.IirFilter(kind, b, a)
    assert q.get_length() == h
    if path == "execute":
        got = np.array([q.execute(v) for v in x], DT[kind])
    elif path == "execute_block":
        got = q.execute_block(x)
    else:
        got = run_dev(ya, q, x)
    np.testing.assert_allclose(got, y, rtol=1e-3, atol=1e-3)          # iirfilt.rs:806-823, epsilon 0.001
    # 64 samples are one chunk that starts from the exact (zero) state: every path is the reference's f32 order, bit for
    # bit (execute_block above 32 samples runs on the device)
    assert np.array_equal(got, Seq32(kind, b, a).execute_block(x))


FLOAT_FORMS = [("tf", 3), ("tf", 7), ("tf", 17), ("tf", 33), ("sos", 1), ("sos", 4), ("sos", 8), ("sos", 16)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form,order", FLOAT_FORMS)
def test_first_chunk_bitwise_on_float_data(ya, kind, form, order):
    """float data, every state size: the first chunk of a device block starts from the exact carried state, so its T
    outputs are the reference's f32 arithmetic bit for bit (a fused or reordered recurrence would differ here); the
    later chunks start from rounded f64 states and stay close"""
    rng = np.random.default_rng(500 + order + 7 * KINDS.index(kind))
    if form == "tf":
        # sum |a[1:]| = 0.9 < 1: stable whatever the f32 rounding of the coefficients (Rouche)
        a = rand_samples(rng, "cccf" if kind == "cccf" else "rrrf", order).astype(CDT[kind])
        a[0] = 1.0
        a[1:] *= np.float32(0.9) / np.float32(np.sum(np.abs(a[1:])))
        b = rand_samples(rng, "cccf" if kind == "cccf" else "rrrf", order).astype(CDT[kind])
        q, r, S = ya.IirFilter(kind, b, a), Seq32(kind, b, a), order - 1
    else:
        b, a = stable_sos(rng, kind, order, rmax=0.9)
        q, r, S = ya.IirFilter.new_sos(kind, b, a, order), Seq32(kind, b, a, nsos=order), 2 * order
    T = chunk_len(S)
    x = rand_samples(rng, kind, 3 * T + 5)
    y = run_dev(ya, q, x)
    want = r.execute_block(x)
    assert np.array_equal(y[:T], want[:T])
    np.testing.assert_allclose(y, want, rtol=1e-3, atol=1e-4 * np.max(np.abs(want)))


@pytest.mark.parametrize("t", ["impulse", "step"])
def test_sos_impulse_step(ya, t):                                        # iirfiltsos.rs:137-244
    b, a, want = GOLD[f"sos_{t}_b"], GOLD[f"sos_{t}_a"], GOLD[f"sos_{t}_y"]
    x = np.zeros(15, np.float32)
    if t == "impulse":
        x[0] = 1.0
    else:
        x[:] = 1.0
    for path in range(3):
        q = ya.IirFilter.new_sos("rrrf", b, a, 1)
        got = (np.array([q.execute(v) for v in x]) if path == 0 else q.execute_block(x) if path == 1
               else run_dev(ya, q, x))
        np.testing.assert_allclose(got, want, atol=1e-4)


def test_integrator_differentiator(ya):                                  # iirfilt.rs:493-538
    q = ya.IirFilter.new_integrator("rrrf")
    assert q.get_length() == 8
    x = np.zeros(40, np.float32)
    x[:10] = 1.0
    assert abs(q.execute_block(x)[-1] - 10.0) < 0.01
    q = ya.IirFilter.new_differentiator("rrrf")
    x = np.arange(400, dtype=np.float32)
    assert abs(q.execute_block(x)[-1] - 1.0) < 0.01
    q = ya.IirFilter.new_differentiator("rrrf")
    assert abs(run_dev(ya, q, x)[-1] - 1.0) < 0.01


def test_dc_blocker_spectrum(ya):                                        # iirfilt.rs:540-578
    rng = np.random.default_rng(11)
    n, nfft, tol = 400000, 1200, 0.7
    q = ya.IirFilter.new_dc_blocker("crcf", 0.2)
    assert np.isclose(q.get_scale(), np.sqrt(np.float32(0.8)))
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)).astype(np.complex64)
    y = q.execute_block(x)
    # the mask is measured with an independent numpy Welch estimate of the reference's Spgram(nfft, Hann, nfft / 2,
    # nfft / 4): Hann window of 600, hop 300, nfft 1200, white noise -> 0 dB (no project code on the measuring side)
    wl, hop = nfft // 2, nfft // 4
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(wl) / (wl - 1))
    segs = np.lib.stride_tricks.sliding_window_view(y.astype(np.complex128), wl)[::hop]
    psd = np.mean(np.abs(np.fft.fft(segs * w, nfft, axis=1)) ** 2, axis=0) / np.sum(w * w)
    psd = 10 * np.log10(np.fft.fftshift(psd))
    f = np.arange(nfft) / nfft - 0.5
    for fmin, fmax, pmin, pmax, lo, hi in [(-0.5, -0.2, -tol, tol, True, True), (-0.002, 0.002, -tol, -20.0, False, True),
                                           (0.2, 0.5, -tol, tol, True, True)]:
        sel = (f >= fmin) & (f <= fmax)
        if lo:
            assert psd[sel].min() >= pmin, (fmin, psd[sel].min())
        if hi:
            assert psd[sel].max() <= pmax, (fmin, psd[sel].max())


def test_config_scale_length(ya):                                        # iirfilt.rs:624-642
    with pytest.raises(ya.ConfigError):
        ya.IirFilter("cccf", [], [])
    with pytest.raises(ya.ConfigError):
        ya.IirFilter("cccf", [0.0], [])
    with pytest.raises(ya.ConfigError):
        ya.IirFilter("cccf", [], [1.0])
    with pytest.raises(ya.ConfigError):
        ya.IirFilter.new_sos("cccf", [], [], 0)
    with pytest.raises(ya.ConfigError):
        ya.IirFilter.new_dc_blocker("crcf", 0.0)
    for bad in [(0.0, 0.5, 1000.0), (1.0, 0.5, 1000.0), (0.1, 0.0, 1000.0), (0.1, 1.0, 1000.0), (0.1, 0.5, 0.0)]:
        with pytest.raises(ya.ConfigError):
            ya.IirFilter.new_pll("rrrf", *bad)
    with pytest.raises(ya.ConfigError, match="33"):
        ya.IirFilter("rrrf", np.ones(34, np.float32), [1.0])
    q = ya.IirFilter("crcf", GOLD["crcf_h7_b"], GOLD["crcf_h7_a"])
    q.set_scale(7.22)
    assert q.get_scale() == np.float32(7.22)
    assert q.get_length() == 7
    assert ya.IirFilter.new_sos("crcf", np.ones(12), np.ones(12), 4).get_length() == 8
    with pytest.raises(ya.ConfigError):                                  # :396-406
        q.execute_block(np.zeros(3, np.complex64), np.zeros(4, np.complex64))
    pll = ya.IirFilter.new_pll("rrrf", 0.1, 0.7071, 1000.0)
    assert pll.get_length() == 2


@pytest.mark.parametrize("t", ["n3", "n8", "sos_n8"])
def test_groupdelay(ya, t):                                              # iirfilt.rs:644-820
    b, a, fc, g0 = (GOLD[f"gd_{t}_{v}"] for v in ("b", "a", "fc", "g0"))
    q = ya.IirFilter.new_sos("rrrf", b, a, 4) if t == "sos_n8" else ya.IirFilter("rrrf", b, a)
    for f, g in zip(fc, g0):
        assert abs(q.groupdelay(f) - g) <= 1e-3 * max(1.0, abs(g)), (f, q.groupdelay(f), g)


@pytest.mark.parametrize("kind", KINDS)
def test_freqresponse(ya, kind):
    b, a = GOLD[f"{kind}_h5_b"], GOLD[f"{kind}_h5_a"]
    q = ya.IirFilter(kind, b, a)
    q.set_scale(0.5)
    bs, as_ = b.astype(np.complex128) / complex(a[0]), a.astype(np.complex128) / complex(a[0])
    for fc in (-0.4, -0.1, 0.0, 0.05, 0.2, 0.45):
        e = np.exp(2j * np.pi * fc * np.arange(5))
        want = 0.5 * np.dot(bs, e) / np.dot(as_, e)
        assert abs(q.freqresponse(fc) - want) <= 1e-4 * max(1.0, abs(want))
        assert abs(q.get_psd(fc) - 10 * np.log10(abs(want) ** 2)) < 1e-3
    sb = np.array([1.0, 0.5, 0.25, 1.0, -0.3, 0.1], CDT[kind])
    sa = np.array([1.0, -0.5, 0.2, 2.0, 0.4, 0.3], CDT[kind])
    q = ya.IirFilter.new_sos(kind, sb, sa, 2)
    e = np.exp(2j * np.pi * 0.1 * np.arange(3))
    want = np.prod([np.dot(sb[3 * k:3 * k + 3], e) / np.dot(sa[3 * k:3 * k + 3], e) for k in range(2)])
    assert abs(q.freqresponse(0.1) - want) <= 1e-5 * abs(want)


@pytest.mark.parametrize("form", ["tf", "sos"])
def test_clone(ya, form):                                                # iirfilt.rs:580-622, iirfiltsos.rs:246-275
    rng = np.random.default_rng(5)
    b, a = GOLD["crcf_h7_b"], GOLD["crcf_h7_a"]
    sb = np.array([0.0976, 0.1953, 0.0976, 1.0, 2.0, 1.0], np.float32)
    sa = np.array([1.0, -0.9428, 0.3333, 1.0, -0.5, 0.25], np.float32)
    mk = (lambda: ya.IirFilter("crcf", b, a)) if form == "tf" else (lambda: ya.IirFilter.new_sos("crcf", sb, sa, 2))
    r0 = Seq32("crcf", b, a) if form == "tf" else Seq32("crcf", sb, sa, nsos=2)
    q0 = mk()
    x = rand_samples(rng, "crcf", 83)
    assert np.array_equal(np.array([q0.execute(v) for v in x]), r0.execute_block(x))
    q1, r1 = q0.clone(), r0.clone()
    x = rand_samples(rng, "crcf", 80)
    y0 = np.array([q0.execute(v) for v in x])
    y1 = np.array([q1.execute(v) for v in x])
    assert np.array_equal(y0, r0.execute_block(x))
    assert np.array_equal(y1, r1.execute_block(x))
    if form == "sos":
        assert np.array_equal(y0, y1)
    # the clone carries on through the device path from the same state
    x = rand_samples(rng, "crcf", 5000)
    np.testing.assert_allclose(run_dev(ya, q1, x), run_dev(ya, q0, x), rtol=1e-4, atol=1e-5)


# ---- bit-exact chunked scan --------------------------------------------------------------------------------------
def int_signal(rng, kind, n):
    if kind == "rrrf":
        return rng.integers(-1, 2, n).astype(np.float32)
    return (rng.integers(-1, 2, n) + 1j * rng.integers(-1, 2, n)).astype(np.complex64)


TF_INT = {1: ([3.0], [1.0]),
          2: ([1.0, 2.0], [1.0, -1.0]),
          3: ([1.0, -1.0, 2.0], [1.0, 0.0, 1.0]),
          9: ([1.0, 0, 0, 1.0, 0, 0, 0, 0, -1.0], [1.0, 0, 0, 0, 0, 0, 0, 0, -1.0]),
          33: ([1.0] + [0.0] * 31 + [-1.0], [1.0] + [0.0] * 31 + [1.0])}
SOS_A = [[1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [1.0, 0.0, 1.0], [1.0, 0.0, -1.0]]


def sos_int(nsos):
    a = np.array([SOS_A[k % 4] for k in range(nsos)], np.float32)
    b = a.copy()                       # b = a: unit gain per section, the states still carry the sums
    b[-1] = [1.0, 1.0, 0.0]            # the last section keeps a pole: the output carries state too
    return b.ravel(), a.ravel()


def chunk_len(S):
    T = 64
    while T < 256 and T < 8 * S:
        T *= 2
    return T


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 9, 33])
def test_bitwise_tf(ya, kind, n):
    rng = np.random.default_rng(100 + n)
    b, a = TF_INT[n]
    T = chunk_len(n - 1)
    # 65 WG T + T + 1: 65 workgroup aggregates, so phase B's lanes take 2 each and the last lane's range is partial
    lens = sorted({1, 2, T - 1, T, T + 1, WG * T - 1, WG * T + 1, WG * WG * T + 1, 65 * WG * T + T + 1,
                   3 * WG * WG * T + 7})
    x = int_signal(rng, kind, sum(lens))
    want = iir64(kind, b, a, x, chunk=4096)
    q = ya.IirFilter(kind, np.array(b, CDT[kind]), np.array(a, CDT[kind]))
    got, o = [], 0
    for m in lens:                                      # one stream cut at odd points
        got.append(run_dev(ya, q, x[o:o + m]))
        o += m
    assert np.array_equal(np.concatenate(got), want)
    # host path and restatement (a) on a prefix; per-sample and block calls interleaved with device calls
    q = ya.IirFilter(kind, np.array(b, CDT[kind]), np.array(a, CDT[kind]))
    r = Seq32(kind, b, a)
    xs = x[:3000]
    y = np.concatenate([q.execute_block(xs[:17]), np.array([q.execute(v) for v in xs[17:40]], DT[kind]),
                        run_dev(ya, q, xs[40:1200]), q.execute_block(xs[1200:1231]), run_dev(ya, q, xs[1231:])])
    assert np.array_equal(y, r.execute_block(xs))
    assert np.array_equal(y, want[:3000])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nsos", [1, 4, 16, 17])
def test_bitwise_sos(ya, kind, nsos):
    rng = np.random.default_rng(200 + nsos)
    b, a = sos_int(nsos)
    T = chunk_len(2 * min(nsos, 16))
    lens = [1, 2, T - 1, T + 1, WG * T - 1, WG * T + 1, WG * WG * T + 3, 65 * WG * T + T + 1, (1 << 22) + 17]
    x = int_signal(rng, kind, sum(lens))
    want = iir64(kind, b, a, x, nsos=nsos, chunk=4096)
    q = ya.IirFilter.new_sos(kind, b.astype(CDT[kind]), a.astype(CDT[kind]), nsos)
    got, o = [], 0
    for m in lens:
        got.append(run_dev(ya, q, x[o:o + m]))
        o += m
    assert np.array_equal(np.concatenate(got), want)
    q = ya.IirFilter.new_sos(kind, b.astype(CDT[kind]), a.astype(CDT[kind]), nsos)
    r = Seq32(kind, b, a, nsos=nsos)
    xs = x[:1500]
    y = np.concatenate([np.array([q.execute(v) for v in xs[:9]], DT[kind]), run_dev(ya, q, xs[9:700]),
                        q.execute_block(xs[700:731]), q.execute_block(xs[731:])])
    assert np.array_equal(y, r.execute_block(xs))


@pytest.mark.parametrize("form", ["tf", "sos"])
def test_reset_then_device_block_then_per_sample(ya, form):
    """reset() after a device block zeroes the host mirror and leaves the device copy stale: the next device block
    must upload the zeros and the per-sample calls after it must fetch the state it left.  The whole sequence equals
    a fresh filter's, bit for bit (integer data: the transfer-function deque's kept head moves no bit)."""
    rng = np.random.default_rng(300)
    kind = "crcf"
    if form == "tf":
        b, a = TF_INT[3]
        q, r = ya.IirFilter(kind, np.array(b, CDT[kind]), np.array(a, CDT[kind])), Seq32(kind, b, a)
    else:
        b, a = sos_int(4)
        q, r = ya.IirFilter.new_sos(kind, b.astype(CDT[kind]), a.astype(CDT[kind]), 4), Seq32(kind, b, a, nsos=4)
    x = int_signal(rng, kind, 2000)
    run_dev(ya, q, x[:700])                             # the device copy is current and not zero
    q.reset()
    y = np.concatenate([run_dev(ya, q, x[700:1500]), np.array([q.execute(v) for v in x[1500:1540]], DT[kind]),
                        run_dev(ya, q, x[1540:])])
    assert np.array_equal(y, r.execute_block(x[700:]))


# ---- accuracy on float data --------------------------------------------------------------------------------------
def stable_sos(rng, kind, nsos, rmax=0.995):
    b, a = [], []
    for k in range(nsos):
        r = rmax if k == 0 else rng.uniform(0.5, rmax)
        th = rng.uniform(0.02, 3.0)
        if kind == "cccf":
            p = r * np.exp(1j * th)
            a += [1.0, -p, 0.0]                         # one complex pole per section
        else:
            a += [1.0, -2 * r * np.cos(th), r * r]
        b += list(rng.standard_normal(3) * (1 - r) + [1.0, 0, 0])
    return np.array(b, CDT[kind]), np.array(a, CDT[kind])


def stable_tf(rng, kind, n, rmax=0.995):
    poles = []
    while len(poles) < n - 1:
        r = rmax if not poles else rng.uniform(0.3, rmax)
        th = rng.uniform(0.05, 3.0)
        if kind == "cccf" or len(poles) == n - 2:
            poles.append(r * np.exp(1j * th) if kind == "cccf" else r)
        else:
            poles += [r * np.exp(1j * th), r * np.exp(-1j * th)]
    a = np.poly(poles)
    a = a if kind == "cccf" else a.real
    b = rng.standard_normal(n) * 0.1
    return np.array(b, CDT[kind]), np.array(a, CDT[kind])


# worst measured ratio ||y_dev - y64|| / ||y_seq32 - y64|| over the ACC cases at 2^20 samples: 0.99 (rrrf, 8 sections);
# the device path restarts every chunk from a rounded f64 state and drifts less than the sequential f32 path
TAU = 2e-7
ACC = [("tf", 3), ("tf", 5), ("tf", 7), ("sos", 1), ("sos", 4), ("sos", 8)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form,order", ACC)
def test_accuracy_2e20(ya, kind, form, order):
    rng = np.random.default_rng(300 + order + 10 * KINDS.index(kind) + (50 if form == "sos" else 0))
    n = 1 << 20
    if form == "tf":
        b, a = stable_tf(rng, kind, order)
        mk = lambda: ya.IirFilter(kind, b, a)
        y64 = iir64(kind, b, a, x := rand_samples(rng, kind, n), chunk=1024)
    else:
        b, a = stable_sos(rng, kind, order)
        mk = lambda: ya.IirFilter.new_sos(kind, b, a, order)
        y64 = iir64(kind, b, a, x := rand_samples(rng, kind, n), nsos=order, chunk=1024)
    y_dev = run_dev(ya, mk(), x)
    y_seq = run_host(mk(), x)
    e_dev, e_seq = np.linalg.norm(y_dev - y64), np.linalg.norm(y_seq - y64)
    bound = 2 * e_seq + TAU * np.linalg.norm(y64)
    print(f"{kind} {form}{order}: dev {e_dev / np.linalg.norm(y64):.3e} seq {e_seq / np.linalg.norm(y64):.3e} "
          f"ratio {e_dev / max(e_seq, 1e-300):.3f}")
    assert e_dev <= bound, (e_dev, e_seq)


@pytest.mark.parametrize("kind", ["crcf"])
def test_accuracy_2e24(ya, kind):
    rng = np.random.default_rng(400)
    n = 1 << 24
    b, a = stable_sos(rng, kind, 4)
    x = rand_samples(rng, kind, n)
    y64 = iir64(kind, b, a, x, nsos=4, chunk=4096)
    y = run_dev(ya, ya.IirFilter.new_sos(kind, b, a, 4), x)
    err = rel_l2(y, y64)
    print(f"2^24 crcf sos4 rel-L2 {err:.3e}")
    assert err < 2e-6


def test_integrator_long(ya):
    """the marginal filter (pole at z = 1) over 2^22 samples: the device path tracks the reference's own f32 path"""
    rng = np.random.default_rng(7)
    n = 1 << 22
    x = (rng.standard_normal(n) * 0.01).astype(np.float32)
    y = run_dev(ya, ya.IirFilter.new_integrator("rrrf"), x)
    y_seq = run_host(ya.IirFilter.new_integrator("rrrf"), x)
    err = rel_l2(y, y_seq)
    print(f"integrator 2^22: rel-L2 device vs host path {err:.3e}")
    assert err < 1e-4
