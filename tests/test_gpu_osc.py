"""Osc (src/nco/osc.rs) through the C ABI and osc_kernels.hip, against the restatement in tests/osc_ref.py: every
per-sample call and every block output word bit for bit, the carried phase word exactly, and the reference's own PLL
and spectrum tests at their tolerances."""
import numpy as np
import pytest

from osc_ref import (MASK, PI, TWO_PI, OscRef, constrain, f32, hann, mix_block_torch, phase_error, pll_error,
                     validate_psd_spgramcf)

pytestmark = pytest.mark.gpu

SCHEMES = [0, 1]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    if yagi_amd.device_count() < 1:
        pytest.fail("no GPU visible")
    return yagi_amd


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def make(ya, scheme):
    return ya.Osc(ya.OscScheme(scheme))


def samples(rng, n):
    """random complex64 with +-0, subnormals and a few large values mixed in"""
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    if n >= 8:
        special = np.array([0.0, -0.0, 1e-40, -3e-42, 1.17e-38, -1e-45, 3e38, -2.5e-39], np.float32)
        k = max(1, n // 16)
        idx = rng.integers(0, n, k)
        x.real[idx] = special[rng.integers(0, 8, k)]
        idx = rng.integers(0, n, k)
        x.imag[idx] = special[rng.integers(0, 8, k)]
    return x


def freq_for(word):
    """the f32 frequency whose constrain() is nearest to `word` (exact where an f32 reaches it)"""
    x = f32(float(word) / 2 ** 32 * float(TWO_PI))
    best = x
    for _ in range(64):
        w = constrain(x)
        if abs(w - word) < abs(constrain(best) - word):
            best = x
        if w == word:
            break
        x = np.nextafter(x, f32(np.inf) if w < word else f32(-np.inf))
    return best


# d_theta words: 0, 1, 2^31, u32::MAX, the adversarial strides of 16, 32, 64 and 512 table entries per sample, and an
# ordinary frequency
WORDS = [0, 1, 1 << 31, MASK, 16 << 22, 32 << 22, 64 << 22, 512 << 22, constrain(0.1234 * 2 * np.pi)]


def set_word(q, ref, word):
    f = -1e-9 if word == MASK else freq_for(word)
    q.set_frequency(f)
    ref.set_frequency(f)
    assert q.get_state()[1] == ref.d_theta
    assert abs(ref.d_theta - word) < 64 and (word not in (0, 1, 1 << 31, MASK) or ref.d_theta == word)
    return ref.d_theta


# ---- per-sample calls ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_per_sample_calls_match_bit_for_bit(ya, scheme):
    q, r = make(ya, scheme), OscRef(scheme)
    rng = np.random.default_rng(11 + scheme)
    ops = [("set_frequency", 0.3), ("set_phase", 99.0), ("adjust_phase", -PI), ("adjust_frequency", -0.123),
           ("set_phase", float(np.nextafter(TWO_PI, f32(0)))), ("adjust_phase", float(TWO_PI)),
           ("set_frequency", -float(PI)), ("adjust_frequency", 1e-5), ("set_phase", -1e-9), ("set_phase", float("nan"))]
    ops += [(rng.choice(["set_frequency", "adjust_frequency", "set_phase", "adjust_phase"]),
             float(rng.uniform(-20, 20))) for _ in range(40)]
    for name, v in ops:
        getattr(q, name)(v)
        getattr(r, name)(v)
        for _ in range(int(rng.integers(0, 5))):
            q.step()
            r.step()
        assert q.get_state() == (r.theta, r.d_theta), (name, v)
        s, c = q.sin_cos()
        rs, rc = r.sin_cos()
        assert (s.view(np.uint32), c.view(np.uint32)) == (rs.view(np.uint32), rc.view(np.uint32))
        assert q.sin().view(np.uint32) == rs.view(np.uint32) and q.cos().view(np.uint32) == rc.view(np.uint32)
        assert bits([q.cexp()]).tolist() == bits([r.cexp()]).tolist()
        assert q.get_phase().view(np.uint32) == f32(r.get_phase()).view(np.uint32)
        assert q.get_frequency().view(np.uint32) == f32(r.get_frequency()).view(np.uint32)
        x = samples(rng, 1)[0]
        assert bits([q.mix_up(x)]).tolist() == bits([r.mix_up(x)]).tolist()
        assert bits([q.mix_down(x)]).tolist() == bits([r.mix_down(x)]).tolist()


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("kind,bw", [("phase", 0.1), ("phase", 0.01), ("freq", 0.1), ("freq", 0.02)])
def test_pll_loops_match_and_lock(ya, scheme, kind, bw):           # osc.rs:229-312
    offsets = [-PI / f32(1.1), -PI / f32(4.0), PI / f32(8.0), PI / f32(2.0)] if kind == "phase" else [-0.8, -0.1, 0.2, 0.4]
    for off in offsets:
        tx, rx = make(ya, scheme), make(ya, scheme)
        rtx, rrx = OscRef(scheme), OscRef(scheme)
        for o, ro in ((tx, rtx),):
            if kind == "phase":
                o.set_phase(off); ro.set_phase(off)
                o.set_frequency(0.0); ro.set_frequency(0.0)
            else:
                o.set_phase(0.0); ro.set_phase(0.0)
                o.set_frequency(off); ro.set_frequency(off)
        rx.pll_set_bandwidth(bw)
        rrx.pll_set_bandwidth(bw)
        for _ in range(int(f32(32.0) / f32(bw))):
            e = phase_error(tx.cexp(), rx.cexp())
            assert e.view(np.uint32) == phase_error(rtx.cexp(), rrx.cexp()).view(np.uint32)
            rx.pll_step(e); rrx.pll_step(e)
            tx.step(); rtx.step()
            rx.step(); rrx.step()
        assert rx.get_state() == (rrx.theta, rrx.d_theta) and tx.get_state() == (rtx.theta, rtx.d_theta)
        assert abs(pll_error(tx.get_phase(), rx.get_phase())) < 1e-2
        assert abs(pll_error(tx.get_frequency(), rx.get_frequency())) < 1e-2


# ---- device blocks -------------------------------------------------------------------------------------------------
def run_dev(torch, q, x, down):
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty_like(xd)
    (q.mix_block_down_dev if down else q.mix_block_up_dev)(xd, x.size, yd)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("down", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, (1 << 20) + 3])
def test_device_blocks_bit_exact(ya, torch, scheme, down, n):
    rng = np.random.default_rng(n * 4 + scheme * 2 + down)
    x = samples(rng, n)
    for word in WORDS:
        q, r = make(ya, scheme), OscRef(scheme)
        q.set_phase(1.234)
        r.set_phase(1.234)
        word = set_word(q, r, word)
        th0 = r.theta
        y = run_dev(torch, q, x, down)
        want = r.mix_block(x, down)
        bad = np.flatnonzero((bits(y) != bits(want)).reshape(-1, 2).any(axis=1))
        assert bad.size == 0, (word, bad[:5], y[bad[:3]], want[bad[:3]])
        assert q.get_state() == (r.theta, word) == ((th0 + n * word) & MASK, word)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("word", [32 << 22, MASK, WORDS[-1]])
def test_device_blocks_bit_exact_2p26(ya, torch, scheme, word):
    n = 1 << 26
    g = torch.Generator(device="cuda").manual_seed(5 + scheme)
    xd = torch.randn(n, dtype=torch.complex64, device="cuda", generator=g)
    xd[::977] = 0
    xd[1::1013] = -0.0
    yd = torch.empty_like(xd)
    for down in (False, True):
        q, r = make(ya, scheme), OscRef(scheme)
        q.set_phase(-2.0)
        r.set_phase(-2.0)
        w = set_word(q, r, word)
        (q.mix_block_down_dev if down else q.mix_block_up_dev)(xd, n, yd)
        want = mix_block_torch(scheme, r.theta, w, xd, down)
        torch.cuda.synchronize()
        same = torch.equal(torch.view_as_real(yd).view(torch.int32), torch.view_as_real(want).view(torch.int32))
        assert same, (scheme, word, down)
        assert q.get_state() == ((r.theta + n * w) & MASK, w)
        del want


@pytest.mark.parametrize("scheme", SCHEMES)
def test_stream_in_pieces_equals_one_call(ya, torch, scheme):
    rng = np.random.default_rng(3 + scheme)
    n = 3 * (1 << 22) + 12345
    x = samples(rng, n)
    xd = torch.from_numpy(x).cuda()
    whole = torch.empty_like(xd)
    q = make(ya, scheme)
    q.set_phase(0.5)
    q.set_frequency(0.1234)
    th0, word = q.get_state()
    p = q.clone()
    q.mix_block_up_dev(xd, n, whole)
    assert q.get_state() == ((th0 + n * word) & MASK, word)
    cut_sets = [list(range(0, 7 * 3000, 7)) + [n],                     # pieces of 7, then the rest
                sorted(set(rng.integers(1, n, 40).tolist())) + [n],   # random cuts (8-byte aligned starts)
                list(range(0, n, 1 << 22)) + [n]]                      # 2^22-sample calls
    for cuts in cut_sets:
        r = p.clone()
        out = torch.empty_like(xd)
        a = 0
        for b in cuts:
            if b <= a:
                continue
            r.mix_block_up_dev(xd[a:], b - a, out[a:])
            assert r.get_state() == ((th0 + b * word) & MASK, word)
            a = b
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(out).view(torch.int32), torch.view_as_real(whole).view(torch.int32))
    torch.cuda.synchronize()
    want = OscRef(scheme)
    want.theta, want.d_theta = th0, word
    assert np.array_equal(bits(whole.cpu().numpy()), bits(want.mix_block_up(x)))


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("down", [False, True])
def test_in_place_equals_out_of_place(ya, torch, scheme, down):
    rng = np.random.default_rng(21)
    n = (1 << 18) + 5
    x = torch.from_numpy(samples(rng, n)).cuda()
    for off in (0, 1):                                                 # 16-byte and 8-byte aligned
        q = make(ya, scheme)
        q.set_frequency(32 * 2 * float(PI) / 1024)
        q2 = q.clone()
        y = torch.empty_like(x)
        fn = (lambda o: o.mix_block_down_dev) if down else (lambda o: o.mix_block_up_dev)
        fn(q)(x[off:], n - off, y[off:])
        z = x.clone()
        fn(q2)(z[off:], n - off, z[off:])
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(y[off:]).view(torch.int32), torch.view_as_real(z[off:]).view(torch.int32))
        assert q.get_state() == q2.get_state()


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n", [1, 100, 4096, 4097, 50000])
def test_host_slices_equal_device_calls(ya, torch, scheme, n):
    rng = np.random.default_rng(n)
    x = samples(rng, n)
    for down in (False, True):
        q = make(ya, scheme)
        q.set_phase(2.5)
        q.set_frequency(-0.7)
        d = q.clone()
        yh = q.mix_block_down(x) if down else q.mix_block_up(x)
        yd = run_dev(torch, d, x, down)
        assert np.array_equal(bits(yh), bits(yd)) and q.get_state() == d.get_state()


@pytest.mark.parametrize("scheme", SCHEMES)
def test_per_sample_continues_after_device_block(ya, torch, scheme):
    rng = np.random.default_rng(9)
    x = samples(rng, 10000)
    q, r = make(ya, scheme), OscRef(scheme)
    for o in (q, r):
        o.set_phase(0.25)
        o.set_frequency(0.9)
    y = run_dev(torch, q, x[:9000], False)
    assert np.array_equal(bits(y), bits(r.mix_block_up(x[:9000])))
    for i in range(9000, 9100):
        assert bits([q.mix_down(x[i])]).tolist() == bits([r.mix_down(x[i])]).tolist()
        q.step()
        r.step()
    y = run_dev(torch, q, x[9100:], True)
    assert np.array_equal(bits(y), bits(r.mix_block_down(x[9100:])))
    assert q.get_state() == (r.theta, r.d_theta)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_clone_is_independent_and_reset(ya, torch, scheme):
    q = make(ya, scheme)
    q.set_phase(1.0)
    q.set_frequency(0.2)
    q.pll_set_bandwidth(0.01)
    c = q.clone()
    assert c.get_state() == q.get_state()
    x = samples(np.random.default_rng(1), 5000)
    run_dev(torch, q, x, False)
    q.pll_step(0.3)
    assert c.get_state() != q.get_state()
    r = OscRef(scheme)
    r.set_phase(1.0)
    r.set_frequency(0.2)
    r.pll_set_bandwidth(0.01)
    assert np.array_equal(bits(run_dev(torch, c, x, True)), bits(r.mix_block_down(x)))
    c.pll_step(0.3)                                                    # the clone kept the PLL gains
    r.pll_step(0.3)
    assert c.get_state() == (r.theta, r.d_theta)
    q.reset()
    assert q.get_state() == (0, 0)
    y = q.mix_block_up(x[:10])
    assert np.array_equal(bits(y), bits(OscRef(scheme).mix_block_up(x[:10])))


def test_errors(ya, torch):
    q = make(ya, 0)
    with pytest.raises(ya.RangeError):
        q.mix_block_up(np.zeros(5, np.complex64), np.zeros(4, np.complex64))
    with pytest.raises(ya.RangeError):
        q.mix_block_down(np.zeros(5, np.complex64), np.zeros(6, np.complex64))
    with pytest.raises(ya.ConfigError):
        q.pll_set_bandwidth(-0.1)
    with pytest.raises(ya.ConfigError):
        q.set_frequency(float("inf"))
    with pytest.raises(ya.ConfigError):
        q.adjust_phase(-3e8)
    x = torch.zeros(100, dtype=torch.complex64, device="cuda")
    with pytest.raises(ya.ConfigError):
        q.mix_block_up_dev(x, 50, x[10:])                              # partial overlap
    import ctypes
    h = ctypes.c_void_p()
    assert ya.lib.yagi_hip_osc_create(5, ctypes.byref(h)) == 2 and not h.value      # unknown scheme: YAGI_ERR_CONFIG
    assert q.get_state() == (0, 0)
    q.mix_block_up_dev(x, 0, x)                                        # n = 0 is a no-op
    q.mix_block_up(np.zeros(0, np.complex64))


# ---- the reference's spectrum tests (osc.rs:648-743) through Osc and Spgram ----------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("freq", [0.0, 0.1234, -0.1234, 0.25, 0.1])
def test_nco_crcf_spectrum(ya, scheme, freq):
    num_samples, nfft = 1 << 16, 9600
    q = make(ya, scheme)
    q.set_frequency(f32(2.0) * PI * f32(freq))
    buf_len = 3 * nfft
    buf0 = np.full(buf_len, complex(f32(1.0) / np.sqrt(f32(nfft), dtype=f32), 0.0), np.complex64)
    w = np.array([hann(i, 2 * buf_len) for i in range(buf_len)], np.float32)
    psd = ya.Spgram(nfft, ya.WindowType.BlackmanHarris, nfft, nfft // 2)
    while psd.get_num_samples_total() < num_samples:
        buf1 = q.mix_block_up(buf0)
        if psd.get_num_samples_total() == 0:
            buf1 = (buf1.real * w + 1j * (buf1.imag * w)).astype(np.complex64)
        psd.write(buf1)
    f = float(f32(freq))
    regions = [(-0.5, f - 0.002, 0.0, -60.0, False, True), (f - 0.002, f + 0.002, 0.0, 0.0, False, True),
               (f + 0.002, 0.5, 0.0, -60.0, False, True)]
    assert validate_psd_spgramcf(psd, regions)
