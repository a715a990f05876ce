"""Modem on the GPU against tests/modem_ref.py (the reference's arithmetic restated in numpy, pinned by
tests/test_modem_ref_cpu.py), fed with the library's OWN constellation and neighbour table, through the host-pointer and
the device-pointer entry points.  Everything but DPSK's x_hat is compared bit for bit and no sample is excluded after the
fact; where atan2f decides (PSK, DPSK) the inputs are BUILT at least 1e-4 rad from every decision boundary, about a
hundred times the few-ulp error allowed to atan2f, and Arb's inputs are selected BEFORE use so that the two nearest points
differ by >= 1e-4 in distance (the reference compares hypot(), the kernel squared distances).

DPSK x_hat = polar(1, theta - residual) carries the device's atan2f and sincosf: it is compared with the f64 evaluation
of the same formula, within 4x the restatement's own worst deviation from it on the same inputs (2 ulp each for the two
device routines); the figures are printed (DESIGN.md section 4 records a run)."""
import numpy as np
import pytest

import modem_ref as mr

pytestmark = pytest.mark.gpu
f32 = np.float32
TD, TM = 2048, 4096            # samples per workgroup: demodulating kernels, modulating kernels
LINEAR = ["Ask2", "Ask4", "Ask16", "Ask256", "Qam4", "Qam8", "Qam16", "Qam32", "Qam256", "Bpsk", "Qpsk", "Ook"]
PSKS = ["Psk2", "Psk4", "Psk8", "Psk256"]
DPSKS = ["Dpsk2", "Dpsk8", "Dpsk256"]


def sizes(T):
    return [0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T + 17]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def make(ya, name):
    m = ya.Modem(ya.ModulationScheme[name])
    kind, bps = mr.SCHEMES[name]
    D = mr.design(kind, bps)
    return m, D, m.get_constellation(), m.get_neighbours()


def dev_demod(ya, m, x, soft, bps, off=0, xhat=True):
    """the _dev entry points; symbol and soft pointers `off` bytes into their allocations"""
    n = x.size
    xd = ya.DeviceArray.from_numpy(np.concatenate([x, np.zeros(1, np.complex64)]))
    sd = ya.DeviceArray(n + 32, np.uint8)
    if soft:
        bd = ya.DeviceArray(n * bps + 32, np.uint8)
        m.demodulate_soft_block_devptr(xd, n, sd.ptr + off, bd.ptr + off)
        ya.synchronize()
        return sd.to_numpy()[off:off + n], None, bd.to_numpy()[off:off + n * bps].reshape(n, bps)
    hd = ya.DeviceArray(n + 1, np.complex64) if xhat else None
    m.demodulate_block_devptr(xd, n, sd.ptr + off, hd)
    ya.synchronize()
    return sd.to_numpy()[off:off + n], (hd.to_numpy()[:n] if xhat else None), None


def check_state(m, D, x, xh):
    r = mr.RefModem(D)
    r.r, r.x_hat = np.complex64(x), np.complex64(xh)
    assert bits(m.get_demodulator_sample()).tolist() == bits(xh).tolist()
    with np.errstate(over="ignore", invalid="ignore"):
        pe, evm = r.get_demodulator_phase_error(), r.get_demodulator_evm()
    assert np.array_equal(np.float32(m.get_demodulator_phase_error()).view(np.uint32), np.float32(pe).view(np.uint32))
    assert np.float32(m.get_demodulator_evm()).view(np.uint32) == np.float32(evm).view(np.uint32)


def sweep(ya, m, D, cmap, nbr, x, T, exact_xhat=True, theta=None):
    """every size, host and device paths, hard (+ xhat) and soft, against one reference run over the longest block"""
    nmax = 3 * T + 17
    assert x.size >= nmax
    want_s, want_xh, want_sb, _ = mr.block_demod(D, cmap, nbr, x[:nmax], f32(0), True, theta=theta)
    for n in sizes(T):
        xs = x[:n]
        for path in ("host", "dev1", "dev3", "dev8"):
            if path != "host" and n not in (17, T + 1, nmax):
                continue
            m.reset()
            if path == "host":
                s, xh = m.demodulate_block(xs, xhat=True)
            else:
                s, xh, _ = dev_demod(ya, m, xs, False, D.bps, int(path[3:]))
            assert np.array_equal(s, want_s[:n]), (n, path)
            if exact_xhat:
                assert np.array_equal(bits(xh), bits(want_xh[:n])), (n, path)
                if n:
                    check_state(m, D, xs[-1], want_xh[n - 1])
            m.reset()
            if path == "host":
                s, sb = m.demodulate_soft_block(xs)
            else:
                s, _, sb = dev_demod(ya, m, xs, True, D.bps, int(path[3:]))
            assert np.array_equal(s, want_s[:n]), (n, path, "soft")
            assert np.array_equal(sb, want_sb[:n]), (n, path, "soft")
            if exact_xhat and n:
                check_state(m, D, xs[-1], want_xh[n - 1])


# ---- constellations --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mr.SCHEMES))
def test_constellation_and_neighbours(ya, name):
    m, D, cmap, nbr = make(ya, name)
    assert m.get_bps() == D.bps and m.get_constellation_size() == D.M and m.get_scheme() == ya.ModulationScheme[name]
    c = cmap.astype(np.complex128)
    if D.kind in (mr.PSK, mr.DPSK):
        k = np.array([mr.gray_decode(i) if D.kind == mr.PSK else i for i in range(D.M)])
        assert np.abs(c - np.exp(2j * np.pi * k / D.M)).max() <= 2.0 ** -21
    else:
        assert np.array_equal(bits(cmap), bits(D.map))            # the restated integer formula, exactly
    assert nbr.shape == (D.M, D.p)
    for i in range(D.M if D.p else 0):
        d = np.abs(c - c[i])
        d[i] = np.inf
        assert i not in nbr[i] and len(set(nbr[i].tolist())) == D.p
        assert np.all(d[nbr[i].astype(int)] <= np.sort(d)[D.p - 1] * (1 + 1e-6))
    # per-sample calls: the reference's round trip (modem.rs:583-609, :821-854)
    for i in range(D.M):
        if D.kind == mr.DPSK:
            break
        y = m.modulate(i)
        assert bits(y).tolist() == bits(cmap[i]).tolist()
        s, soft = m.demodulate_soft(y)
        assert s == i and mr.pack_soft_bits(soft, D.bps) == i and m.demodulate(y) == i


def test_arb_table_is_balanced_and_scaled(ya):
    """within 4 ulp per component, the ulp being that of the component itself, of the f64 computation"""
    rng = np.random.default_rng(5)
    for M in (4, 16, 64, 256):
        t = (rng.standard_normal(M) + 1j * rng.standard_normal(M) + (0.3 - 0.2j)).astype(np.complex64)
        got = ya.Modem.from_table(t).get_constellation()
        t64 = t.astype(np.complex128)
        t64 = t64 - t64.mean()
        t64 = t64 / np.sqrt(np.mean(np.abs(t64) ** 2))
        for g, w in ((got.real, t64.real), (got.imag, t64.imag)):
            ulp = np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)
            worst = float(np.max(np.abs(g.astype(np.float64) - w) / ulp))
            print(f"arb M = {M}: worst component error {worst:.2f} ulp")
            assert worst <= 4.0


def test_unsupported_schemes_are_config_errors(ya):
    for name in mr.UNSUPPORTED + ["Arb", "Unknown"]:
        with pytest.raises(ya.ConfigError):
            ya.Modem(ya.ModulationScheme[name])
    for bad in (np.ones(3, np.complex64), np.ones(1, np.complex64), np.ones(512, np.complex64), np.zeros(4, np.complex64)):
        with pytest.raises(ya.ConfigError):
            ya.Modem.from_table(bad)


# ---- modulation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Ask2", "Qam8", "Psk256", "Bpsk", "Ook"])
def test_modulate_block(ya, name):
    m, D, cmap, _ = make(ya, name)
    rng = np.random.default_rng(11)
    sym = rng.integers(0, D.M, 3 * TM + 17 + 8).astype(np.uint8)
    for n in sizes(TM):
        assert np.array_equal(bits(m.modulate_block(sym[:n])), bits(cmap[sym[:n]])), n
        for off in (1, 3, 8):
            if n not in (17, TM + 1, 3 * TM + 17):
                continue
            sd = ya.DeviceArray.from_numpy(sym)
            yd = ya.DeviceArray(n + 1, np.complex64)
            m.modulate_block_devptr(sd.ptr + off, n, yd)
            assert np.array_equal(bits(yd.to_numpy()[:n]), bits(cmap[sym[off:off + n]])), (n, off)


def test_out_of_range_symbol_is_rejected_and_nothing_is_written(ya):
    m, D, cmap, _ = make(ya, "Qam16")
    n = 2 * TM + 5
    sym = np.zeros(n, np.uint8)
    sym[TM + 3] = 16
    y = np.full(n, 7 + 7j, np.complex64)
    with pytest.raises(ya.RangeError):
        m.modulate_block(sym, y)
    assert np.all(y == 7 + 7j)
    sd = ya.DeviceArray.from_numpy(sym)
    yd = ya.DeviceArray.from_numpy(y)
    with pytest.raises(ya.RangeError):
        m.modulate_block_devptr(sd, n, yd)
    assert np.array_equal(bits(yd.to_numpy()), bits(y))
    with pytest.raises(ya.RangeError):
        m.modulate(16)
    d, Dd, dmap, _ = make(ya, "Dpsk8")
    d.modulate_block(np.array([1, 2], np.uint8))
    sym[TM + 3] = 8
    sym[:TM] = 1
    with pytest.raises(ya.RangeError):
        d.modulate_block_devptr(ya.DeviceArray.from_numpy(sym), n, yd)
    assert np.array_equal(bits(yd.to_numpy()), bits(y))
    k = mr.dpsk_indices([1, 2, 5], 8)                                 # the failed call left the running index alone
    assert bits(d.modulate(5)).tolist() == bits(dmap[k[-1]]).tolist()


@pytest.mark.parametrize("name", DPSKS)
def test_dpsk_modulate_is_the_exact_running_index(ya, name):
    m, D, cmap, _ = make(ya, name)
    rng = np.random.default_rng(13)
    n = 3 * TM + 17
    sym = rng.integers(0, D.M, n).astype(np.uint8)
    k = mr.dpsk_indices(sym, D.M)
    assert np.array_equal(bits(m.modulate_block(sym)), bits(cmap[k]))
    # cut inside and at workgroup seams, mixed with per-sample calls, a clone in mid-stream, and reset
    m.reset()
    cuts = [0, 5, TM, TM + 1, TM + 2, 2 * TM - 1, 2 * TM + 600, n]
    got, other = [], None
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b - a == 1:
            got.append(np.array([m.modulate(int(sym[a]))], np.complex64))
        elif a == TM + 2:
            sd = ya.DeviceArray.from_numpy(sym[a:b])
            yd = ya.DeviceArray(b - a, np.complex64)
            m.modulate_block_devptr(sd, b - a, yd)
            got.append(yd.to_numpy())
            other = m.clone()
        else:
            got.append(m.modulate_block(sym[a:b]))
    assert np.array_equal(bits(np.concatenate(got)), bits(cmap[k]))
    a = cuts[-3]
    assert np.array_equal(bits(other.modulate_block(sym[a:])), bits(cmap[k[a:]]))
    m.reset()
    assert np.array_equal(bits(m.modulate_block(sym[:40])), bits(cmap[k[:40]]))
    # against the reference's sequential f32 phase (restated) and f64 truth, within the CPU test's printed bound
    r = mr.RefModem(D)
    nn = 600
    seq = np.array([r.modulate(int(s)) for s in sym[:nn]])
    y = cmap[k[:nn]].astype(np.complex128)
    truth = mr.dpsk_truth(sym[:nn], D.M)
    bound = mr.dpsk_drift_bound(nn, D.M)
    print(f"{name}: exact-index form vs truth {np.abs(y - truth).max():.3e}; vs the sequential f32 modulator "
          f"{np.abs(y - seq).max():.3e} (its bound at n = {nn}: {bound:.3e})")
    assert np.abs(y - truth).max() <= 2.0 ** -21
    assert np.abs(y - seq).max() <= bound


# ---- demodulation: the schemes decided by comparisons alone ---------------------------------------------------------
def linear_inputs(D, rng, n):
    x = (D.map[rng.integers(0, D.M, n)] + 0.25 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    a = D.alpha if D.kind in (mr.ASK, mr.QAM) else f32(1)
    thr = [f32(0), f32(-0.0), mr.FRAC_1_SQRT_2, -mr.FRAC_1_SQRT_2, mr.SQRT_2, f32(1e30), f32(-1e30), f32(3e38), f32(-3e38),
           f32(4.0), f32(-4.0)]
    for j in range(1, min(D.M, 64) + 1):
        thr += [f32(j) * a, -(f32(j) * a), np.nextafter(f32(j) * a, f32(9)), np.nextafter(f32(j) * a, f32(-9))]
    acc = f32(0)
    for k in range(D.bps):                                       # the sums of reference[k] as the loop forms them
        acc = acc + D.ref[k] if D.ref.size else acc
        thr += [acc, -acc]
    thr = np.array(thr, f32)
    special = np.concatenate([thr + 1j * rng.choice(thr, thr.size), rng.choice(thr, thr.size) + 1j * thr,
                              thr + 0j, 0.3 + 1j * thr]).astype(np.complex64)
    pos = rng.choice(n, special.size, replace=False)
    x[pos] = special
    x[n - 1] = special[3]
    return x


@pytest.mark.parametrize("name", LINEAR)
def test_linear_schemes_bit_for_bit(ya, name):
    m, D, cmap, nbr = make(ya, name)
    x = linear_inputs(D, np.random.default_rng(len(name) * 7 + D.bps), 3 * TD + 17)
    sweep(ya, m, D, cmap, nbr, x, TD)


# ---- PSK / DPSK: phases built away from the boundaries -------------------------------------------------------------
def phase_steps(D, rng, n):
    """n phases (PSK) or phase differences (DPSK), each a decision boundary + delta, 1e-4 <= |delta| <= half spacing"""
    half = np.pi / D.M
    b = (2 * rng.integers(0, D.M, n) + 1) * half
    delta = rng.uniform(1e-4, half - 1e-4, n) * rng.choice([-1.0, 1.0], n)
    delta[: n // 4] = 1e-4 * np.sign(delta[: n // 4])             # a quarter of them right at the allowed minimum
    return b + delta


@pytest.mark.parametrize("name", PSKS)
def test_psk_bit_for_bit(ya, name):
    m, D, cmap, nbr = make(ya, name)
    rng = np.random.default_rng(D.bps)
    n = 3 * TD + 17
    x = (rng.uniform(0.3, 2.0, n) * np.exp(1j * phase_steps(D, rng, n))).astype(np.complex64)
    sweep(ya, m, D, cmap, nbr, x, TD)


def dpsk_truth_xhat(D, x, phi0=0.0):
    th = np.angle(x.astype(np.complex128))
    prev = np.concatenate([[phi0], th[:-1]])
    d = th - prev - np.pi * (1.0 - 1.0 / D.M)
    d = np.where(d > np.pi, d - 2 * np.pi, np.where(d < -np.pi, d + 2 * np.pi, d))
    for k in range(D.bps):
        r = (2.0 ** (D.bps - k - 1)) * np.pi / D.M
        d = np.where(d > 0, d - r, d + r)
    return np.exp(1j * (th - d))


@pytest.mark.parametrize("name", DPSKS)
def test_dpsk_symbols_exact_and_xhat_within_bound(ya, name):
    m, D, cmap, nbr = make(ya, name)
    rng = np.random.default_rng(D.bps + 40)
    n = 3 * TD + 17
    theta = np.cumsum(phase_steps(D, rng, n))
    x = (rng.uniform(0.3, 2.0, n) * np.exp(1j * theta)).astype(np.complex64)
    sweep(ya, m, D, cmap, nbr, x, TD, exact_xhat=False)
    want_s, want_xh, _, _ = mr.block_demod(D, cmap, nbr, x, f32(0), False)
    truth = dpsk_truth_xhat(D, x)
    own = np.abs(want_xh.astype(np.complex128) - truth).max()
    bound = 4 * own
    # blocks cut inside and at workgroup seams, per-sample calls between them, a clone in mid-stream
    m.reset()
    cuts = [0, 7, TD, TD + 1, TD + 2, 2 * TD - 1, 2 * TD + 300, n]
    s_got, xh_got, other = [], [], None
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b - a == 1:
            s_got.append(np.array([m.demodulate(x[a])], np.uint8))
            xh_got.append(np.array([m.get_demodulator_sample()], np.complex64))
        elif a == TD + 2:
            s, xh, _ = dev_demod(ya, m, x[a:b], False, D.bps, 3)
            s_got.append(s)
            xh_got.append(xh)
            other = m.clone()
        else:
            s, xh = m.demodulate_block(x[a:b], xhat=True)
            s_got.append(s)
            xh_got.append(xh)
    assert np.array_equal(np.concatenate(s_got), want_s)
    dev = np.abs(np.concatenate(xh_got).astype(np.complex128) - truth).max()
    print(f"{name}: x_hat vs f64 truth: device {dev:.3e}, restatement {own:.3e}, bound {bound:.3e}")
    assert dev <= bound
    assert abs(complex(m.get_demodulator_sample()) - truth[-1]) <= bound
    a = cuts[-3]
    s, sb = other.demodulate_soft_block(x[a:])
    assert np.array_equal(s, want_s[a:]) and np.array_equal(sb, np.stack([mr.unpack_soft_bits(int(v), D.bps) for v in s]))
    m.reset()                                                      # after reset the first difference is against phi = 0
    assert np.array_equal(m.demodulate_block(x[:50]), want_s[:50])


# ---- Arb -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [4, 16, 64, 256])
def test_arb_bit_for_bit_with_the_soft_quirk(ya, M):
    rng = np.random.default_rng(M)
    bps = M.bit_length() - 1
    t = (rng.standard_normal(M) + 1j * rng.standard_normal(M)).astype(np.complex64)
    m = ya.Modem.from_table(t)
    cmap = m.get_constellation()
    D = mr.design(mr.ARB, bps, t)
    assert m.get_scheme() == ya.ModulationScheme.Arb and m.get_neighbours().shape == (M, 0)
    n = 3 * TD + 17
    draw = int(n * 1.005) + 8
    x = (cmap[rng.integers(0, M, draw)] + 0.35 * (rng.standard_normal(draw) + 1j * rng.standard_normal(draw))).astype(np.complex64)
    d = np.sort(np.abs(x.astype(np.complex128)[:, None] - cmap.astype(np.complex128)[None, :]), 1)
    keep = d[:, 1] - d[:, 0] >= 1e-4
    assert keep.mean() >= 0.99, keep.mean()                      # selected BEFORE use; nothing is excluded afterwards
    x = x[keep]
    assert x.size >= n
    x = x[:n]
    sweep(ya, m, D, cmap, np.zeros((M, 0), np.uint8), x, TD)
    # the quirk is really there: the "fixed" loop (bit of the candidate index) gives other soft bytes
    _, _, sb_q, _ = mr.block_demod(D, cmap, np.zeros((M, 0), np.uint8), x[:400], f32(0), True)
    _, _, sb_f, _ = mr.block_demod(D, cmap, np.zeros((M, 0), np.uint8), x[:400], f32(0), True, fixed=True)
    differ = np.flatnonzero(np.any(sb_q != sb_f, 1))
    assert differ.size > 0
    i = int(differ[0])
    s, sb = m.demodulate_soft(x[i])
    assert np.array_equal(sb, sb_q[i]) and not np.array_equal(sb, sb_f[i])
    _, sbb = m.demodulate_soft_block(x[:400])
    assert np.array_equal(sbb[i], sb_q[i])


def test_python_helpers(ya):
    for s in range(256):
        assert ya.gray_decode(ya.gray_encode(s)) == s == mr.gray_decode(mr.gray_encode(s))
        assert ya.gray_encode(s) == mr.gray_encode(s) and ya.gray_decode(s) == mr.gray_decode(s)
    for bps in (1, 3, 8):
        for s in range(1 << bps):
            assert ya.pack_soft_bits(ya.unpack_soft_bits(s, bps), bps) == s
