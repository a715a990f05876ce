"""Pins tests/modem_ref.py -- the numpy restatement of the reference's Modem that the GPU tests compare against -- with the
reference's own tests (src/modem/modem.rs: mod/demod round trip :583-609, soft demodulation :821-854, demodulator
statistics :1066-1139, copy :1351-1384) for every scheme the library builds, and checks the helpers and the tables."""
import numpy as np
import pytest

import modem_ref as mr

f32 = np.float32
NAMES = sorted(mr.SCHEMES)


def _pair(name):
    kind, bps = mr.SCHEMES[name]
    D = mr.design(kind, bps)
    return D, mr.RefModem(D), mr.RefModem(D)


@pytest.mark.parametrize("name", NAMES)
def test_mod_demod_round_trip(name):
    D, mod, dem = _pair(name)
    e = 0.0
    for i in range(D.M):
        x = mod.modulate(i)
        assert dem.demodulate(x) == i
        assert abs(dem.get_demodulator_phase_error()) <= 1e-3
        assert abs(dem.get_demodulator_evm()) <= 1e-3
        e += float(abs(x)) ** 2
    assert abs(np.sqrt(e / D.M) - 1.0) <= 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_soft_demodulation_packs_to_the_hard_symbol(name):
    D, mod, dem = _pair(name)
    for i in range(D.M):
        x = mod.modulate(i)
        s, soft = dem.demodulate_soft(x)
        assert s == i
        assert soft.size == D.bps and mr.pack_soft_bits(soft, D.bps) == i
        assert abs(dem.get_demodulator_phase_error()) <= 1e-3
        assert abs(dem.get_demodulator_evm()) <= 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_demodulator_statistics(name):
    D, mod, dem = _pair(name)
    for sign in (1.0, -1.0):
        rot = np.complex64(complex(f32(np.cos(f32(0.01))), f32(sign) * f32(np.sin(f32(0.01)))))
        for i in range(D.M):
            mod.reset()
            dem.reset()
            x = mod.modulate(i)
            if abs(x) < 1e-3:
                continue
            assert dem.demodulate(np.complex64(x * rot)) == i
            assert sign * dem.get_demodulator_phase_error() > 0.0


@pytest.mark.parametrize("name", NAMES)
def test_copy_continues_identically(name):
    D, m0, _ = _pair(name)
    rng = np.random.default_rng(7)
    for _ in range(10):
        m0.modulate(int(rng.integers(D.M)))
        m0.demodulate(np.complex64(complex(rng.standard_normal(), rng.standard_normal())))
    m1 = m0.copy()
    for _ in range(10):
        s = int(rng.integers(D.M))
        assert m0.modulate(s) == m1.modulate(s)
        x = np.complex64(complex(rng.standard_normal(), rng.standard_normal()))
        assert m0.demodulate(x) == m1.demodulate(x)
        assert m0.get_demodulator_sample() == m1.get_demodulator_sample()


def test_arb_round_trip_and_soft():
    rng = np.random.default_rng(3)
    for bps in (2, 4, 6):
        t = (rng.standard_normal(1 << bps) + 1j * rng.standard_normal(1 << bps)).astype(np.complex64)
        D = mr.design(mr.ARB, bps, t)
        assert abs(np.mean(D.map)) < 1e-6 and abs(np.mean(np.abs(D.map) ** 2) - 1.0) < 1e-5
        m = mr.RefModem(D)
        for i in range(D.M):
            assert m.demodulate(m.modulate(i)) == i
            s, soft = m.demodulate_soft(m.modulate(i))
            assert s == i and soft.size == bps


def test_gray_and_soft_bit_helpers():
    for s in range(256):
        assert mr.gray_decode(mr.gray_encode(s)) == s and mr.gray_encode(mr.gray_decode(s)) == s
        assert bin(mr.gray_encode(s) ^ mr.gray_encode((s + 1) & 255)).count("1") == 1
    for bps in range(1, 9):
        for s in range(1 << bps):
            soft = mr.unpack_soft_bits(s, bps)
            assert soft.size == bps and set(soft.tolist()) <= {0, 255}
            assert mr.pack_soft_bits(soft, bps) == s
    assert mr.pack_soft_bits([127, 128], 2) == 1               # the erasure value counts as 0
    assert [mr.soft_byte(v) for v in (-1.0, -0.0, 0.9, 254.99, 255.0, 1e9, np.nan, np.inf, -np.inf)] == \
        [0, 0, 0, 254, 255, 255, 0, 255, 0]


@pytest.mark.parametrize("name", [n for n in NAMES if mr.design(*mr.SCHEMES[n]).p])
def test_neighbour_tables_hold_the_nearest_points(name):
    """for each symbol the p nearest OTHER points by f64 distance; a tie at the cut may resolve either way"""
    D = mr.design(*mr.SCHEMES[name])
    c = D.map.astype(np.complex128)
    assert D.nbr.shape == (D.M, D.p)
    for i in range(D.M):
        d = np.abs(c - c[i])
        d[i] = np.inf
        row = D.nbr[i].astype(int)
        assert i not in row and len(set(row.tolist())) == D.p
        cut = np.sort(d)[D.p - 1]
        assert np.all(d[row] <= cut * (1 + 1e-6)), (name, i)


@pytest.mark.parametrize("bps", [1, 3, 8])
def test_sequential_dpsk_modulator_stays_within_its_drift_bound(bps):
    """the reference's f32 phase accumulator against f64 truth: the bound grows with n (printed: the GPU test uses it)"""
    D = mr.design(mr.DPSK, bps)
    m = mr.RefModem(D)
    rng = np.random.default_rng(bps)
    n = 600
    sym = rng.integers(0, D.M, n)
    y = np.array([m.modulate(int(s)) for s in sym])
    truth = mr.dpsk_truth(sym, D.M)
    err = np.abs(y.astype(np.complex128) - truth)
    for cut in (10, 100, n):
        bound = mr.dpsk_drift_bound(cut, D.M)
        print(f"dpsk{D.M}: n = {cut}: bound {bound:.3e}, worst deviation of the sequential f32 modulator {err[:cut].max():.3e}")
        assert err[:cut].max() <= bound
    # the library's form: the exact index; its only error is the table's
    k = mr.dpsk_indices(sym, D.M)
    assert np.abs(D.map[k].astype(np.complex128) - truth).max() <= 2.0 ** -21


@pytest.mark.parametrize("name", NAMES + ["Arb4", "Arb32"])
def test_array_form_equals_the_per_sample_form(name):
    rng = np.random.default_rng(len(name))
    if name.startswith("Arb"):
        bps = int(name[3:]).bit_length() - 1
        D = mr.design(mr.ARB, bps, (rng.standard_normal(1 << bps) + 1j * rng.standard_normal(1 << bps)).astype(np.complex64))
    else:
        D = mr.design(*mr.SCHEMES[name])
    n = 150
    x = (D.map[rng.integers(0, D.M, n)] + 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    x[:4] = [0, complex(-0.0, 0.0), 1e30, complex(-1e30, 1e30)]
    for soft in (False, True):
        m = mr.RefModem(D)
        m.phi = f32(0.3)
        with np.errstate(over="ignore", invalid="ignore"):
            want = [m.demodulate_soft(v) + (m.x_hat,) if soft else (m.demodulate(v), None, m.x_hat) for v in x]
        s, xh, sb, phi = mr.block_demod(D, D.map, D.nbr, x, f32(0.3), soft)
        assert np.array_equal(s, [w[0] for w in want])
        assert np.array_equal(xh.view(np.uint32), np.array([w[2] for w in want], np.complex64).view(np.uint32))
        if soft:
            assert np.array_equal(sb, np.array([w[1] for w in want]))
        if D.kind == mr.DPSK:
            assert phi == m.phi
