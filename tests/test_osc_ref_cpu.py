"""tests/osc_ref.py (the restatement the GPU tests compare Osc against bit for bit) pinned to the reference's own Osc
tests (src/nco/osc.rs:216-798) at their own tolerances, and to constrain()'s edge cases.  Runs without a GPU."""
import numpy as np
import pytest

from osc_ref import (MASK, NCO_TAB, PI, TWO_PI, VCO_S, VCO_V, OscRef, constrain, cosf, f32, hann, phase_error,
                     pll_error, sin_cos_words, sinf, validate_psd_spectrum)

NCO, VCO = 0, 1


def test_tables_follow_the_reference_construction():
    # nco.rs:24: sin(2 pi i / 1024); the quarter-turn entries are the libm values of the exact f32 arguments
    assert NCO_TAB[0] == 0.0 and NCO_TAB[256] == 1.0
    assert np.max(np.abs(NCO_TAB - np.sin(2 * np.pi * np.arange(1024) / 1024))) < 1e-6
    # vco.rs:54-74: value 1 at pi/2, -1 at 3pi/2, odd symmetry about pi, even about pi/2 (mirrored values)
    assert VCO_V[256] == 1.0 and VCO_V[768] == -1.0
    assert np.array_equal(VCO_V[512:768], -VCO_V[0:256]) and np.array_equal(VCO_V[257:512], VCO_V[255:0:-1])
    assert np.array_equal(VCO_S[257:512], -VCO_S[254::-1]) and np.array_equal(VCO_S[769:], VCO_S[254::-1])
    # the interpolated VCO is within 1e-5 of sin over a full turn
    th = np.arange(0, 1 << 32, 4099, dtype=np.int64)
    s, c = sin_cos_words(True, th)
    assert np.max(np.abs(s - np.sin(th * 2 * np.pi / 2 ** 32))) < 1e-5
    assert np.max(np.abs(c - np.cos(th * 2 * np.pi / 2 ** 32))) < 1e-5


PHASE_CASES = [(-6.283185307, 1.000000000, 0.000000000), (-6.195739393, 0.996179042, 0.087334510),
               (-5.951041106, 0.945345356, 0.326070787), (-5.131745978, 0.407173250, 0.913350943),
               (-4.748043551, 0.035647016, 0.999364443), (-3.041191113, -0.994963998, -0.100232943),
               (-1.947799864, -0.368136099, -0.929771914), (-1.143752030, 0.414182352, -0.910193924),
               (-1.029377689, 0.515352252, -0.856978446), (-0.174356887, 0.984838307, -0.173474811),
               (-0.114520496, 0.993449692, -0.114270338), (0.000000000, 1.000000000, 0.000000000),
               (1.436080000, 0.134309213, 0.990939471), (2.016119855, -0.430749878, 0.902471353),
               (2.996498473, -0.989492293, 0.144585621), (3.403689755, -0.965848729, -0.259106603),
               (3.591162483, -0.900634128, -0.434578148), (5.111428476, 0.388533479, -0.921434607),
               (5.727585681, 0.849584319, -0.527452828), (6.283185307, 1.000000000, -0.000000000)]


def test_nco_crcf_phase():                                    # osc.rs:345-369
    for th, ec, es in PHASE_CASES:
        q = OscRef(NCO)
        q.set_phase(th)
        assert abs(q.cos() - ec) < 0.02 and abs(q.sin() - es) < 0.02, th


def test_nco_basic():                                         # osc.rs:373-414
    q = OscRef(NCO)
    tol, f = 1e-4, f32(2.0) * PI / f32(64.0)
    q.set_phase(0.0)
    assert abs(q.cos() - 1) < tol and abs(q.sin()) < tol
    q.set_phase(PI / f32(2.0))
    assert abs(q.cos()) < tol and abs(q.sin() - 1) < tol
    for mult in (f32(1.0), f32(2.0)):
        q.set_phase(0.0)
        q.set_frequency(mult * f)
        for i in range(128):
            s, c = q.sin_cos()
            ph = f32(i) * mult * f if mult != 1 else f32(i) * f
            assert abs(s - sinf(ph)) < tol and abs(c - cosf(ph)) < tol, (mult, i)
            q.step()


def test_nco_mixing():                                        # osc.rs:418-446
    q = OscRef(NCO)
    q.set_frequency(0.1)
    q.set_phase(PI)
    for _ in range(64):
        s, c = q.sin_cos()
        y = q.mix_down(np.complex64(complex(c, s)))
        assert abs(y.real - 1) < 0.05 and abs(y.imag) < 0.05
        q.step()


def test_nco_block_mixing_in_pieces_of_7():                   # osc.rs:450-488
    f, phi, n = f32(0.1), PI, 1024
    x = np.array([complex(cosf(f * f32(i) + phi), sinf(f * f32(i) + phi)) for i in range(n)], np.complex64)
    q = OscRef(NCO)
    q.set_frequency(f)
    q.set_phase(phi)
    y = np.concatenate([q.mix_block_down(x[i:i + 7]) for i in range(0, n, 7)])
    assert np.all(np.abs(y.real - 1) < 0.05) and np.all(np.abs(y.imag) < 0.05)
    # pieces or one block: the same bits and the same phase word
    r = OscRef(NCO)
    r.set_frequency(f)
    r.set_phase(phi)
    assert np.array_equal(r.mix_block_down(x).view(np.uint32), y.view(np.uint32)) and r.theta == q.theta


MIX_CASES = [(0.0, 0.0), (1.234, 0.0), (-1.234, 0.0), (99.0, 0.0), (float(PI), 0.0), (0.0, float(PI)),
             (0.0, -float(PI)), (0.0, 0.123), (0.0, -0.123), (0.0, 1e-5)]


@pytest.mark.parametrize("scheme", [NCO, VCO])
@pytest.mark.parametrize("phase,freq", MIX_CASES)
def test_nco_crcf_mix(scheme, phase, freq):                   # osc.rs:490-645 (20 cases)
    rng = np.random.default_rng(7)
    n = 1200
    ang = (f32(2.0) * PI * rng.random(n, dtype=np.float32)).astype(f32)
    x = np.array([complex(cosf(a), sinf(a)) for a in ang], np.complex64)
    q = OscRef(scheme)
    q.set_phase(phase)
    q.set_frequency(freq)
    y = q.mix_block_up(x)
    th = f32(phase)
    for i in range(n):
        e = np.complex64(complex(cosf(th), sinf(th)))
        v = np.complex64(x[i] * e)
        assert abs(y[i].real - v.real) < 1e-2 and abs(y[i].imag - v.imag) < 1e-2, i
        th = f32(th + f32(freq))
        while th > PI:
            th = f32(th - TWO_PI)
        while th < -PI:
            th = f32(th + TWO_PI)


def test_nco_crcf_frequency():                                # osc.rs:770-798
    for k in (2, 3, 5, 7):
        f = f32(1.0) / np.sqrt(f32(k), dtype=f32)
        q = OscRef(NCO)
        q.set_phase(0.0)
        q.set_frequency(f)
        for i in range(256):
            ph = f32(i) * f
            y = q.cexp()
            assert abs(y.real - cosf(ph)) < 0.04 and abs(y.imag - sinf(ph)) < 0.04, (k, i)
            q.step()


def pll_run(scheme, phase_offset, freq_offset, bw, n):        # osc.rs:229-268
    tx, rx = OscRef(scheme), OscRef(scheme)
    tx.set_phase(phase_offset)
    tx.set_frequency(freq_offset)
    rx.pll_set_bandwidth(bw)
    for _ in range(n):
        rx.pll_step(phase_error(tx.cexp(), rx.cexp()))
        tx.step()
        rx.step()
    return pll_error(tx.get_phase(), rx.get_phase()), pll_error(tx.get_frequency(), rx.get_frequency())


# the reference also runs bandwidth 1e-4 (320 000 steps per case); that loop is the same code for longer, and too slow
# in Python to run here
@pytest.mark.parametrize("bw", [0.1, 0.01, 0.001])
def test_nco_crcf_pll_phase(bw):                              # osc.rs:272-290
    for off in (-PI / f32(1.1), -PI / f32(2.0), -PI / f32(4.0), -PI / f32(8.0), PI / f32(8.0), PI / f32(4.0),
                PI / f32(2.0), PI / f32(1.1)):
        ep, ef = pll_run(NCO, off, 0.0, bw, int(f32(32.0) / f32(bw)))
        assert abs(ep) < 1e-2 and abs(ef) < 1e-2, (bw, off, ep, ef)


@pytest.mark.parametrize("bw", [0.1, 0.05, 0.02, 0.01])
def test_nco_crcf_pll_freq(bw):                               # osc.rs:294-312
    for off in (-0.8, -0.4, -0.2, -0.1, 0.1, 0.2, 0.4, 0.8):
        ep, ef = pll_run(NCO, 0.0, off, bw, int(f32(32.0) / f32(bw)))
        assert abs(ep) < 1e-2 and abs(ef) < 1e-2, (bw, off, ep, ef)


def test_constrain_edge_cases():                              # osc.rs:191-201
    two_pi = TWO_PI
    assert constrain(0.0) == 0 and constrain(-0.0) == 0
    assert constrain(two_pi) == 0                              # exactly 2 pi: one subtraction
    below = np.nextafter(two_pi, f32(0.0))
    assert constrain(below) == (1 << 32) - 256                 # (1 - 2^-24) * 2^32, the largest word reachable from [0, 2 pi)
    assert constrain(f32(-1e-9)) == MASK                       # -1e-9 + 2 pi rounds to 2 pi: the cast saturates
    assert constrain(-PI) == 1 << 31                           # -pi + 2 pi == pi exactly
    assert constrain(PI) == 1 << 31
    assert constrain(float("nan")) == 0                        # NaN skips both loops and casts to 0
    assert constrain(float("inf")) is None and constrain(float("-inf")) is None   # the reference never returns
    assert constrain(f32(3e8)) is None                         # 2 pi is below half an ulp: no progress
    # 99.0: fifteen f32 subtractions of 2 pi, each rounded; the word is within their rounding of the exact one
    exact = (99.0 - 15 * float(two_pi)) / float(two_pi) * 2 ** 32
    assert abs(constrain(99.0) - exact) < 15 * 4e-6 / float(two_pi) * 2 ** 32 + 512
    # negative frequencies wrap to the top of the circle and read back negative through get_frequency's fold
    for f in (-0.123, -1.0, -float(PI) + 1e-3):
        q = OscRef(NCO)
        q.set_frequency(f)
        assert q.d_theta > 1 << 31
        assert abs(q.get_frequency() - f) < 1e-6


def test_hann_and_psd_mask_restatements():
    assert hann(0, 11) == 0.0 and abs(hann(5, 11) - 1.0) < 1e-7
    psd = np.full(64, -80.0, np.float32)
    psd[40] = 0.0
    f40 = 40 / 64 - 0.5
    regions = [(-0.5, f40 - 0.01, 0, -60, False, True), (f40 - 0.01, f40 + 0.01, 0, 0, False, True),
               (f40 + 0.01, 0.5, 0, -60, False, True)]
    assert validate_psd_spectrum(psd, 64, regions)
    psd[10] = -50.0
    assert not validate_psd_spectrum(psd, 64, regions)
    with pytest.raises(ValueError):
        validate_psd_spectrum(psd, 64, [(-0.6, 0.0, 0, 0, False, True)])
