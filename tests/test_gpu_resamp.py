"""Resamp through the C ABI -- mirrors src/filter/resampler/resamp.rs:24-165 and its tests (:167-391).

Expected outputs come from resamp_util.RefResamp: the reference's per-sample loop (u32 phase, step = round(2^24 /
rate)) over the golden-pinned oracle.FirPfbFilter; large blocks are checked against the closed form of the same
schedule.  Integer data makes every sum exact, so the comparisons are bit for bit."""
import math

import numpy as np
import pytest

from gpu_util import int_samples, int_taps, rand_samples, rel_l2
from psd_util import validate_psd_signal
from resamp_util import RefResamp, bank, closed_form, designed_taps, loop_count, num_output, rust_step

pytestmark = pytest.mark.gpu
KINDS = ["rrrf", "crcf", "cccf"]
SIZES = [1, 2, 3, 20, 7, 64, 4, 4, 4, 27]                 # resamp.rs:336


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


def run_dev(ya, q, x):
    """one execute_block_dev call on a copy of x; returns the outputs"""
    ny = q.get_num_output(len(x))
    xd = ya.DeviceArray.from_numpy(np.ascontiguousarray(x))
    yd = ya.DeviceArray(max(ny, 1), x.dtype)
    nw = q.execute_block_dev(xd, len(x), yd, ny)
    assert nw == ny
    return yd.to_numpy(nw)


def test_config_and_getters(ya):
    cases = [((0.0, 7, 0.25, 60.0, 256), ya.ConfigError),      # rate <= 0
             ((-1.0, 7, 0.25, 60.0, 256), ya.ConfigError),
             ((1.0, 0, 0.25, 60.0, 256), ya.ConfigError),      # m == 0
             ((1.0, 7, 0.0, 60.0, 256), ya.ConfigError),       # fc outside (0, 0.5)
             ((1.0, 7, 0.5, 60.0, 256), ya.ConfigError),
             ((1.0, 7, 0.25, 0.0, 256), ya.ConfigError),       # as <= 0
             ((1.0, 7, 0.25, 60.0, 0), ya.ValueError_),        # nextpow2(0) is Error::Value
             ((1.0, 7, 0.25, 60.0, 1), ya.ConfigError),        # bits 0
             ((1.0, 2, 0.25, 60.0, (1 << 16) + 1), ya.ConfigError),    # bits 17
             ((0.0039, 7, 0.25, 60.0, 16), ya.ConfigError),    # set_rate range
             ((250.5, 7, 0.25, 60.0, 16), ya.ConfigError)]
    for args, err in cases:
        with pytest.raises(err):
            ya.Resamp("crcf", *args)
    with pytest.raises(ya.ConfigError):
        ya.Resamp.new_default("crcf", 0.0)
    with pytest.raises(ya.ConfigError):
        ya.Resamp.from_taps("crcf", 1.0, 2, 12, np.ones(48, np.float32))     # npfb not a power of two
    q = ya.Resamp("crcf", 0.9, 5, 0.3, 60.0, 100)               # npfb rounded up to 128
    assert q.get_rate() == np.float32(0.9) and q.get_delay() == 5
    d = ya.Resamp.new_default("rrrf", 1.5)
    assert d.get_delay() == 7 and d.get_rate() == np.float32(1.5)
    for bad in (0.0, -2.0, 0.0039, 250.01):
        with pytest.raises(ya.ConfigError):
            d.set_rate(bad)
    assert d.get_rate() == np.float32(1.5)
    for bad in (0.0, -1.0, 200.0, 0.002):                       # gamma <= 0, or the product outside [0.004, 250]
        with pytest.raises(ya.ConfigError):
            d.adjust_rate(bad)
    d.adjust_rate(2.0)
    assert d.get_rate() == np.float32(3.0)
    d.set_rate(250.0)
    d.set_rate(0.004)
    x = np.zeros(300, np.float32)
    with pytest.raises(ya.RangeError):                          # output capacity below get_num_output
        d.execute_block_dev(ya.DeviceArray.from_numpy(x), 300, ya.DeviceArray(1, np.float32), 0)


def test_schedule_closed_form_matches_the_loop():
    """the host-side closed form (count, carried phase) against the reference loop, rates 0.004 .. 250"""
    for rate in [0.004, 0.0041, 0.127115323, 0.5, 1.0, math.sqrt(2), math.sqrt(17), math.exp(5), 249.9, 250.0]:
        step, p, pc = rust_step(rate), 0, 0
        for n in SIZES * 3 + [1000]:
            a, p = loop_count(p, step, n)
            b, pc = num_output(pc, step, n)
            assert (a, p) == (b, pc)


@pytest.mark.parametrize("rate,npfb", [(1.0, 64), (1.0, 256), (0.5, 256), (math.sqrt(2), 256), (math.sqrt(17), 16),
                                       (1 / math.pi, 64), (math.exp(5), 64), (math.exp(-5), 64),
                                       (0.004, 64), (250.0, 64)])
def test_num_output(ya, rate, npfb):
    """resamp.rs:315-390 (num_output_0 .. 7, plus both ends of the rate range): get_num_output(n) == nw of
    execute_block == the reference loop, the size sequence run 8 times; again through execute_block_dev"""
    rate = float(np.float32(rate))
    for dev in (False, True):
        q = ya.Resamp("cccf", rate, 20, 0.4, 60.0, npfb)
        step, phase = rust_step(rate), 0
        for _ in range(8):
            for n in SIZES:
                want, phase = loop_count(phase, step, n)
                assert q.get_num_output(n) == want
                x = np.zeros(n, np.complex64)
                got = len(run_dev(ya, q, x)) if dev else len(q.execute_block(x))
                assert got == want


# (rate, npfb, m) cases: every rate of the issue, each npfb and m several times
PARITY = [(0.004, 16, 7), (0.127115323, 2048, 20), (0.5, 2, 1), (0.7123921, 256, 7), (1.0, 16, 20),
          (math.sqrt(2), 2048, 1), (math.sqrt(17), 256, 20), (math.exp(5), 2, 7), (250.0, 256, 1),
          (0.004, 2048, 1), (250.0, 16, 20), (0.7123921, 2, 20)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rate,npfb,m", PARITY)
def test_bit_exact_mixed_calls(ya, oracle, kind, rate, npfb, m):
    """integer taps and samples: ragged calls (shorter than 2m, producing nothing, single samples) through execute,
    execute_block (host mirror and device) and execute_block_dev, with adjust_rate between calls, equal the
    reference loop bit for bit"""
    rng = np.random.default_rng(int(rate * 1000) + 7 * npfb + m)
    rate = float(np.float32(rate))
    h = int_taps(rng, kind, 2 * m * npfb + 5)
    nx = int(min(4000, max(40 + 4 * m, 6000 / rate)))
    x = int_samples(rng, kind, nx)
    ref = RefResamp(oracle, kind, rate, m, npfb, h)
    q = ya.Resamp.from_taps(kind, rate, m, npfb, h)
    gamma = np.float32(0.999) if rate > 1 else np.float32(1.001)
    cuts = [1, 2, max(1, 2 * m - 1), 1, 5, 33, 1, 2, 31, 70, 1, 3]
    pos, call = 0, 0
    while pos < nx:
        n = min(cuts[call % len(cuts)] if call < 3 * len(cuts) else nx - pos, nx - pos)
        seg = x[pos:pos + n]
        want = ref.execute_block(seg)
        mode = call % 4
        if mode == 0 and n == 1:
            got = q.execute(seg[0])
        elif mode == 1:
            got = q.execute_block(seg)
        else:
            got = run_dev(ya, q, seg)
        assert got.shape == want.shape, (call, n, mode)
        assert np.array_equal(got, want), (call, n, mode)
        if call % 5 == 4:
            q.adjust_rate(gamma)
            ref.adjust_rate(gamma)
            if 0.01 < rate < 100:                             # near the ends of the range: keep moving inwards
                gamma = np.float32(1) / gamma
            assert q.get_rate() == ref.r
        pos += n
        call += 1


@pytest.mark.parametrize("kind,rate", [("crcf", 0.3), ("crcf", 1.1), ("crcf", 3.7), ("rrrf", 1.1)])
def test_large_device_blocks(ya, kind, rate):
    """2^24 integer inputs in one call (many workgroups, ragged last tile) == the closed-form schedule; the same
    stream cut into many short calls gives the same bits"""
    m, npfb = 7, 256
    rng = np.random.default_rng(int(rate * 10))
    rate = float(np.float32(rate))
    h = int_taps(rng, kind, 2 * m * npfb)
    n = 1 << 24
    x = int_samples(rng, kind, n)
    hb = bank(h, m, npfb)
    want, _ = closed_form(hb, np.zeros(2 * m, x.dtype), x, rust_step(rate), 0, 8)
    q = ya.Resamp.from_taps(kind, rate, m, npfb, h)
    xd = ya.DeviceArray.from_numpy(x)
    ny = q.get_num_output(n)
    assert ny == len(want)
    yd = ya.DeviceArray(ny, x.dtype)
    assert q.execute_block_dev(xd, n, yd, ny) == ny
    assert np.array_equal(yd.to_numpy(), want)
    q.reset()
    cuts = np.concatenate([[1, 3, 17, 2, 13], rng.integers(1, 200_000, 300)])
    bounds = np.minimum(np.concatenate([[0], np.cumsum(cuts)]), n)
    bounds = np.unique(np.append(bounds, n))
    yd.zero()
    off = 0
    for a, b in zip(bounds[:-1], bounds[1:]):
        a, b = int(a), int(b)
        cnt = q.get_num_output(b - a)
        nw = q.execute_block_dev(xd.ptr + a * x.itemsize, b - a, yd.ptr + off * x.itemsize, cnt)
        assert nw == cnt
        off += nw
    assert off == ny
    assert np.array_equal(yd.to_numpy(), want)


@pytest.mark.parametrize("kind,rate,m,fc,as_,npfb", [("crcf", 0.7123921, 7, 0.25, 60.0, 256),
                                                      ("cccf", math.sqrt(2), 12, 0.4, 60.0, 64),
                                                      ("rrrf", 3.7, 5, 0.3, 80.0, 100),
                                                      ("crcf", 0.127115323, 20, 0.45, 60.0, 2048)])
def test_designed_taps(ya, oracle, kind, rate, m, fc, as_, npfb):
    """new() on random data against the loop over the reference's design (Kaiser, DC gain npfb by a sequential f32
    sum); one host block and one device block"""
    rng = np.random.default_rng(5)
    rate = float(np.float32(rate))
    p2 = 1 << (int(npfb) - 1).bit_length()
    h = designed_taps(oracle, m, fc, as_, p2)
    x = rand_samples(rng, kind, 3000)
    ref = RefResamp(oracle, kind, rate, m, p2, h)
    want = ref.execute_block(x)
    q = ya.Resamp(kind, rate, m, fc, as_, npfb)
    got = np.concatenate([q.execute_block(x[:1700]), run_dev(ya, q, x[1700:])])
    assert got.shape == want.shape
    assert rel_l2(got, want) <= 1e-6


@pytest.mark.parametrize("r,as_", [(0.127115323, 60.0), (0.373737373, 60.0), (0.676543210, 60.0), (0.973621947, 60.0),
                                   (0.127115323, 80.0), (0.373737373, 80.0), (0.676543210, 80.0), (0.973621947, 80.0)])
def test_spectral_mask(ya, oracle, r, as_):
    """resamp.rs:177-262 (resamp_crcf_00 .. 03, 10 .. 13): Resamp::<Complex32> (cccf), m 20, fc 0.45, npfb 2048, a
    Kaiser pulse of bandwidth r bw through it, the output spectrum inside the reference's regions"""
    bw, tol, m, npfb, fc = 0.25, 0.5, 20, 2048, 0.45
    r32 = np.float32(r)
    q = ya.Resamp("cccf", float(r32), m, fc, as_, npfb)
    p = int(np.float32(40.0) / r32)
    pulse_len = 4 * p + 1
    pulse = oracle.fir_design_kaiser(pulse_len, float(np.float32(0.5) * r32 * np.float32(bw)), 120.0, 0.0)
    num_input = pulse_len + 2 * m + 1
    x = np.zeros(num_input, np.complex64)
    x[:pulse_len] = pulse * np.float32(bw)
    nout = q.get_num_output(num_input)
    y = q.execute_block(x)
    assert len(y) == nout > 0
    regions = [(-0.5, -0.6 * bw, 0.0, -as_ + tol, False, True),
               (-0.4 * bw, 0.4 * bw, -tol, tol, True, True),
               (0.6 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    ok, worst = validate_psd_signal(y, regions)
    assert ok, worst


def test_copy(ya):
    """resamp.rs:392-431 (resamp_crcf_copy): clone after 80 samples, then equal counts (< 2) and equal samples"""
    rng = np.random.default_rng(17)
    q0 = ya.Resamp("cccf", float(np.float32(0.71239213987520)), 17, 0.37, 60.0, 64)
    for v in rand_samples(rng, "cccf", 80):
        q0.execute(v)
    q1 = q0.clone()
    for v in rand_samples(rng, "cccf", 80):
        y0, y1 = q0.execute(v), q1.execute(v)
        assert len(y0) < 2 and len(y1) < 2 and len(y0) == len(y1)
        assert np.array_equal(y0, y1)
    x = rand_samples(rng, "cccf", 500)                          # and on the device path
    assert np.array_equal(run_dev(ya, q0, x), run_dev(ya, q1, x))
