"""Fdelay on the device (fdelay_kernels.hip) against tests/fdelay_ref.py: every output word of the fixed-delay block form
and of the per-sample-delay track form bit for bit, through host and device calls, on calls cut across the tile seam and
shorter than both histories, with the delay changing between and inside calls; and the reference's own tests
(src/filter/fdelay.rs:146-279) on the device output."""
import numpy as np
import pytest

from fdelay_ref import KINDS, Design, FdelayRef, block, delay_estimate, f32, lag, reset_state, same_bits
from test_fdelay_ref_cpu import DELAYS, SHAPES, doppler_input, doppler_peak, rand_input, splits, tracks

pytestmark = pytest.mark.gpu


def ya():
    import yagi_amd
    return yagi_amd


def dev_call(q, x, delays=None):
    Y = ya()
    n = len(x)
    xd = Y.DeviceArray.from_numpy(x) if n else Y.DeviceArray(1, x.dtype)
    yd = Y.DeviceArray(max(n, 1), x.dtype)
    if delays is None:
        q.execute_block_dev(xd, n, yd)
    else:
        dd = Y.DeviceArray.from_numpy(np.asarray(delays, f32)) if n else Y.DeviceArray(1, f32)
        q.execute_track_dev(dd, xd, n, yd)
    Y.synchronize()
    return yd.to_numpy(n) if n else np.zeros(0, x.dtype)


def call(q, path, x, delays=None):
    if path == "dev":
        return dev_call(q, x, delays)
    return q.execute_block(x) if delays is None else q.execute_track(delays, x)


def wrap_delay(nmax, npfb):
    """a delay whose branch rounds up to npfb and wraps into the window index"""
    d = f32(min(2, nmax - 1)) + f32(1.0) / f32(4 * npfb)
    return d


def fixed_delays(nmax, npfb):
    return [f32(0.0), f32(nmax), wrap_delay(nmax, npfb), f32(nmax) * f32(0.37)]


@pytest.fixture(scope="module")
def designs(oracle):
    cache = {}

    def get(kind, shape):
        if (kind, shape) not in cache:
            cache[(kind, shape)] = Design(oracle, kind, *shape)
        return cache[(kind, shape)]
    return get


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_fixed_delay_bitwise(designs, kind, shape, path):
    d = designs(kind, shape)
    q = ya().Fdelay(kind, *shape)
    st = reset_state(d)
    rng = np.random.default_rng(11)
    ds = fixed_delays(d.nmax, d.npfb)
    w, f = lag(ds[2], d.nmax, d.npfb)
    assert f == 0 and f32(f32(d.nmax) - ds[2]) != np.floor(f32(d.nmax) - ds[2])       # the wrap case wraps
    for i, n in enumerate(splits(d.Ls)):
        x = rand_input(rng, kind, n)
        if i > 0:                                                # the first call runs at reset()'s own lag
            dl = ds[(i - 1) % len(ds)]
            q.set_delay(dl)
            st = st[:2] + (dl,) + lag(dl, d.nmax, d.npfb)
        want, st = block(d, st, x)
        got = call(q, path, x)
        assert same_bits(got, want), (kind, shape, path, i, n)
        assert q.get_delay() == st[2]


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_track_bitwise(designs, kind, shape, path):
    d = designs(kind, shape)
    q = ya().Fdelay(kind, *shape)
    st = reset_state(d)
    rng = np.random.default_rng(12)
    cuts = splits(d.Ls)
    total = sum(cuts)
    for name, tr in tracks(rng, d.nmax, d.npfb, total).items():
        at = 0
        for i, n in enumerate(cuts):
            x = rand_input(rng, kind, n)
            want, st = block(d, st, x, tr[at: at + n])
            got = call(q, path, x, tr[at: at + n])
            assert same_bits(got, want), (kind, shape, path, name, i, n)
            if n:
                assert q.get_delay() == tr[at + n - 1]
            at += n
        # a fixed-delay call at the lag the track left, then one after set_delay: both forms share one state
        x = rand_input(rng, kind, 700)
        want, st = block(d, st, x)
        assert same_bits(call(q, path, x), want), (kind, shape, path, name, "fixed after track")
        dl = f32(d.nmax) * f32(0.61)
        q.set_delay(dl)
        st = st[:2] + (dl,) + lag(dl, d.nmax, d.npfb)
        x = rand_input(rng, kind, 300)
        want, st = block(d, st, x)
        assert same_bits(call(q, path, x), want), (kind, shape, path, name, "fixed after set_delay")


@pytest.mark.parametrize("kind", list(KINDS))
def test_impulse_sign_of_zero(designs, kind):
    shape = (5, 2, 3)
    d = designs(kind, shape)
    for amp in (1.0, -1.0):
        q = ya().Fdelay(kind, *shape)
        x = np.zeros(1500, d.tdt)
        x[0] = amp
        x[1030] = -amp
        x[7::2] = -0.0                                            # negative zeros through the products and the unit scale
        tr = np.linspace(0, 5, 1500).astype(f32)
        st = reset_state(d)
        want, st = block(d, st, x)
        assert same_bits(dev_call(q, x), want)
        want, st = block(d, st, x, tr)
        assert same_bits(dev_call(q, x, tr), want)


@pytest.mark.parametrize("path", ["single", "host", "dev"])
@pytest.mark.parametrize("delay", DELAYS)
def test_reference_delay_estimates(delay, path):                  # fdelay.rs:146-222
    nmax, m, npfb = 200, 12, 64
    q = ya().Fdelay("rrrf", nmax, m, npfb)
    q.set_delay(f32(delay) * f32(0.7))
    q.adjust_delay(f32(delay) * f32(0.3))
    assert (q.get_nmax(), q.get_m(), q.get_npfb()) == (nmax, m, npfb)
    assert abs(float(q.get_delay()) - delay) <= 1e-6 * max(1.0, delay)
    x = np.zeros(nmax + 2 * m, f32)
    x[0] = 1.0
    if path == "single":
        y = np.zeros_like(x)
        for i, v in enumerate(x):
            q.push(v)
            y[i] = q.execute()
    else:
        y = call(q, path, x)
    assert abs(float(delay_estimate(y, m)) - delay) <= 0.01


@pytest.mark.parametrize("path", ["host", "dev"])
def test_doppler_peak(path):
    q = ya().Fdelay("crcf", 200, 12, 64)
    x, tr = doppler_input()
    assert doppler_peak(call(q, path, x, tr)) == 504


def test_config_errors_leave_object_unchanged(designs):           # fdelay.rs:224-249
    Y = ya()
    for bad in ((0, 12, 64), (200, 0, 64), (200, 12, 0)):
        with pytest.raises(Y.ConfigError):
            Y.Fdelay("rrrf", *bad)
    with pytest.raises(Y.ConfigError):
        Y.Fdelay("rrrf", 0)
    shape = (200, 8, 64)
    d = designs("rrrf", shape)
    q = Y.Fdelay("rrrf", 200)
    assert (q.get_nmax(), q.get_m(), q.get_npfb()) == shape
    rng = np.random.default_rng(5)
    st = reset_state(d)
    q.set_delay(7.25)
    st = st[:2] + (f32(7.25),) + lag(7.25, 200, 64)
    x = rand_input(rng, "rrrf", 900)
    want, st = block(d, st, x)
    assert same_bits(q.execute_block(x), want)
    bad_track = np.full(300, 3.0, f32)
    bad_track[299] = 200.5
    for fn in (lambda: q.set_delay(-1.0), lambda: q.set_delay(201.0), lambda: q.set_delay(float("nan")),
               lambda: q.adjust_delay(-8.0), lambda: q.adjust_delay(193.0),
               lambda: q.execute_track(bad_track, x[:300])):
        with pytest.raises(Y.ConfigError):
            fn()
        assert q.get_delay() == f32(7.25)
    x = rand_input(rng, "rrrf", 500)
    want, st = block(d, st, x)
    assert same_bits(q.execute_block(x), want)


@pytest.mark.parametrize("kind", list(KINDS))
def test_push_write_execute_and_mixing(oracle, designs, kind):    # fdelay.rs:252-279
    Y = ya()
    shape = (200, 8, 64)
    d = designs(kind, shape)
    q0, q1, ref = Y.Fdelay(kind, 200), Y.Fdelay(kind, 200), FdelayRef(oracle, d)
    for q in (q0, q1, ref):
        q.set_delay(7.2280)
    buf = np.array([-1.0, 3.0, 5.0, -3.0, 5.0, 1.0, -3.0, -4.0], d.tdt)
    for trial in range(20):
        n = trial % 8
        for v in buf[:n]:
            q0.push(v)
        q1.write(buf[:n])
        ref.write(buf[:n])
        v0, v1 = q0.execute(), q1.execute()
        assert same_bits(np.array([v0]), np.array([v1])) and same_bits(np.array([v0]), np.array([ref.execute()]))
    # per-sample calls, then a device block, then per-sample calls again: one state
    rng = np.random.default_rng(3)
    x = rand_input(rng, kind, 1300)
    assert same_bits(dev_call(q0, x), ref.execute_block(x))
    for v in buf:
        q0.push(v)
        ref.push(v)
        assert same_bits(np.array([q0.execute()]), np.array([ref.execute()]))
    tr = (rng.random(400) * 200).astype(f32)
    x = rand_input(rng, kind, 400)
    assert same_bits(dev_call(q0, x, tr), ref.execute_track(tr, x))
    q0.push(buf[0])
    ref.push(buf[0])
    assert same_bits(np.array([q0.execute()]), np.array([ref.execute()]))
    assert q0.get_delay() == ref.get_delay()


def test_clone_reset_and_stream(designs):
    import torch
    Y = ya()
    shape = (200, 8, 64)
    d = designs("crcf", shape)
    rng = np.random.default_rng(8)
    q = Y.Fdelay("crcf", 200)
    st = reset_state(d)
    s = torch.cuda.Stream()
    q.set_stream(s.cuda_stream)
    tr = (rng.random(3000) * 200).astype(f32)
    x = rand_input(rng, "crcf", 3000)
    want, st = block(d, st, x, tr)
    with torch.cuda.stream(s):
        assert same_bits(dev_call(q, x, tr), want)
    c = q.clone()                                                 # mid-stream, after a device track
    assert c.get_delay() == q.get_delay() == tr[-1]
    x = rand_input(rng, "crcf", 2100)
    want, st2 = block(d, st, x)
    assert same_bits(dev_call(q, x), want) and same_bits(dev_call(c, x), want)
    q.reset()
    assert q.get_delay() == 0
    want, _ = block(d, reset_state(d), x)
    assert same_bits(dev_call(q, x), want)
    want, _ = block(d, st2, x[:50])                               # the clone is untouched by the reset
    assert same_bits(c.execute_block(x[:50]), want)


def test_dev_track_clamps(designs):
    shape = (5, 2, 3)
    d = designs("rrrf", shape)
    q = ya().Fdelay("rrrf", *shape)
    rng = np.random.default_rng(9)
    x = rand_input(rng, "rrrf", 1200)
    tr = (rng.random(1200) * 9 - 2).astype(f32)                  # below 0 and above nmax
    tr[5] = np.nan
    tr[6] = -np.inf
    tr[7] = np.inf
    tr[-1] = 77.0
    clamped = np.where(tr >= 0, np.minimum(tr, f32(5)), f32(0)).astype(f32)
    want, st = block(d, reset_state(d), x, clamped)
    assert same_bits(dev_call(q, x, tr), want)
    assert q.get_delay() == f32(5.0)


# Shapes beyond the issue's five.  The track kernel stages its nmax-deep input halo in LDS while tile, halo and span fit
# 64 KiB (kFdLdsBudget) and gathers through L2 above: with m = 8 (Ls = 16, 1039-sample tile span) and 4096 B of branch
# indices that is (1039 + 1039 + nmax) * sizeof(T) + 4096 <= 65536, so nmax = 5602 is the last complex shape in LDS and
# 5603 the first through L2 (real: 13282 / 13283).
BEYOND_LDS = [("crcf", (5602, 8, 64)), ("crcf", (5603, 8, 64)), ("crcf", (9000, 8, 64)), ("cccf", (9000, 8, 64)),
              ("rrrf", (13283, 8, 64)), ("rrrf", (20000, 8, 64))]


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("kind,shape", BEYOND_LDS)
def test_track_beyond_the_lds_halo(designs, kind, shape, path):
    d = designs(kind, shape)
    q = ya().Fdelay(kind, *shape)
    st = reset_state(d)
    rng = np.random.default_rng(14)
    cuts = splits(d.Ls) + [1, 4100]                               # every call is shorter than the history
    trs = tracks(rng, d.nmax, d.npfb, sum(cuts))
    for name in ("random", "ramp", "step"):
        at = 0
        for i, n in enumerate(cuts):
            x = rand_input(rng, kind, n)
            want, st = block(d, st, x, trs[name][at: at + n])
            got = call(q, path, x, trs[name][at: at + n])
            assert same_bits(got, want), (kind, shape, path, name, i, n)
            at += n
        x = rand_input(rng, kind, 2100)                           # the fixed-delay form on the same long history
        want, st = block(d, st, x)
        assert same_bits(call(q, path, x), want), (kind, shape, path, name, "fixed after track")
        assert q.get_delay() == st[2]


# branch lengths that give the block kernel's sliding window full chunks AND a remainder: Ls = 12 against 8 real
# outputs per lane (1 chunk + 4 taps), Ls = 5 against 4 complex ones (1 chunk + 1 tap; real: the remainder alone)
CHUNK_SHAPES = [(7, 6, 5), (3, 2, 1)]


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("shape", CHUNK_SHAPES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_chunk_and_remainder_branch_lengths(designs, kind, shape, path):
    d = designs(kind, shape)
    assert d.Ls == {(7, 6, 5): 12, (3, 2, 1): 5}[shape]
    q = ya().Fdelay(kind, *shape)
    st = reset_state(d)
    rng = np.random.default_rng(15)
    ds = fixed_delays(d.nmax, d.npfb)
    cuts = splits(d.Ls)
    tr = tracks(rng, d.nmax, d.npfb, sum(cuts))["random"]
    at = 0
    for i, n in enumerate(cuts):
        x = rand_input(rng, kind, n)
        dl = ds[i % len(ds)]
        q.set_delay(dl)
        st = st[:2] + (dl,) + lag(dl, d.nmax, d.npfb)
        want, st = block(d, st, x)
        assert same_bits(call(q, path, x), want), (kind, shape, path, "fixed", i, n)
        x = rand_input(rng, kind, n)
        want, st = block(d, st, x, tr[at: at + n])
        assert same_bits(call(q, path, x, tr[at: at + n]), want), (kind, shape, path, "track", i, n)
        at += n


@pytest.mark.parametrize("kind", list(KINDS))
def test_dev_buffers_off_16_byte_alignment(designs, kind):
    """full tiles whose x and y start one element into an allocation: the block kernel's element-wise store path"""
    Y = ya()
    shape = (200, 8, 64)
    d = designs(kind, shape)
    q = Y.Fdelay(kind, *shape)
    q.set_delay(33.4)
    st = reset_state(d)
    st = st[:2] + (f32(33.4),) + lag(33.4, 200, 64)
    rng = np.random.default_rng(16)
    n = 5000                                                       # two full tiles of either size and a partial one
    x = rand_input(rng, kind, n)
    item = x.dtype.itemsize
    xd = Y.DeviceArray.from_numpy(np.concatenate([np.zeros(1, x.dtype), x]))
    yd = Y.DeviceArray(n + 1, x.dtype)
    want, st = block(d, st, x)
    q.execute_block_dev(xd.ptr + item, n, yd.ptr + item)
    Y.synchronize()
    assert same_bits(yd.to_numpy(n, 1), want)
    tr = (rng.random(n) * 200).astype(f32)
    want, st = block(d, st, x, tr)
    q.execute_track_dev(Y.DeviceArray.from_numpy(tr), xd.ptr + item, n, yd.ptr + item)
    Y.synchronize()
    assert same_bits(yd.to_numpy(n, 1), want)


def test_default_constructor_and_scale_methods():
    Y = ya()
    q = Y.Fdelay("crcf", 300)                                     # create_default: fdelay.rs:55-57
    assert (q.get_nmax(), q.get_m(), q.get_npfb()) == (300, 8, 64)
    for fn in (lambda: q.set_scale(2.0), q.get_scale):
        with pytest.raises(Y.ConfigError):
            fn()
    with pytest.raises(Y.ConfigError):
        Y.Fdelay("rrrf", (1 << 24) + 1)                           # beyond the exact range of set_delay's f32 steps
