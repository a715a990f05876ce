"""Channel on the device (channel_kernels.hip) against the library's host form and tests/channel_ref.py: every word
equal, at every admissible launch arrangement, at the seams of the tile and of the carried window, across uneven calls,
in the broadcast form, for both oscillator schemes, after reset, reset_channel, a seek beyond 2^32 and a clone."""
import functools

import numpy as np
import pytest

import channel_ref as cr

pytestmark = pytest.mark.gpu

SEED = 41
F = np.float32


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def scheme(ya, vco):
    return ya.OscScheme.Vco if vco else ya.OscScheme.Nco


def pair(ya, C, L, vco=False):
    q, r = ya.Channel(C, L, scheme(ya, vco)), cr.ChannelRef(C, L, vco)
    for o in (q, r):
        cr.configure(o, C, L)
    q.set_seed(SEED)
    r.seed = SEED
    return q, r


@functools.lru_cache(maxsize=None)
def reference(C, L, vco, n, bcast=False):
    """(x, y) of one stream from reset: computed once, shared, read-only"""
    r = cr.ChannelRef(C, L, vco)
    cr.configure(r, C, L)
    r.seed = SEED
    x = cr.streams(n, 1, 100 + C + L)[:, 0] if bcast else cr.streams(n, C, 100 + C + L)
    y = r.execute_block(x)
    x.setflags(write=False), y.setflags(write=False)
    return x, y


def run_cut(q, x, cuts, bcast=False):
    at, out = 0, []
    for n in cuts:
        out.append(q.execute_bcast(x[at:at + n]) if bcast else q.execute(x[at:at + n]))
        at += n
    assert at == len(x)
    return np.concatenate(out)


@pytest.mark.parametrize("L", [1, 2, 17, cr.TAPS_MAX])
@pytest.mark.parametrize("C", [1, 3, 64, 65])
def test_seams_of_the_tile_and_the_window(ya, C, L):
    ts = ya.channel_plan(C, L, 1 << 20)["tile_steps"]
    cuts = [0, 1, max(L - 2, 0), ts - 1, ts, ts + 1]
    for n in cuts[3:]:
        assert ya.channel_plan(C, L, n)["tile_steps"] == ts, "the seam is read from the plan of the call itself"
    x, want = reference(C, L, False, sum(cuts))
    q, r = pair(ya, C, L)
    assert cr.same_words(run_cut(q, x, cuts), want)
    host = ya.Channel.execute_host(*cr.ChannelRef.words(pair_ref(C, L)), x, seed=SEED)
    assert cr.same_words(host, want)
    th, d = q.get_osc_state()
    rr = pair_ref(C, L)
    rr.execute_block(x)
    assert list(th) == rr.theta and list(d) == rr.d_theta and list(q.get_position()) == rr.t


def pair_ref(C, L, vco=False):
    r = cr.ChannelRef(C, L, vco)
    cr.configure(r, C, L)
    r.seed = SEED
    return r


@pytest.mark.parametrize("links", [1, 2, 4, 8, 16, 32, 64])
@pytest.mark.parametrize("C,L", [(3, 17), (65, 5)])
def test_every_arrangement_gives_the_same_words(ya, C, L, links):
    n = 700
    x, want = reference(C, L, True, n)
    xb, wantb = reference(C, L, True, n, bcast=True)
    q, _ = pair(ya, C, L, True)
    for rows in (1, 2, 4, 8, 16):
        q.set_shape(links, rows)
        shape = q.get_shape(n)
        assert (shape["links"], shape["rows"], shape["tile_steps"]) == (links, rows, 256 // links * rows)
        ts = shape["tile_steps"]
        q.reset()
        assert cr.same_words(run_cut(q, x, [ts + 1, n - ts - 1] if ts + 1 < n else [n]), want), (links, rows)
        q.reset()
        assert cr.same_words(run_cut(q, xb, [3, n - 3], bcast=True), wantb), (links, rows, "bcast")
    q.set_shape(0, 0)
    assert q.get_shape(n) == ya.channel_plan(C, L, n, ya.OscScheme.Vco)


def test_more_tiles_than_a_launch_holds_workgroups(ya):
    """at 4 steps per tile a call of 2^22 + 7 steps has more than 2^20 tiles: a workgroup then takes several in turn.
    The host form is the reference here (it equals the restatement, tests/test_channel_capi_cpu.py)"""
    L, n = 3, (1 << 22) + 7
    x = cr.streams(n, 1, 31)
    q, r = pair(ya, 1, L)
    q.set_shape(64, 1)
    assert q.get_shape(n)["tile_steps"] == 4
    want = ya.Channel.execute_host(*r.words(), x, seed=SEED)
    got = q.execute(x)
    assert cr.same_words(got, want)
    tail = cr.streams(9, 1, 32)
    q.set_shape(0, 0)
    r.execute_block(x[-(L - 1):])                                # the window and the words the long call left
    r.theta[0] = (r.theta[0] + (n - (L - 1)) * r.d_theta[0]) & 0xFFFFFFFF
    r.t[0] = n
    assert cr.same_words(q.execute(tail), r.execute_block(tail))


@pytest.mark.parametrize("bcast", [False, True])
@pytest.mark.parametrize("vco", [False, True])
def test_uneven_calls_equal_one_call(ya, vco, bcast):
    C, L, n = 5, 9, 1500
    x, want = reference(C, L, vco, n, bcast)
    q, _ = pair(ya, C, L, vco)
    one = q.execute_bcast(x) if bcast else q.execute(x)
    assert cr.same_words(one, want)
    q.reset()
    cuts = [0, 1, 3, L - 2, L - 1, 1, 700, 2]
    assert cr.same_words(run_cut(q, x, cuts + [n - sum(cuts)], bcast), want)


def test_pitched_and_bcast_calls_share_one_window(ya):
    C, L = 4, 6
    q, r = pair(ya, C, L)
    x = cr.streams(40, C, 8)
    xb = cr.streams(3, 1, 9)[:, 0]
    got = [q.execute(x[:20]), q.execute_bcast(xb), q.execute(x[20:])]
    want = [r.execute_block(x[:20]), r.execute_block(xb), r.execute_block(x[20:])]
    for g, w in zip(got, want):
        assert cr.same_words(g, w)


def test_reset_and_reset_channel(ya):
    C, L, n = 6, 8, 300
    q, r = pair(ya, C, L)
    x = cr.streams(n, C, 12)
    for o, run in ((q, q.execute), (r, r.execute_block)):
        run(x[:100])
        o.reset_channel(2)
    assert cr.same_words(q.execute(x[100:200]), r.execute_block(x[100:200]))
    th, _ = q.get_osc_state()
    assert list(th) == r.theta and list(q.get_position()) == r.t and r.t[2] == 100 and r.t[0] == 200
    q.reset(), r.reset()
    assert cr.same_words(q.execute(x[200:]), r.execute_block(x[200:]))
    assert cr.same_words(q.execute(x[:50]), r.execute_block(x[:50]))
    assert list(q.get_position()) == [150] * C
    fresh = pair_ref(C, L)
    fresh.execute_block(x[200:]), fresh.execute_block(x[:50])
    th, _ = q.get_osc_state()
    assert list(th) == fresh.theta, "reset puts every oscillator back to the phi last set"
    g, s = q.get_gain_noise()
    assert cr.same_words(g, r.gamma) and cr.same_words(s, r.nstd) and cr.same_words(q.get_multipath(), r.h), "parameters stay"


def test_set_position_above_2_32(ya):
    C, L, n = 3, 2, 600
    q, r = pair(ya, C, L)
    x = cr.streams(n, C, 13)
    start = (1 << 32) - 300
    for o in (q, r):
        o.set_position(1, start)
        o.set_position(2, (1 << 63) + 5)
    a, b = q.execute(x[:400]), q.execute(x[400:])
    assert cr.same_words(np.concatenate([a, b]), r.execute_block(x))
    assert list(q.get_position()) == [n, start + n, (1 << 63) + 5 + n]
    far = ya.Channel(1, 1)
    far.set_seed(SEED)
    far.set_gain_noise(0, 0.0, 1.0)
    far.set_position(0, (1 << 32) + 17)
    re, im = cr.noise(SEED, 0, np.arange(4, dtype=np.uint64) + np.uint64((1 << 32) + 17))
    got = far.execute(np.ones((4, 1), np.complex64))
    assert cr.same_words(got[:, 0].real.copy(), F(0.0) + F(1.0) * re) and cr.same_words(got[:, 0].imag.copy(), F(0.0) + F(1.0) * im)


def test_a_clone_taken_mid_stream_continues_identically(ya):
    C, L, n = 66, 7, 500
    x, want = reference(C, L, True, n)
    q, _ = pair(ya, C, L, True)
    q.set_shape(8, 2)
    assert cr.same_words(q.execute(x[:123]), want[:123])
    k = q.clone()
    assert k.get_shape(50) == q.get_shape(50)
    assert cr.same_words(k.execute(x[123:]), want[123:])
    assert cr.same_words(q.execute(x[123:]), want[123:])
    assert cr.same_words(k.get_multipath(), q.get_multipath()) and k.get_seed() == SEED


@pytest.mark.parametrize("bcast", [False, True])
def test_nan_footprint(ya, bcast):
    C, L, n, c, s = 70, 5, 300, 37, 130
    x, want = reference(C, L, False, n, bcast)
    q, _ = pair(ya, C, L)
    q.set_shape(64, 1)                                         # tile of 4 steps: the footprint crosses tiles
    bad = np.array(x)
    if bcast:
        bad[s] = np.nan
    else:
        bad[s, c] = np.nan
    y = q.execute_bcast(bad) if bcast else q.execute(bad)
    changed = (y.view(np.uint32).reshape(n, C, 2) != np.asarray(want).view(np.uint32).reshape(n, C, 2)).any(axis=2)
    expect = np.zeros((n, C), bool)
    if bcast:
        expect[s:s + L, :] = True
    else:
        expect[s:s + L, c] = True
    assert np.array_equal(changed, expect)
    assert np.isnan(y[expect]).all()


@pytest.mark.parametrize("vco", [False, True])
def test_offset_only_equals_the_device_osc(ya, vco):
    n = 5000
    x = cr.streams(n, 1, 21)[:, 0]
    q, o = ya.Channel(1, 1, scheme(ya, vco)), ya.Osc(scheme(ya, vco))
    q.set_carrier_offset(0, 0.37, 6.28)
    o.set_frequency(0.37), o.set_phase(6.28)
    xd, yd = ya.DeviceArray.from_numpy(x), ya.DeviceArray(n, np.complex64)
    o.mix_block_up_dev(xd, n, yd)
    ya.synchronize()
    assert cr.same_words(q.execute(x[:, None])[:, 0], yd.to_numpy())


def test_bad_arguments_on_a_built_object(ya):
    q, _ = pair(ya, 3, 4)
    x = np.zeros((5, 3), np.complex64)
    d = ya.DeviceArray(64, np.complex64)
    for bad in (lambda: q.set_shape(3, 1), lambda: q.set_shape(128, 1), lambda: q.set_shape(4, 3), lambda: q.set_shape(4, 32),
                lambda: q.set_shape(0, 1), lambda: q.reset_channel(3), lambda: q.set_awgn(3, 0.0, 0.0),
                lambda: q.set_gain_noise(3, 1.0, 0.0), lambda: q.set_carrier_offset(3, 0.0, 0.0),
                lambda: q.set_carrier_offset(0, float("inf"), 0.0), lambda: q.set_carrier_offset(0, 0.0, 1e30),
                lambda: q.set_multipath(3, np.zeros(4, np.complex64)), lambda: q.set_position(3, 0),
                lambda: q.execute_devptr(d, 2, 5, d.ptr + 8 * 32, 3), lambda: q.execute_devptr(d, 3, 5, d.ptr + 8 * 32, 2),
                lambda: q.execute_devptr(d, 3, 5, d.ptr + 8 * 8, 3), lambda: q.execute_bcast_devptr(d, 5, d.ptr + 8 * 4, 3),
                lambda: q.execute_devptr(d, 3, 1 << 31, d.ptr + 8 * 32, 3), lambda: q.execute_devptr(d.ptr + 4, 3, 5, d.ptr + 8 * 32, 3),
                lambda: q.execute_devptr(None, 3, 5, d, 3)):
        with pytest.raises(ya.ConfigError):
            bad()
    th, dth = q.get_osc_state()
    r = pair_ref(3, 4)
    assert list(th) == r.theta and list(dth) == r.d_theta, "a refused offset changes nothing"
    q.execute_devptr(None, 3, 0, None, 3)                       # n = 0 is valid and touches nothing
    assert cr.same_words(q.execute(x), r.execute_block(x))
