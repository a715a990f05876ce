"""Agc on the device against tests/agc_ref.py, bit for bit (a NaN matching a NaN): every output word, the status plane,
and after every call the gains, the squelch modes and the locks."""
import functools

import numpy as np
import pytest

import agc_ref as ar

pytestmark = pytest.mark.gpu

N = 260
CUTS = (0, 1, 7, N - 8)            # the rows of the calls: an empty one, one row, less than a chunk, the rest
BW, G0, THR, TIMEOUT, SCALE = 0.25, 1000.0, -50.0, 5, 1.5


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def configure(q, squelch):
    q.set_bandwidth(BW), q.set_scale(SCALE), q.set_gain(G0)
    q.squelch_set_threshold(THR), q.squelch_set_timeout(TIMEOUT)
    if squelch:
        q.squelch_enable()


@functools.lru_cache(maxsize=None)
def reference(C, kind, squelch):
    """the restatement over the cut stream, once per shape: per call (y, status, g, mode, locked)"""
    x = ar.streams(N, C, 100 + C, kind)
    r = ar.AgcRef(C, kind)
    configure(r, squelch)
    out, at = [], 0
    for rows in CUTS:
        y, st = r.execute_block(x[at:at + rows])
        out.append((y, st, r.get_gain(), r.squelch_get_status(), r.get_locked()))
        at += rows
    for v in out:
        for a in v:
            a.setflags(write=False)
    x.setflags(write=False)
    return x, out


def check_state(q, want):
    assert ar.same_words(q.get_gain(), want[2])
    assert np.array_equal(q.squelch_get_status(), want[3]) and np.array_equal(q.get_locked(), want[4])


@pytest.mark.parametrize("status", [False, True])
@pytest.mark.parametrize("squelch", [False, True])
@pytest.mark.parametrize("kind", ["crcf", "rrrf"])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 200])
def test_host_blocks(ya, C, kind, squelch, status):
    x, want = reference(C, kind, squelch)
    q = ya.Agc(C, kind)
    configure(q, squelch)
    at = 0
    for rows, w in zip(CUTS, want):
        got = q.execute_block(x[at:at + rows], status=status)
        y, st = got if status else (got, None)
        assert ar.same_words(y, w[0]), (C, kind, squelch, at)
        if status:
            assert np.array_equal(st, w[1])
        check_state(q, w)
        at += rows


@pytest.mark.parametrize("status", [False, True])
@pytest.mark.parametrize("squelch", [False, True])
@pytest.mark.parametrize("kind", ["crcf", "rrrf"])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 200])
def test_device_blocks_with_wide_pitches(ya, C, kind, squelch, status):
    x, want = reference(C, kind, squelch)
    q = ya.Agc(C, kind)
    configure(q, squelch)
    at = 0
    for rows, w in zip(CUTS, want):
        y, st = ar.run_dev(ya, q, x[at:at + rows], status=status, pad=3)
        assert ar.same_words(y[:, :C], w[0]) and (y[:, C:] == 0).all(), (C, kind, squelch, at)
        if status:
            assert np.array_equal(st[:, :C], w[1]) and (st[:, C:] == 0).all()
        check_state(q, w)
        at += rows


@pytest.mark.parametrize("kind", ["crcf", "rrrf"])
def test_in_place_equals_out_of_place(ya, kind):
    C = 65
    x, want = reference(C, kind, True)
    q = ya.Agc(C, kind)
    configure(q, True)
    xd = ya.DeviceArray.from_numpy(np.ascontiguousarray(x))
    q.execute_block_devptr(xd.ptr, C, N, xd.ptr, C)
    ya.synchronize()
    y = xd.to_numpy().reshape(N, C)
    xd.free()
    assert ar.same_words(y, np.concatenate([w[0] for w in want]))
    check_state(q, want[-1])
    with pytest.raises(ya.ConfigError):                              # a partial overlap
        q.execute_block_devptr(1 << 20, C, 4, (1 << 20) + 8, C)


@pytest.mark.parametrize("kind", ["crcf", "rrrf"])
def test_a_subset_locked_in_mid_stream(ya, kind):
    C = 70
    x = ar.streams(120, C, 5, kind)
    q, r = ya.Agc(C, kind), ar.AgcRef(C, kind)
    configure(q, True), configure(r, True)
    assert ar.same_words(q.execute_block(x[:50]), r.execute_block(x[:50])[0])
    free = r.clone()
    locked = (np.arange(C) % 3 == 0).astype(np.uint8)
    q.set_locked(locked), r.set_locked(locked)
    assert not q.is_locked() and np.array_equal(q.get_locked(), locked)
    g0 = q.get_gain()
    y, st = q.execute_block(x[50:], status=True)
    wy, wst = r.execute_block(x[50:])
    fy, _ = free.execute_block(x[50:])
    assert ar.same_words(y, wy) and np.array_equal(st, wst)
    on = locked != 0
    assert ar.same_words(q.get_gain()[on], g0[on]), "a locked channel's gain moved"
    assert ar.same_words(y[:, ~on], fy[:, ~on]), "locking some channels changed the others"
    assert ar.same_words(q.get_gain(), r.get_gain())
    q.lock()
    assert q.is_locked()
    q.unlock()
    assert not q.get_locked().any()


def test_clone_reset_and_the_setters_between_calls(ya):
    C, kind = 66, "crcf"
    x = ar.streams(90, C, 9, kind)
    q, r = ya.Agc(C, kind), ar.AgcRef(C, kind)
    configure(q, True), configure(r, True)

    def both(lo, hi, *pairs):
        for a, b in pairs or ((q, r),):
            y, st = a.execute_block(x[lo:hi], status=True)
            wy, wst = b.execute_block(x[lo:hi])
            assert ar.same_words(y, wy) and np.array_equal(st, wst), (lo, hi)
            assert ar.same_words(a.get_gain(), b.get_gain())
            assert ar.same_words(a.get_rssi(), b.get_rssi()) and ar.same_words(a.get_signal_level(), b.get_signal_level())
            assert np.array_equal(a.squelch_get_status(), b.squelch_get_status())

    both(0, 20)
    q2, r2 = q.clone(), r.clone()
    both(20, 30, (q, r), (q2, r2))
    q.reset_channel(5), r.reset_channel(5)
    q.set_bandwidth(0.05), r.set_bandwidth(0.05)
    q.set_scale(0.5), r.set_scale(0.5)
    both(30, 40)
    gains = (1.0 + np.arange(C)).astype(np.float32)
    q.set_gains(gains), r.set_gains(gains)
    both(40, 50)
    q.set_rssi(-37.5), r.set_rssi(-37.5)
    both(50, 60)
    q.set_signal_level(0.02), r.set_signal_level(0.02)
    both(60, 70)
    q.squelch_disable(), r.squelch_disable()
    both(70, 80)
    q.reset(), r.reset()
    both(80, 90, (q, r), (q2, r2))
    assert q.get_bandwidth() == np.float32(0.05) and q.get_scale() == 0.5 and not q.squelch_is_enabled()
    assert q2.squelch_is_enabled() and q2.squelch_get_threshold() == THR and q2.squelch_get_timeout() == TIMEOUT


@pytest.mark.parametrize("kind", ["crcf", "rrrf"])
def test_init_on_a_block(ya, kind):
    C = 67
    x = ar.streams(37, C, 21, kind)
    q, r = ya.Agc(C, kind), ar.AgcRef(C, kind)
    q.init(x), r.init(x)
    assert ar.same_words(q.get_gain(), r.get_gain())
    xd = ya.DeviceArray.from_numpy(np.ascontiguousarray(x[:20]))
    q.init_devptr(xd.ptr, C, 20), r.init(x[:20])
    xd.free()
    assert ar.same_words(q.get_gain(), r.get_gain())
    y, wy = q.execute_block(x), r.execute_block(x)[0]
    assert ar.same_words(y, wy)


@pytest.mark.parametrize("kind", ["crcf", "rrrf"])
def test_zeros_a_nan_and_an_inf_stay_in_their_columns(ya, kind):
    C, n = 6, 150
    clean = ar.noise(1, n, C, 0.1, kind)
    dirty = clean.copy()
    dirty[:, 1] = 0
    dirty[40, 3] = np.nan
    dirty[60, 4] = np.inf
    outs = []
    for x in (clean, dirty):
        q, r = ya.Agc(C, kind), ar.AgcRef(C, kind)
        configure(q, True), configure(r, True)
        y, st = q.execute_block(x, status=True)
        wy, wst = r.execute_block(x)
        assert ar.same_words(y, wy) and np.array_equal(st, wst)
        assert ar.same_words(q.get_gain(), r.get_gain()) and np.array_equal(q.squelch_get_status(), r.squelch_get_status())
        outs.append((y, q.get_gain()))
    keep = [0, 2, 5]
    assert ar.same_words(outs[0][0][:, keep], outs[1][0][:, keep]) and ar.same_words(outs[0][1][keep], outs[1][1][keep])
    g = outs[1][1]
    assert g[1] == np.float32(1e6), "a channel of zeros ends at the gain limit"
    assert np.isfinite(g[3]) and np.isnan(outs[1][0][41:, 3]).sum() == 0, "the NaN sits in y2' and freezes g"


@pytest.mark.parametrize("kind", ["crcf", "rrrf"])
def test_bad_arguments_on_the_object(ya, kind):
    """every bad argument of agc.rs:505-529 and the stated deviations, on an object; a refused call changes nothing"""
    C = 4
    q = ya.Agc(C, kind)
    q.set_bandwidth(0.1), q.set_scale(2.0), q.set_gain(3.0), q.squelch_set_timeout(7)
    nan = float("nan")
    for call, v in (("set_bandwidth", -1.0), ("set_bandwidth", 2.0), ("set_bandwidth", nan),
                    ("set_gain", 0.0), ("set_gain", -1.0), ("set_gain", nan),
                    ("set_signal_level", 0.0), ("set_signal_level", -1.0), ("set_signal_level", nan),
                    ("set_scale", 0.0), ("set_scale", -1.0), ("set_scale", nan),
                    ("squelch_set_timeout", 0), ("squelch_set_timeout", 1 << 32), ("reset_channel", C),
                    ("set_gains", [1.0, 1.0, 0.0, 1.0]), ("set_gains", [1.0, -1.0, 1.0, 1.0]), ("set_gains", [1.0, 1.0, 1.0]),
                    ("set_locked", [1, 0, 1]), ("init", np.zeros((0, C), q.T)), ("init", np.zeros((3, C + 1), q.T))):
        with pytest.raises(ya.ConfigError):
            getattr(q, call)(v)
    room = ya.DeviceArray(1 << 14, np.uint8)                         # every pointer below lies inside this allocation
    room.zero()
    base, far, plane = room.ptr, room.ptr + (1 << 12), room.ptr + (1 << 13)
    for args in ((base, C, 0), (base, C - 1, 5), (None, C, 5)):      # n = 0; pitch < C; no block
        with pytest.raises(ya.ConfigError):
            q.init_devptr(*args)
    for args in ((base, C - 1, 4, far, C), (base, C, 4, far, C - 1),
                 (base, C, 4, far, C, plane, C - 1),                 # status pitch < C
                 (None, C, 4, far, C), (base, C, 4, None, C),
                 (base, C, 4, base + 8, C),                          # x and y overlap in part
                 (base, C, 4, base, C + 1),                          # the same start at another pitch
                 (base, C, 4, far, C, far + 3, C),                   # the status plane inside y
                 (base, C, 4, far, C, base + 5, C)):                 # the status plane inside x
        with pytest.raises(ya.ConfigError):
            q.execute_block_devptr(*args)
    ya.synchronize()
    assert not room.to_numpy().any(), "a refused call wrote"
    room.free()
    with pytest.raises(ya.ConfigError):
        q.execute_block(np.zeros((3, C + 1), q.T))
    assert q.get_bandwidth() == np.float32(0.1) and q.get_scale() == 2.0 and q.squelch_get_timeout() == 7
    assert (q.get_gain() == 3.0).all() and not q.get_locked().any()
    r = ar.AgcRef(C, kind)
    r.set_bandwidth(0.1), r.set_scale(2.0), r.set_gain(3.0)
    x = ar.streams(12, C, 2, kind)
    assert ar.same_words(q.execute_block(x), r.execute_block(x)[0]), "the refused calls left the object as it was"


def test_the_references_own_tests_on_the_device(ya):
    """agc.rs: dc gain control (:259-287), scale (:289-311), lock (:468-502) and the squelch checkpoints (:412-466), on
    three identical channels"""
    C = 3
    x = np.full((256, C), 0.1, np.complex64)
    q = ya.Agc(C)
    q.set_bandwidth(0.1)
    y = q.execute_block(x)
    assert np.allclose(y[-1].real, 1.0, atol=1e-3) and np.allclose(y[-1].imag, 0.0, atol=1e-3)
    assert np.allclose(q.get_gain(), 10.0, atol=1e-3)
    q.set_gain(1.0)
    assert (q.get_gain() == 1.0).all()

    q = ya.Agc(C)
    q.set_bandwidth(0.1), q.set_scale(4.0)
    y = q.execute_block(x)
    assert q.get_scale() == 4.0 and np.allclose(y[-1].real, 4.0, atol=1e-3) and np.allclose(y[-1].imag, 0.0, atol=1e-3)

    q = ya.Agc(C)
    q.set_bandwidth(0.1), q.set_rssi(0.0)
    assert np.allclose(q.get_rssi(), 0.0, atol=1e-6) and not q.is_locked()
    q.lock()
    assert q.is_locked()
    for _ in range(4):
        q.execute_block(x)
    assert np.allclose(q.get_rssi(), 0.0, atol=1e-6)
    q.unlock()
    assert not q.is_locked()
    q.init(x[:4])
    assert np.allclose(q.get_rssi(), 20.0 * np.log10(np.float32(0.1)), atol=1e-2)

    q = ya.Agc(C)
    q.set_bandwidth(0.25), q.set_signal_level(1e-3)
    assert not q.squelch_is_enabled()
    q.squelch_enable(), q.squelch_set_threshold(-50.0), q.squelch_set_timeout(100)
    s = np.repeat(ar.squelch_stimulus()[:, None], C, axis=1)
    _, st = q.execute_block(s, status=True)
    M = ya.AgcSquelchMode
    for i, mode in ((0, M.ENABLED), (500, M.ENABLED), (600, M.SIGNALHI), (1400, M.SIGNALHI), (1500, M.SIGNALLO),
                    (1600, M.ENABLED), (1900, M.ENABLED)):
        assert (st[i] == int(mode)).all(), (i, st[i])
