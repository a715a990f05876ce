"""Agc through the C ABI without a GPU: execute_host (the library's definition on the host) equals tests/agc_ref.py bit
for bit, the argument checks answer before any device is asked for, and the header's constants equal the Python enum."""
import re

import numpy as np
import pytest

import agc_ref as ar
from conftest import ROOT, has_gpu

import yagi_amd as ya


def restate(kind, C, bw, scale, g0, locked, squelch, thr, timeout, x):
    r = ar.AgcRef(C, kind)
    r.set_bandwidth(bw), r.set_scale(scale)
    r.squelch_set_threshold(thr), r.squelch_set_timeout(timeout)
    if squelch:
        r.squelch_enable()
    r.reset()
    r.set_gain(g0)
    if locked:
        r.lock()
    y, st = r.execute_block(x)
    return y, st, r.get_gain(), r.squelch_get_status()


@pytest.mark.parametrize("kind", ["crcf", "rrrf"])
@pytest.mark.parametrize("bw", [0.0, 0.01, 0.25, 1.0])
@pytest.mark.parametrize("locked,squelch", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_execute_host_equals_the_restatement(kind, bw, locked, squelch):
    C, n, pad = 7, 120, 3
    x = ar.streams(n, C, 11, kind)
    g0, thr, timeout, scale = 30.0, -50.0, 5, 1.5
    want = restate(kind, C, bw, scale, g0, locked, squelch, thr, timeout, x)
    wide = np.full((n, C + pad), 9, x.dtype)
    wide[:, :C] = x
    y0 = np.full((n, C + pad + 1), 7, x.dtype)
    y, st, g, mode = ya.Agc.execute_host(C, bw, scale, g0, locked, squelch, thr, timeout, wide, kind=kind, status=True,
                                         x_pitch=C + pad, y_pitch=C + pad + 1, status_pitch=C + 2, y=y0)
    assert ar.same_words(y[:, :C], want[0])
    assert (y[:, C:] == 7).all(), "a gap column of y was written"
    assert np.array_equal(st[:, :C], want[1]) and (st[:, C:] == 0).all()
    assert ar.same_words(g, want[2]) and np.array_equal(mode, want[3])
    if not squelch:
        assert (st == 0).all() and (mode == 0).all()


@pytest.mark.parametrize("kind", ["crcf", "rrrf"])
def test_alpha_zero_and_an_inf_sample(kind):
    """0 Inf is a NaN: it lands in y2', the gate `y2' > 1e-6` stays shut and g is frozen where it was.  (minNum's NaN
    branch, g = 1e6, would need ln(y2') = Inf at alpha = 0, and at alpha = 0 y2' can only stay or turn NaN.)"""
    x = np.ones((6, 2), ya.KINDS[kind][0])
    x[2, 1] = np.inf
    want = restate(kind, 2, 0.0, 1.0, 2.0, 0, 1, 0.0, 100, x)
    y, st, g, mode = ya.Agc.execute_host(2, 0.0, 1.0, 2.0, 0, 1, 0.0, 100, x, kind=kind, status=True)
    assert ar.same_words(y, want[0]) and np.array_equal(st, want[1]) and ar.same_words(g, want[2])
    assert g[0] == np.float32(2.0) and g[1] == np.float32(2.0)


def test_in_place_on_the_host_equals_out_of_place():
    x = ar.streams(50, 5, 3)
    y, _, g, _ = ya.Agc.execute_host(5, 0.1, 1.0, 1.0, 0, 0, 0.0, 100, x)
    z = x.copy()
    y2, _, g2, _ = ya.Agc.execute_host(5, 0.1, 1.0, 1.0, 0, 0, 0.0, 100, z, y=z)
    assert y2 is z and ar.same_words(y, z) and ar.same_words(g, g2)


def host(**kw):
    a = dict(channels=4, bandwidth=0.1, scale=1.0, g0=1.0, locked=0, squelch=1, threshold=0.0, timeout=100,
             x=np.ones((8, 4), np.complex64))
    a.update(kw)
    return ya.Agc.execute_host(**a)


@pytest.mark.parametrize("bad", [dict(bandwidth=-1.0), dict(bandwidth=2.0), dict(bandwidth=float("nan")), dict(g0=0.0),
                                 dict(g0=-1.0), dict(scale=0.0), dict(scale=-1.0), dict(timeout=0), dict(timeout=1 << 32),
                                 dict(channels=0, x=np.ones((8, 0), np.complex64)),
                                 dict(x=np.ones((8, 3), np.complex64), x_pitch=3), dict(y_pitch=3),
                                 dict(status=True, status_pitch=3)])
def test_bad_arguments_are_config_errors(bad):
    host()
    with pytest.raises(ya.ConfigError):
        host(**bad)


def test_partial_overlap_is_a_config_error():
    buf = np.ones((9, 4), np.complex64)
    with pytest.raises(ya.ConfigError):
        host(x=buf[:8], y=buf[1:])                                  # shifted by one row
    wide = np.ones((8, 6), np.complex64)
    with pytest.raises(ya.ConfigError):                             # the same start at another pitch
        fn = ya.lib.yagi_hip_agc_crcf_execute_host
        ya._check(fn(4, 0.1, 1.0, 1.0, 0, 0, 0.0, 100, wide.ctypes.data, 6, 8, wide.ctypes.data, 5, None, 0, None, None))
    y = np.zeros((8, 4), np.complex64)                             # the status plane inside y, and inside x
    for plane in (y.ctypes.data + 3, wide.ctypes.data + 5):
        with pytest.raises(ya.ConfigError):
            ya._check(fn(4, 0.1, 1.0, 1.0, 0, 0, 0.0, 100, wide.ctypes.data, 6, 8, y.ctypes.data, 4, plane, 4, None, None))
    with pytest.raises(ya.ConfigError):                             # n is below 2^31; refused before a sample is read
        ya._check(fn(4, 0.1, 1.0, 1.0, 0, 0, 0.0, 100, wide.ctypes.data, 6, 1 << 31, y.ctypes.data, 4, None, 0, None, None))


@pytest.mark.parametrize("kind", ["crcf", "rrrf"])
def test_the_constructor_checks_before_the_device(kind):
    """with or without a GPU; the object's setters are checked where an object can be built (tests/test_gpu_agc.py)"""
    with pytest.raises(ya.ConfigError):
        ya.Agc(0, kind)
    with pytest.raises(ya.ConfigError):
        ya.Agc(ya.AGC_CHANNELS_MAX + 1, kind)
    with pytest.raises(ya.ConfigError):
        ya.Agc(4, "cccf")


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
@pytest.mark.parametrize("kind", ["crcf", "rrrf"])
def test_create_without_a_gpu_is_a_device_error(kind):
    with pytest.raises(ya.DeviceError):
        ya.Agc(4, kind)


def test_the_headers_constants_equal_the_enum():
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    body = re.search(r"enum \{\s*YAGI_AGC_SQUELCH_DISABLED = 0,([^}]*)\}", hdr).group(1)
    names = ["DISABLED"] + [m for m in re.findall(r"YAGI_AGC_SQUELCH_(\w+)", body)]
    assert names == [m.name for m in ya.AgcSquelchMode] and [int(m) for m in ya.AgcSquelchMode] == list(range(7))
    assert (ar.DISABLED, ar.ENABLED, ar.RISE, ar.SIGNALHI, ar.FALL, ar.SIGNALLO, ar.TIMEOUT) == tuple(range(7))
    assert int(re.search(r"#define YAGI_AGC_CHANNELS_MAX (\d+)", hdr).group(1)) == ya.AGC_CHANNELS_MAX == ar.CHANNELS_MAX
