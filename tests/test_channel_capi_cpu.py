"""Channel through the C ABI without a GPU: execute_host (the library's definition on the host) and the array forms of
the words equal tests/channel_ref.py bit for bit, and the argument checks of create, the plan and execute_host answer
before any device is asked for.  The setters need a built object, and an object needs a device: their config errors are
in tests/test_gpu_channel.py."""
import re

import numpy as np
import pytest

import channel_ref as cr
from conftest import ROOT, has_gpu

import yagi_amd as ya

F = np.float32


def ref_and_words(C_, L, vco, seed=41):
    r = cr.ChannelRef(C_, L, vco)
    cr.configure(r, C_, L)
    r.seed = seed
    r.set_position(C_ - 1, (1 << 40) + 3)
    return r, r.words()


@pytest.mark.parametrize("vco", [False, True])
@pytest.mark.parametrize("C_,L", [(1, 1), (3, 2), (7, 17), (2, cr.TAPS_MAX)])
def test_execute_host_equals_the_restatement(C_, L, vco):
    n, pad = 90, 3
    x = cr.streams(n, C_, 11 + L)
    r, words = ref_and_words(C_, L, vco)
    want = r.execute_block(x)
    assert cr.same_words(want, ref_and_words(C_, L, vco)[0].execute_seq(x))
    scheme = ya.OscScheme.Vco if vco else ya.OscScheme.Nco
    wide = np.full((n, C_ + pad), 9, np.complex64)
    wide[:, :C_] = x
    y0 = np.full((n, C_ + pad + 1), 7, np.complex64)
    y = ya.Channel.execute_host(*words, wide, osc_scheme=scheme, seed=41, x_pitch=C_ + pad, y_pitch=C_ + pad + 1, y=y0)
    assert cr.same_words(y[:, :C_], want)
    assert (y[:, C_:] == 7).all(), "a gap column of y was written"
    assert cr.same_words(ya.Channel.execute_host(*words, x, osc_scheme=scheme, seed=41), want)


@pytest.mark.parametrize("vco", [False, True])
def test_execute_host_bcast(vco):
    C_, L, n = 5, 6, 70
    x = cr.streams(n, 1, 2)[:, 0]
    r, words = ref_and_words(C_, L, vco)
    want = r.execute_block(x)
    y = ya.Channel.execute_host(*words, x, osc_scheme=ya.OscScheme(int(vco)), seed=41, bcast=True, y_pitch=C_ + 2)
    assert cr.same_words(y[:, :C_], want) and (y[:, C_:] == 0).all()


def test_execute_host_n0_and_nonfinite_samples():
    C_, L = 3, 4
    r, words = ref_and_words(C_, L, False)
    assert ya.Channel.execute_host(*words, np.zeros((0, C_), np.complex64), seed=41).shape == (0, C_)
    x = cr.streams(30, C_, 3)
    x[5, 1], x[9, 2] = np.nan, np.inf
    y = ya.Channel.execute_host(*words, x, seed=41)
    assert cr.same_words(y, r.execute_block(x))
    clean = x.copy()
    clean[5, 1] = clean[9, 2] = 0
    yc = ya.Channel.execute_host(*words, clean, seed=41)
    diff = y.view(np.uint32).reshape(30, C_, 2) != yc.view(np.uint32).reshape(30, C_, 2)
    rows1, rows2 = np.flatnonzero(diff[:, 1].any(axis=1)), np.flatnonzero(diff[:, 2].any(axis=1))
    assert not diff[:, 0].any() and set(rows1) <= set(range(5, 5 + L)) and set(rows2) <= set(range(9, 9 + L))
    assert np.isnan(y[5:5 + L, 1]).all()


def test_the_words_on_arrays():
    k2 = np.concatenate([np.arange(0, 1 << 24, 4099), [0, 1 << 22, 1 << 23, 3 << 22, (1 << 24) - 1, (1 << 21) - 1, 1 << 21]])
    c, s = ya.channel_cos_sin(k2)
    wc, ws = cr.cos_sin64(k2)
    assert np.array_equal(c.view(np.uint64), wc.view(np.uint64)) and np.array_equal(s.view(np.uint64), ws.view(np.uint64))
    k1 = np.concatenate([np.arange(1, (1 << 24) + 1, 4099), [1, 2, 1 << 23, (1 << 24) - 1, 1 << 24]])
    assert cr.same_words(ya.channel_radius(k1), cr.radius(k1))
    for seed, link, first in ((0, 0, 0), (2 ** 64 - 1, 5, (1 << 32) - 3), (12345, 1 << 19, (1 << 63) + 9)):
        got = ya.channel_noise(seed, link, first, 300)
        re, im = cr.noise(seed, link, (np.arange(300, dtype=np.uint64) + np.uint64(first)))
        assert cr.same_words(got.real.copy(), re) and cr.same_words(got.imag.copy(), im)


def test_cos_sin_words_of_the_library_on_all_arguments():
    for lo in range(0, 1 << 24, 1 << 22):
        k2 = np.arange(lo, lo + (1 << 22), dtype=np.int64)
        c, s = ya.channel_cos_sin(k2)
        wc, ws = cr.cos_sin64(k2)
        assert np.array_equal(c.view(np.uint64), wc.view(np.uint64)) and np.array_equal(s.view(np.uint64), ws.view(np.uint64))


@pytest.mark.parametrize("n0,snr", [(0.0, 0.0), (-20.0, 10.0), (-37.5, 3.25), (6.0, -12.0), (-200.0, 30.0), (np.nan, 1.0)])
def test_awgn_words(n0, snr):
    g, s = ya.channel_awgn_words(n0, snr)
    wg, ws = cr.awgn_words(n0, snr)
    assert cr.same_words(np.array([g, s], F), np.array([wg, ws], F)), (g, s, wg, ws)
    if n0 == 0.0 and snr == 0.0:
        assert g == 1 and s == 1


def test_constrain_is_oscs():
    import osc_ref as orf
    for v in (0.0, 0.37, -0.37, 6.28, 7.0, -3.1415927, 99.0):
        assert ya.channel_constrain(v) == orf.constrain(v)
    with pytest.raises(ya.ConfigError):
        ya.channel_constrain(float("inf"))


def test_the_plan_and_the_header_constants():
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    assert int(re.search(r"#define YAGI_CHANNEL_CHANNELS_MAX (\d+)", hdr).group(1)) == ya.CHANNEL_CHANNELS_MAX == cr.CHANNELS_MAX
    assert int(re.search(r"#define YAGI_CHANNEL_TAPS_MAX (\d+)", hdr).group(1)) == ya.CHANNEL_TAPS_MAX == cr.TAPS_MAX >= 32
    assert float.fromhex(re.search(r"#define YAGI_CHANNEL_COSSIN_E (\S+)", hdr).group(1)) == ya.CHANNEL_COSSIN_E == cr.COSSIN_E
    assert cr.COSSIN_E <= 2.0 ** -40
    for channels, wide in ((1, 1), (3, 4), (64, 64), (65, 64), (1 << 20, 64)):
        for L, deep in ((1, 2), (2, 4), (8, 16), (17, 64), (32, 64), (cr.TAPS_MAX, 128)):
            links = min(wide, max(8, 256 // deep))            # as wide as the bank, twice as deep as the taps, 8 links at least
            for bcast in (False, True):
                p = ya.channel_plan(channels, L, 100000, ya.OscScheme.Vco, bcast)
                assert (p["links"], p["rows"]) == (links, 8), (channels, L, p)
                assert p["tile_steps"] == 256 // links * 8 >= 4 * L and p["lds_bytes"] <= 64 * 1024
    assert ya.channel_plan(1, 1, 0)["rows"] == 1 and ya.channel_plan(64, 1, 5)["rows"] == 2
    assert ya.channel_plan(64, 1, 4)["rows"] == 1 and ya.channel_plan(64, 1, 17)["rows"] == 8


BAD_CREATE = [(0, 1, 0), (ya.CHANNEL_CHANNELS_MAX + 1, 1, 0), (1, 0, 0), (1, ya.CHANNEL_TAPS_MAX + 1, 0), (1, 1, 2), (1, 1, -1)]


@pytest.mark.parametrize("channels,L,scheme", BAD_CREATE)
def test_create_config_errors_need_no_device(channels, L, scheme):
    with pytest.raises(ya.ConfigError):
        ya.Channel(channels, L, scheme)
    with pytest.raises(ya.ConfigError):
        ya.channel_plan(channels, L, 10, scheme)


def test_execute_host_config_errors():
    r, words = ref_and_words(2, 3, False)
    x = cr.streams(8, 2, 1)
    with pytest.raises(ya.ConfigError):                       # a pitch below channels
        ya.Channel.execute_host(*words, np.zeros((8, 1), np.complex64), x_pitch=1)
    with pytest.raises(ya.ConfigError):
        ya.Channel.execute_host(*words, x, y_pitch=1)
    with pytest.raises(ya.ConfigError):                       # x and y overlap
        ya.Channel.execute_host(*words, x, y=x)
    with pytest.raises(ya.ConfigError):                       # taps beyond the limit
        ya.Channel.execute_host(np.zeros((2, cr.TAPS_MAX + 1), np.complex64), *words[1:], x)
    with pytest.raises(ya.ConfigError):
        ya.Channel.execute_host(*words, x, osc_scheme=3)


@pytest.mark.skipif(has_gpu(), reason="the answer without a device")
def test_a_valid_create_without_a_device_is_a_device_error():
    with pytest.raises(ya.DeviceError):
        ya.Channel(4, 3)
