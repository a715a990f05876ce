"""tests/agc_ref.py against the reference's own nine tests (src/agc/agc.rs:259-557, at their tolerances, randnf replaced by
a seeded generator), the squelch coverage of the stimuli the GPU tests use, and the loop on the platform's logf / expf /
log10f against the loop on the library's words."""
import numpy as np
import pytest

import agc_ref as ar

F = np.float32


def polar(r, theta):
    return complex(F(r) * np.cos(F(theta), dtype=F), F(r) * np.sin(F(theta), dtype=F))


def test_dc_gain_control():
    q = ar.AgcScalar()
    q.set_bandwidth(0.1)
    for _ in range(256):
        y = q.execute(complex(F(0.1), 0))
    assert abs(y.real - 1.0) <= 1e-3 and abs(y.imag) <= 1e-3 and abs(q.g - 10.0) <= 1e-3
    q.set_gain(1.0)
    assert q.g == 1.0


def test_scale():
    q = ar.AgcScalar()
    q.set_bandwidth(0.1), q.set_scale(4.0)
    assert q.scale == 4.0
    for _ in range(256):
        y = q.execute(complex(F(0.1), 0))
    assert abs(y.real - 4.0) <= 1e-3 and abs(y.imag) <= 1e-3


def test_ac_gain_control():
    q = ar.AgcScalar()
    q.set_bandwidth(0.1)
    for i in range(256):
        z = polar(1.0, F(i) * F(0.1))
        q.execute(complex(F(0.1) * F(z.real), F(0.1) * F(z.imag)))
    assert abs(q.g - 10.0) <= 1e-3


def test_rssi_sinusoid():
    q = ar.AgcScalar()
    q.set_bandwidth(0.05)
    for i in range(512):
        z = polar(1.0, F(0.1) * F(i))
        q.execute(complex(F(0.3) * F(z.real), F(0.3) * F(z.imag)))
    assert abs(q.get_signal_level() - F(0.3)) <= 1e-3


def test_rssi_noise():
    q = ar.AgcScalar()
    q.set_bandwidth(2e-3)
    nstd = 10.0 ** (-30.0 / 20.0)
    for v in ar.noise(1, 8000, 1, nstd)[:, 0]:
        q.execute(v)
    assert abs(q.get_rssi() - (-30.0)) <= 1.0


CHECKPOINTS = ((0, ar.ENABLED), (500, ar.ENABLED), (600, ar.SIGNALHI), (1400, ar.SIGNALHI), (1500, ar.SIGNALLO),
               (1600, ar.ENABLED), (1900, ar.ENABLED))


def squelch_run(words):
    q = ar.AgcScalar(words=words)
    q.set_bandwidth(0.25), q.set_signal_level(1e-3)
    assert q.squelch_mode == ar.DISABLED
    q.squelch_enable()
    q.squelch_threshold = F(-50.0)
    q.squelch_set_timeout(100)
    modes = []
    for v in ar.squelch_stimulus():
        q.execute(v)
        modes.append(q.squelch_mode)
    return modes


def test_squelch_checkpoints():
    modes = squelch_run(ar.OWN)
    for i, want in CHECKPOINTS:
        assert modes[i] == want, (i, modes[i])


def test_lock():
    q = ar.AgcScalar()
    q.set_bandwidth(0.1)
    buf = [complex(F(0.1), 0)] * 4
    q.set_rssi(0.0)
    assert abs(q.get_rssi()) <= 1e-6 and not q.is_locked
    q.is_locked = True
    for _ in range(256):
        for v in buf:
            assert q.execute(v) == complex(F(0.1) * q.g, 0)         # locked: not scaled, g frozen
    assert abs(q.get_rssi()) <= 1e-6
    q.is_locked = False
    q.init(buf)
    assert abs(q.get_rssi() - 20.0 * np.log10(F(0.1))) <= 1e-2


def test_invalid_config():
    q = ar.AgcScalar()
    for call, v in (("set_bandwidth", -1.0), ("set_bandwidth", 2.0), ("set_gain", 0.0), ("set_gain", -1.0),
                    ("set_signal_level", 0.0), ("set_signal_level", -1.0), ("set_scale", 0.0), ("set_scale", -1.0),
                    ("init", []), ("squelch_set_timeout", 0)):
        with pytest.raises(ar.ConfigError):
            getattr(q, call)(v)


def test_copy():
    x = ar.noise(4, 64, 1)[:, 0]
    q0 = ar.AgcRef(1)
    q0.set_bandwidth(0.01234)
    q0.execute_block(x[:32, None])
    q1 = q0.clone()
    assert ar.same_words(q0.execute_block(x[32:, None])[0], q1.execute_block(x[32:, None])[0])


def test_the_gpu_stimuli_walk_every_edge_of_the_squelch_machine():
    import test_gpu_agc as t
    edges = set()
    for kind in ("crcf", "rrrf"):
        x = ar.streams(t.N, 65, 100 + 65, kind)
        r = ar.AgcRef(65, kind)
        t.configure(r, True)
        r.execute_block(x, edges)
    e, r_, hi, f, lo, to = ar.ENABLED, ar.RISE, ar.SIGNALHI, ar.FALL, ar.SIGNALLO, ar.TIMEOUT
    assert edges == {(e, e), (e, r_), (r_, hi), (r_, f), (hi, hi), (hi, f), (f, hi), (f, lo), (lo, to), (lo, hi), (lo, lo),
                     (to, e)}


def test_one_row_stimulus_visits_all_enabled_modes():
    x = ar.hopping(1, 200, 8)
    r = ar.AgcRef(8)
    r.set_bandwidth(0.25), r.set_gain(1000.0), r.squelch_enable(), r.squelch_set_threshold(-50.0), r.squelch_set_timeout(5)
    _, st = r.execute_block(x)
    assert set(np.unique(st)) == {ar.ENABLED, ar.RISE, ar.SIGNALHI, ar.FALL, ar.SIGNALLO, ar.TIMEOUT}


# ---- the platform's libm in place of the library's words ---------------------------------------------------------------
ULP_BOUND = 8      # four times the largest distance measured (2 ulp)


def ulps(a, b):
    a, b = np.asarray(a, F).view(np.int32).astype(np.int64), np.asarray(b, F).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def test_libm_squelch_sequence_is_identical():
    assert squelch_run(ar.libm_words()) == squelch_run(ar.OWN)


@pytest.mark.parametrize("bw", [1e-3, 1e-2, 0.1, 0.5, 1.0])
def test_libm_gain_stays_within_the_bound(bw):
    libm = ar.libm_words()
    worst = 0
    for seed, amp in ((1, 0.03), (2, 1.0), (3, 40.0)):
        a, b = ar.AgcScalar(words=ar.OWN), ar.AgcScalar(words=libm)
        a.set_bandwidth(bw), b.set_bandwidth(bw)
        for v in ar.noise(seed, 4000, 1, amp)[:, 0]:
            a.execute(v), b.execute(v)
            worst = max(worst, int(ulps(a.g, b.g)))
    print(f"bandwidth {bw}: g on the platform's libm within {worst} ulp of g on the library's words")
    assert worst <= ULP_BOUND
