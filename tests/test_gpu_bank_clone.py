"""A clone of a channel-bank object (SymSync, EqLms, EqRls, Agc, SymTrack, Channel) carries every setting and the whole
state: with every setter of the Python class moved off its default and one block run, each getter of the clone gives
the original's words, and a second block gives the same words from both.  C = 3 at the smallest designs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C, ROWS = 3, 24
QPSK = (np.array([1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j]) * np.sqrt(0.5)).astype(np.complex64)


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def block(seed, real=False):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((ROWS, C)) + 1j * g.standard_normal((ROWS, C))) * 0.5
    return x.real.astype(np.float32) if real else x.astype(np.complex64)


def symsync(ya):
    q = ya.SymSync.rnyquist(C, ya.FirFilterShape.Arkaiser, 2, 2, 0.3, 4)
    q.set_output_rate(2)
    q.set_lf_bw(0.05)
    q.lock()
    get = lambda o: [o.is_locked(), o.k_out, o.branch_length, o.get_tau(), o.get_stalled()]
    return q, get, lambda o, x: o.execute(x)


def eqlms(ya):
    q = ya.EqLms(C, 3)
    q.set_bw(0.3)
    q.set_constellation(QPSK)
    get = lambda o: [o.get_bw(), o.get_length(), o.get_coefficients(), o.get_weights()]
    return q, get, lambda o, x: o.decim_block(2, ya.EqLmsUpdate.DECISION, x)


def eqrls(ya):
    q = ya.EqRls(C, 3)
    planned, _, admissible = ya.eqrls_plan(C, 3)
    q.set_lanes(next(L for L in admissible if L != planned))
    assert q.get_lanes() != planned
    q.set_bw(0.95)
    q.set_constellation(QPSK)
    get = lambda o: [o.get_bw(), o.get_length(), o.get_lanes(), o.get_coefficients(), o.get_weights(), o.get_matrix()]
    return q, get, lambda o, x: o.step_block(2, ya.EqRlsUpdate.DECISION, x)


def agc(ya, kind):
    q = ya.Agc(C, kind)
    q.set_bandwidth(0.05)
    q.set_scale(0.7)
    q.set_gain(3.0)
    q.set_signal_level(0.25)
    q.set_rssi(-6.0)
    q.set_gains([0.5, 2.0, 4.0])
    q.lock()
    q.unlock()
    q.set_locked([1, 0, 0])
    q.squelch_enable()
    q.squelch_set_threshold(-20.0)
    q.squelch_set_timeout(7)
    get = lambda o: [o.is_locked(), o.get_locked(), o.get_bandwidth(), o.get_scale(), o.get_gain(), o.get_signal_level(),
                     o.get_rssi(), o.squelch_is_enabled(), o.squelch_get_threshold(), o.squelch_get_timeout(),
                     o.squelch_get_status()]
    return q, get, lambda o, x: o.execute_block(x.real.copy() if kind == "rrrf" else x, status=True)


def symtrack(ya):
    q = ya.SymTrack(C, ya.FirFilterShape.Arkaiser, 2, 2, 0.3, ya.ModulationScheme.Qpsk, ya.OscScheme.Nco, 4, 3)
    q.set_bandwidth(0.5)
    q.set_bandwidths(0.03, 0.002, 0.03, 0.002)
    q.set_eq_strategy(ya.SymTrackEq.DD)
    q.set_eq_holdoff(5)
    q.set_nco_all([0.01, -0.02, 0.03], [0.1, 0.2, 0.3])
    q.set_nco(1, 0.015, -0.4)
    get = lambda o: [o.get_bandwidth(), o.get_tau(), o.get_gain(), o.get_rssi(), o.get_nco_frequency(), o.get_nco_phase(),
                     *o.get_nco_state(), o.get_weights(), o.get_num_syms(), o.get_stalled()]
    return q, get, lambda o, x: o.execute(x)


def channel(ya):
    q = ya.Channel(C, 3)
    q.set_seed(41)
    q.set_awgn(0, -30.0, 20.0)
    q.set_awgn_all([-30.0, -40.0, -50.0], [20.0, 10.0, 30.0])
    q.set_gain_noise(1, 0.8, 0.02)
    q.set_gain_noise_all([0.9, 0.8, 1.1], [0.01, 0.02, 0.03])
    q.set_carrier_offset(2, 0.05, 0.3)
    q.set_carrier_offset_all([0.01, -0.02, 0.03], [0.1, 0.2, 0.3])
    g = np.random.default_rng(7)
    h = (g.standard_normal((C, 3)) + 1j * g.standard_normal((C, 3))).astype(np.complex64)
    q.set_multipath(0, h[1])
    q.set_multipath_all(h)
    q.set_position(0, 5)
    q.set_position_all([1 << 33, 17, 3])
    planned = q.get_shape(ROWS)
    forced = (2, 2) if (planned["links"], planned["rows"]) != (2, 2) else (4, 1)
    q.set_shape(*forced)
    assert (q.get_shape(ROWS)["links"], q.get_shape(ROWS)["rows"]) == forced
    get = lambda o: [o.get_multipath(), o.get_seed(), o.get_position(), *o.get_gain_noise(), *o.get_osc_state(),
                     sorted(o.get_shape(ROWS).items())]
    return q, get, lambda o, x: o.execute(x)


BANKS = {"symsync": symsync, "eqlms": eqlms, "eqrls": eqrls, "agc_crcf": lambda ya: agc(ya, "crcf"),
         "agc_rrrf": lambda ya: agc(ya, "rrrf"), "symtrack": symtrack, "channel": channel}


def words(values):
    """every value as its bytes, so NaN compares equal to itself and -0.0 differs from 0.0"""
    values = values if isinstance(values, (list, tuple)) else [values]
    return [None if v is None else repr(v) if isinstance(v, list) else np.asarray(v).tobytes() for v in values]


@pytest.mark.parametrize("name", list(BANKS))
def test_a_clone_carries_every_setting_and_the_state(ya, name):
    q, get, run = BANKS[name](ya)
    first = run(q, block(1))
    assert any(np.asarray(v).any() for v in (first if isinstance(first, tuple) else [first]) if v is not None)
    r = q.clone()
    assert words(get(r)) == words(get(q))
    x = block(2)
    assert words(run(r, x)) == words(run(q, x))
    assert words(get(r)) == words(get(q))
