"""The bank kernels' row chunking (yagi_amd/csrc/bank_lane.hpp): two consecutive device-pointer calls whose lengths sit at
the seams of the row queue, against the Python restatements word for word, outputs and every getter.

A kernel requests its rows a chunk of A ahead; A is that kernel's constant in kernels.hpp, named at each test.  Call
lengths (n1, n2) are drawn from {0, 1, A - 1, A, A + 1, 2 A + 1} so that a call is empty, shorter than a chunk, ends on a
chunk's last row, starts a chunk of one row, or spans three chunks, and the second call reads the window the first left.
The designs are small: rings of length 1 (EqLms h_len = 1, EqRls p = 1), rings longer than both calls together (the pair
(1, 1)) and calls of at least three ring lengths (the pair (2 A + 1, 2 A + 1)).  C = 1 is one lane of one wave, C = 65 one
lane of a second workgroup."""
import numpy as np
import pytest

import agc_ref as ar
import eqlms_ref as er
import eqrls_ref as rr
import symsync_ref as ss
import symtrack_ref as st

pytestmark = pytest.mark.gpu

CHANNELS = [1, 65]


def pairs(A):
    """(n1, n2): every length of {0, 1, A - 1, A, A + 1, 2 A + 1} as the first and as the second call, two empty calls and
    two calls of exactly one chunk"""
    return [(0, A + 1), (1, 1), (A - 1, A), (A, A - 1), (A + 1, 0), (2 * A + 1, 2 * A + 1), (0, 0), (A, A)]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def halves(x, n1, n2):
    return x[:n1], x[n1:n1 + n2]


# ---- SymSync: kSymsyncAhead = 16 ------------------------------------------------------------------------------------------
SS_K, SS_M, SS_NPFB = 2, 2, 8                                # 8 taps per branch: the ring has 8 slots


@pytest.mark.parametrize("n1,n2", pairs(16))
@pytest.mark.parametrize("C", CHANNELS)
def test_symsync(ya, C, n1, n2):
    h = ya.SymSync.rnyquist_taps(ya.FirFilterShape.Arkaiser, SS_K, SS_M, 0.35, SS_NPFB)
    q, r = ya.SymSync(C, SS_K, SS_NPFB, h), ss.SymSyncRef(C, SS_K, SS_NPFB, h)
    assert q.branch_length == 2 * SS_K * SS_M
    x = ss.streams(SS_K, max(n1 + n2, 1), C, 11 + C)              # the stimulus has no empty form
    for part in halves(x, n1, n2):
        room = ss.default_ycap(len(part), SS_K, 1)
        want = r.execute(part, room)
        assert ss.same_outputs(ss.run_dev(ya, q, part, room), want), (C, n1, n2, len(part))
        assert ss.same_words(q.get_tau(), r.get_tau())
        assert np.array_equal(q.get_stalled(), want[2]) and not want[2].any()
        assert not q.is_locked()                                   # get_tau, get_stalled and is_locked are all it has


# ---- EqLms: kEqlmsAhead = 16 rows, kEqlmsAheadD = 8 rows of known symbols ------------------------------------------------
def eqlms_pair(ya, C, h_len):
    q, r = ya.EqLms(C, h_len), er.EqLmsRef(C, h_len)
    for o in (q, r):
        o.set_bw(0.1)
    return q, r


def eqlms_same(q, r):
    return er.same_words(q.get_coefficients(), r.get_coefficients()) and er.same_words(q.get_weights(), r.get_weights())


@pytest.mark.parametrize("n1,n2", pairs(16))
@pytest.mark.parametrize("h_len", [1, 5])
@pytest.mark.parametrize("C", CHANNELS)
def test_eqlms_execute_block(ya, C, h_len, n1, n2):
    q, r = eqlms_pair(ya, C, h_len)
    x = er.noise(21 + C, n1 + n2, C, np.array([0.5, 2.0, 1.0])[np.arange(C) % 3])
    for part in halves(x, n1, n2):
        want = r.execute_block(1, part)
        assert er.same_words(er.run_dev(ya, q, 1, part), want), (C, h_len, n1, n2, len(part))
        assert eqlms_same(q, r)


#                                      rows of the set, one symbol each     7, 8, 9 and 17 symbols of two rows
@pytest.mark.parametrize("k,n1,n2", [(1, a, b) for a, b in pairs(16)] + [(2, 14, 18), (2, 16, 34), (2, 18, 16), (2, 34, 14)])
@pytest.mark.parametrize("h_len", [1, 5])
@pytest.mark.parametrize("C", CHANNELS)
def test_eqlms_decim_block_train(ya, C, h_len, k, n1, n2):
    q, r = eqlms_pair(ya, C, h_len)
    x = er.noise(31 + C, n1 + n2, C, np.array([0.5, 2.0, 1.0])[np.arange(C) % 3])
    d = er.symbols((n1 + n2) // k, C, 3)
    for xs, ds in zip(halves(x, n1, n2), halves(d, n1 // k, n2 // k)):
        want = r.decim_block(k, er.TRAIN, xs, ds)
        assert er.same_words(er.run_dev(ya, q, k, xs, er.TRAIN, ds), want), (C, h_len, k, n1, n2, len(xs))
        assert eqlms_same(q, r)


# ---- EqRls: kEqrlsAhead = 8 -------------------------------------------------------------------------------------------------
def eqrls_dev(ya, q, x, d):
    """step_block_devptr in TRAIN, one row per symbol, on plain device buffers"""
    n, C = x.shape
    xd = ya.DeviceArray.from_numpy(x) if n else ya.DeviceArray(1, np.complex64)
    dd = ya.DeviceArray.from_numpy(d) if n else ya.DeviceArray(1, np.complex64)
    yd = ya.DeviceArray(max(n, 1) * C, np.complex64)
    yd.zero()
    q.step_block_devptr(1, int(rr.TRAIN), xd.ptr, C, n, dd.ptr, C, yd.ptr, C)
    ya.synchronize()
    y = yd.to_numpy()[:n * C].reshape(n, C).copy()
    for b in (xd, dd, yd):
        b.free()
    return y


@pytest.mark.parametrize("n1,n2", pairs(8))
@pytest.mark.parametrize("p,L", [(1, 1), (4, 1), (4, 2)])     # 2 lanes per channel are admissible from p = 2
@pytest.mark.parametrize("C", CHANNELS)
def test_eqrls_train(ya, C, p, L, n1, n2):
    q, r = ya.EqRls(C, p), rr.EqRlsRef(C, p)
    q.set_lanes(L)
    assert q.get_lanes() == L
    x = np.ascontiguousarray(er.noise(41 + C, n1 + n2, C, np.array([0.5, 2.0, 1.0])[np.arange(C) % 3]))
    d = np.ascontiguousarray(er.symbols(n1 + n2, C, 5))
    for xs, ds in zip(halves(x, n1, n2), halves(d, n1, n2)):
        want = r.step_block(1, rr.TRAIN, xs, ds)
        got = eqrls_dev(ya, q, np.ascontiguousarray(xs), np.ascontiguousarray(ds))
        assert rr.same_words(got, want), (C, p, L, n1, n2, len(xs))
        assert rr.state_same(q, r)


# ---- Agc: kAgcAhead = 8 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", pairs(8))
@pytest.mark.parametrize("C", CHANNELS)
def test_agc_crcf_with_status(ya, C, n1, n2):
    q, r = ya.Agc(C, "crcf"), ar.AgcRef(C, "crcf")
    for o in (q, r):
        o.set_bandwidth(0.25), o.set_gain(100.0), o.squelch_enable(), o.squelch_set_threshold(-30.0), o.squelch_set_timeout(3)
    x = ar.hopping(51 + C, n1 + n2, C, "crcf")
    for part in halves(x, n1, n2):
        wy, wst = r.execute_block(part)
        y, status = ar.run_dev(ya, q, part, status=True)
        assert ar.same_words(y, wy) and np.array_equal(status, wst), (C, n1, n2, len(part))
        for g in ("get_gain", "get_signal_level", "get_rssi"):
            assert ar.same_words(getattr(q, g)(), getattr(r, g)()), g
        assert np.array_equal(q.squelch_get_status(), r.squelch_get_status())
        assert np.array_equal(q.get_locked(), r.get_locked())


# ---- SymTrack: kSymtrackAhead = 16 ------------------------------------------------------------------------------------------
ST_K, ST_M, ST_NPFB, ST_EQ = 2, 2, 8, 2                      # the synchroniser's ring has 8 slots, the equalizer's 2


@pytest.mark.parametrize("n1,n2", pairs(16))
@pytest.mark.parametrize("C", CHANNELS)
def test_symtrack(ya, oracle, C, n1, n2):
    q = ya.SymTrack(C, st.FT, ST_K, ST_M, st.BETA, ya.ModulationScheme.Qpsk, ya.OscScheme.Nco, ST_NPFB, ST_EQ)
    r = st.SymTrackRef(C, st.FT, ST_K, ST_M, st.BETA, "Qpsk", False, ST_NPFB, ST_EQ)
    for o in (q, r):
        o.set_eq_holdoff(3)
    x = st.streams(61 + C, "Qpsk", max(n1 + n2, 1), C, ST_K, ST_M, st.BETA)
    for part in halves(x, n1, n2):
        room = q.default_ycap(len(part))
        want = r.execute(part, room)
        bad = st.same_outputs(st.run_dev(ya, q, part, room), want)
        assert not bad and not want[3].any(), (C, n1, n2, len(part), bad)
        assert not st.same_getters(q, r)
