"""SymTrack on the GPU against tests/symtrack_ref.py, the per-channel restatement over the parts' scalar restatements:
every word of y and sym below ny, ny, the stall reason and every getter after every call, bit for bit (a NaN matching a
NaN).  The restatement is a scalar Python loop, so the blocks are a few hundred rows; the shapes are the smallest that
cross each seam: a lane short of a wave, a wave, a lane more, several workgroups; the branch taps' three bank shapes and
the long one; one, two and nine equalizer taps; both oscillator tables; the three equalizer strategies; every kind of
decision; the hold-off gate inside a call and at a call boundary; calls of 0, 1, 3 and odd row counts.
The last test runs SymTrack open loop against the library's own Agc, SymSync, Osc, EqLms and Modem objects, which does
not go through the restatement at all."""
import numpy as np
import pytest

import symtrack_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


FT, BETA, SCHEMES, SHAPES, KINDS = sr.FT, sr.BETA, sr.SCHEMES, sr.SHAPES, sr.KINDS


def make(ya, C, k, m, npfb, scheme, vco=False, eq_len=9, strategy=sr.CM, holdoff=200):
    s = SCHEMES[scheme]
    q = ya.SymTrack(C, FT, k, m, BETA, s if not isinstance(s, str) else ya.ModulationScheme[s],
                    ya.OscScheme.Vco if vco else ya.OscScheme.Nco, npfb, eq_len)
    r = sr.SymTrackRef(C, FT, k, m, BETA, s, vco, npfb, eq_len)
    for o in (q, r):
        o.set_eq_strategy(strategy)
        o.set_eq_holdoff(holdoff)
    return q, r


def check_call(ya, q, r, x, ycap, dev_pad=None, what=""):
    """one call on both; dev_pad = None takes host pointers, else device pointers at pitch C + dev_pad"""
    want = r.execute(x, ycap)
    got = q.execute(x, ycap) if dev_pad is None else sr.run_dev(ya, q, x, ycap, dev_pad)
    assert not sr.same_outputs(got, want), (what, sr.same_outputs(got, want))
    assert not sr.same_getters(q, r), (what, sr.same_getters(q, r))
    return got


@pytest.mark.parametrize("C,k,m,npfb,eq_len,vco,n", SHAPES)
def test_words_and_getters_call_by_call(ya, oracle, C, k, m, npfb, eq_len, vco, n):
    """the stream cut into calls of 0, 1, 3 and odd row counts, host and device pointers (pitch C + 3) in turn; a second
    object that takes the whole stream in one call gives the same words: the result does not depend on the cuts"""
    q, r = make(ya, C, k, m, npfb, "Qpsk", vco, eq_len, sr.CM, 3)
    whole = q.clone()
    f = (0.04 * (np.arange(C) % 7 - 3) / 3.0).astype(np.float32)
    ph = (0.3 * (np.arange(C) % 5)).astype(np.float32)
    for o in (q, r, whole):
        o.set_nco_all(f, ph)
    assert not sr.same_getters(q, r)
    x = sr.streams(C + n, "Qpsk", n, C, k, m, BETA)
    ys, ss = [[] for _ in range(C)], [[] for _ in range(C)]
    for i, (a, b) in enumerate(sr.cuts(n)):
        y, sym, ny, st = check_call(ya, q, r, x[a:b], q.default_ycap(b - a), None if i % 2 else 3, (a, b))
        assert not st.any()
        for c in range(C):
            ys[c].append(y[:ny[c], c])
            ss[c].append(sym[:ny[c], c])
    y, sym, ny, st = whole.execute(x, q.default_ycap(n))
    for c in range(C):
        assert sr.same_words(np.concatenate(ys[c]), y[:ny[c], c].copy()), c
        assert np.array_equal(np.concatenate(ss[c]), sym[:ny[c], c]), c
    assert not sr.same_getters(whole, r)


@pytest.mark.parametrize("scheme,vco,strategy,eq_len", KINDS)
def test_every_kind_of_decision(ya, oracle, scheme, vco, strategy, eq_len):
    C, k, m, npfb, n = 4, 2, 2, 8, 240
    q, r = make(ya, C, k, m, npfb, scheme, vco, eq_len, strategy, 3)
    x = sr.streams(11, SCHEMES[scheme], n, C, k, m, BETA)
    for a, b in ((0, 101), (101, n)):
        y, sym, ny, st = check_call(ya, q, r, x[a:b], q.default_ycap(b - a), None, (scheme, a))
    assert ny.min() > 40 and int(q.get_num_syms().min()) > 100       # well past the hold-off: the weights have moved
    if strategy != sr.OFF:
        fresh = ya.SymTrack(1, FT, k, m, BETA, ya.ModulationScheme.Qpsk, ya.OscScheme.Nco, npfb, eq_len)
        assert not np.array_equal(q.get_weights()[0], fresh.get_weights()[0])


@pytest.mark.parametrize("holdoff", [0, 3, 200])
def test_the_holdoff_gate_inside_a_call_and_at_a_call_boundary(ya, oracle, holdoff):
    """the first update runs on the symbol with num_syms = holdoff + 1.  One pair of objects crosses the gate inside a
    call; another is cut exactly where channel 0 has counted holdoff + 1 symbols, so the first update is the first
    symbol of the next call"""
    C, k, m, npfb = 2, 2, 2, 8
    n = 2 * (holdoff + 12)
    x = sr.streams(5, "Qpsk", n, C, k, m, BETA)
    q, r = make(ya, C, k, m, npfb, "Qpsk", False, 9, sr.CM, holdoff)
    w0 = q.get_weights().copy()
    check_call(ya, q, r, x, q.default_ycap(n), 3, "inside")
    assert int(q.get_num_syms().min()) > holdoff + 2 and not np.array_equal(q.get_weights(), w0)
    q, r = make(ya, C, k, m, npfb, "Qpsk", False, 9, sr.CM, holdoff)
    probe, rows = r.clone(), 0
    while int(probe.get_num_syms()[0]) < holdoff + 1:                # one row at a time: where the boundary falls
        probe.execute(x[rows:rows + 1], 4)
        rows += 1
    assert int(probe.get_num_syms()[0]) == holdoff + 1 and rows < n - 8
    check_call(ya, q, r, x[:rows], q.default_ycap(rows), None, "up to the gate")
    assert sr.same_words(q.get_weights()[0], w0[0])                  # channel 0 has not updated yet
    check_call(ya, q, r, x[rows:rows + 1], 4, None, "one row")
    check_call(ya, q, r, x[rows + 1:], q.default_ycap(n - rows - 1), 3, "behind the gate")
    assert not np.array_equal(q.get_weights()[0], w0[0])


def test_setters_clone_and_reset_between_calls(ya, oracle):
    C, k, m, npfb, n = 5, 2, 2, 8, 60
    q, r = make(ya, C, k, m, npfb, "Qam16", True, 9, sr.CM, 3)
    x = sr.streams(21, "Qam16", 5 * n, C, k, m, BETA)
    check_call(ya, q, r, x[:n], q.default_ycap(n), None, "first")
    q2, r2 = q.clone(), r.clone()
    assert not sr.same_getters(q2, r2)
    for o in (q, r):
        o.reset_channel(2)
        o.set_bandwidth(0.4)
    assert q.get_bandwidth() == np.float32(0.4)
    check_call(ya, q, r, x[n:2 * n], q.default_ycap(n), 3, "after reset_channel and set_bandwidth")
    for o in (q, r):
        o.set_eq_strategy(sr.DD)
        o.set_nco(1, 0.25, 1.0)
    check_call(ya, q, r, x[2 * n:3 * n], q.default_ycap(n), None, "after set_eq_strategy and set_nco")
    for o in (q, r):
        o.set_bandwidths(0.05, 0.002, 0.0, 0.01)
        o.set_eq_strategy(sr.OFF)
    check_call(ya, q, r, x[3 * n:4 * n], q.default_ycap(n), 3, "after set_bandwidths")
    for o in (q, r):
        o.reset()
    check_call(ya, q, r, x[4 * n:], q.default_ycap(n), None, "after reset")
    check_call(ya, q2, r2, x[n:2 * n], q.default_ycap(n), 3, "the clone goes on from the first call")


def test_zero_and_non_finite_channels_change_only_their_own_column(ya, oracle):
    C, k, m, npfb, n = 5, 2, 2, 8, 120
    x = sr.streams(31, "Qpsk", n, C, k, m, BETA)
    odd = x.copy()
    odd[:, 1] = 0
    odd[40, 3] = np.nan
    odd[77, 3] = np.complex64(complex(np.inf, 1.0))
    q, r = make(ya, C, k, m, npfb, "Qpsk", False, 9, sr.CM, 3)
    plain, _ = make(ya, C, k, m, npfb, "Qpsk", False, 9, sr.CM, 3)
    ycap = q.default_ycap(n) + 40
    got = check_call(ya, q, r, odd, ycap, 3, "odd")
    ref = plain.execute(x, ycap)
    for c in (0, 2, 4):
        assert got[2][c] == ref[2][c] and sr.same_words(got[0][:got[2][c], c].copy(), ref[0][:ref[2][c], c].copy()), c
        assert np.array_equal(got[1][:got[2][c], c], ref[1][:ref[2][c], c])
    more = sr.streams(32, "Qpsk", 50, C, k, m, BETA)
    check_call(ya, q, r, more, q.default_ycap(50) + 40, None, "a second call")


def test_a_small_ycap_stalls_channels_mid_call(ya, oracle):
    C, k, m, npfb, n = 66, 2, 2, 8, 50
    q, r = make(ya, C, k, m, npfb, "Qpsk", False, 2, sr.CM, 3)
    x = sr.streams(41, "Qpsk", 2 * n, C, k, m, BETA)
    x[:, ::3] = 0                                                    # every third channel silent: its loop emits as the others
    y, sym, ny, st = check_call(ya, q, r, x[:n], 20, 3, "stalling")
    assert (st == sr.STALL_CAPACITY).all() and (ny == 20).all()
    for o in (q, r):
        o.reset_channel(7)
    y, sym, ny, st = check_call(ya, q, r, x[n:], 40, None, "stalled channels ignore their input")
    assert ny[7] > 0 and st[7] == 0 and ny[np.arange(C) != 7].max() == 0 and (st[np.arange(C) != 7] == sr.STALL_CAPACITY).all()


def test_a_huge_sample_with_the_gain_frozen_stalls_on_the_pll_rule(ya, oracle):
    """agc bandwidth 0 freezes the gain at 1, so the 1e30 sample reaches the demodulator and e beta passes 256.  (The
    four bandwidths are set one by one: set_bandwidth(0) would zero the PLL's gains too, and e 0 never reaches 256.)"""
    C, k, m, npfb, n, victim = 4, 2, 2, 8, 80, 2
    q, r = make(ya, C, k, m, npfb, "Qpsk", False, 9, sr.CM, 3)
    for o in (q, r):
        o.set_bandwidths(0.0, 0.0009, 0.018, 0.0009)
    x = sr.pll_stimulus(C, k, m, n, victim, 41)
    y, sym, ny, st = check_call(ya, q, r, x, q.default_ycap(n), 3, "pll")
    assert st.tolist() == [0, 0, sr.STALL_PLL, 0] and 18 <= ny[victim] <= 24
    check_call(ya, q, r, x[:30], q.default_ycap(30), None, "afterwards")
    for o in (q, r):
        o.reset_channel(victim)
    y, sym, ny, st = check_call(ya, q, r, x[:30], q.default_ycap(30), 3, "revived")
    assert not st.any() and ny[victim] > 0


def test_open_loop_against_the_librarys_own_objects(ya):
    """only the agc and the timing loop run (strategy OFF, PLL bandwidth 0, a fixed oscillator frequency per channel): every
    word equals Agc.execute_block -> SymSync.execute (k_out = 2) -> Osc.mix_block_down per channel -> EqLms.decim_block(2,
    NONE) -> Modem.demodulate_block, column by column over each channel's outputs, an odd last one dropped"""
    C, k, m, npfb, eq_len, n = 65, 2, 3, 16, 9, 400
    bw_agc, bw_sync = 0.018, 0.0009
    x = sr.streams(61, "Qam16", n, C, k, m, BETA)
    f = (0.05 * (np.arange(C) % 9 - 4) / 4.0).astype(np.float32)
    for vco in (False, True):
        q = ya.SymTrack(C, FT, k, m, BETA, ya.ModulationScheme.Qam16, ya.OscScheme.Vco if vco else ya.OscScheme.Nco, npfb, eq_len)
        q.set_bandwidths(bw_agc, bw_sync, 0.0, 0.0)
        q.set_eq_strategy(ya.SymTrackEq.OFF)
        q.set_nco_all(f)
        y, sym, ny, st = q.execute(x, n)
        assert not st.any()

        agc = ya.Agc(C)
        agc.set_bandwidth(bw_agc)
        v = agc.execute_block(x)
        ss = ya.SymSync.rnyquist(C, FT, k, m, BETA, npfb)
        ss.set_output_rate(2)
        ss.set_lf_bw(bw_sync)
        s, ns, stalled = ss.execute(v, 2 * n)
        assert not stalled.any() and np.array_equal(ny, (ns + 1) // 2)
        rows = int(ns.max()) // 2 * 2
        u = np.zeros((rows, C), np.complex64)
        for c in range(C):
            osc = ya.Osc(ya.OscScheme.Vco if vco else ya.OscScheme.Nco)
            osc.set_frequency(float(f[c]))
            col = np.ascontiguousarray(s[:ns[c], c])
            xd, yd = ya.DeviceArray.from_numpy(col), ya.DeviceArray(col.size, np.complex64)
            osc.mix_block_down_dev(xd, col.size, yd)
            ya.synchronize()
            u[:min(rows, ns[c]), c] = yd.to_numpy()[:min(rows, ns[c])]
            xd.free()
            yd.free()
        eq = ya.EqLms.lowpass(C, eq_len, 0.45)
        d = eq.decim_block(2, ya.EqLmsUpdate.NONE, u)
        modem = ya.Modem(ya.ModulationScheme.Qam16)
        for c in range(C):
            full = int(ns[c]) // 2
            assert full > 150
            assert sr.same_words(y[:full, c].copy(), d[:full, c].copy()), (vco, c)
            assert np.array_equal(sym[:full, c], modem.demodulate_block(d[:full, c].copy())), (vco, c)
        assert sr.same_words(q.get_tau(), ss.get_tau()) and sr.same_words(q.get_gain(), agc.get_gain())
