"""tests/symsync_ref.py against itself, no GPU needed: the channel-vectorised restatement of Symsync<Complex32> equals the
scalar form built on the oracle's FirPfbFilter and dotprod bit for bit; the reference's own config and copy tests; the lock
property within the reference's bound; the quirks the library keeps (complex division by k, the derivative window that
survives reset(), a NaN that stalls its channel alone); and the chunking property under state changes at the cuts."""
import numpy as np
import pytest

import symsync_ref as sr

AMPS = [0.5, 0.5, 4.0, 0.2, 1.0]            # channel 2 is loud enough for q to clamp and del to wander


def shape():
    import yagi_amd as ya
    return ya.FirFilterShape


def taps(k, m, npfb, beta=0.3):
    return sr.rnyquist_taps(shape().Arkaiser, k, m, beta, npfb)


@pytest.mark.parametrize("locked", [False, True])
@pytest.mark.parametrize("k_out", [1, 2, 4])
@pytest.mark.parametrize("npfb", [1, 8, 32])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_vector_form_equals_scalar_form(oracle, k, npfb, k_out, locked):
    C, n, cut = 5, 150, 70
    h = taps(k, 2, npfb)
    x = sr.noise(100 * k + npfb + k_out, n, C, AMPS)
    ycap = sr.default_ycap(n, k, k_out) + 100
    r = sr.SymSyncRef(C, k, npfb, h)
    r.set_output_rate(k_out)
    r.set_lf_bw(0.02)
    a = r.execute(x[:cut], ycap)
    if locked:
        r.lock()
    b = r.execute(x[cut:], ycap)
    assert not a[2].any() and not b[2].any() and a[1].min() > 0 and b[1].min() > 0
    for c in range(C):
        q = sr.SymSyncScalar(k, npfb, h)
        q.set_output_rate(k_out)
        q.set_lf_bw(0.02)
        ya_, na, _ = q.execute(x[:cut, c], ycap)
        q.locked = locked
        yb, nb, _ = q.execute(x[cut:, c], ycap)
        assert (na, nb) == (a[1][c], b[1][c])
        assert sr.same_words(ya_[:na], a[0][:na, c]) and sr.same_words(yb[:nb], b[0][:nb, c])
        assert sr.same_words(np.float32(q.tau_decim), r.get_tau()[c])
    if not locked and k_out == 1:                                   # the loud channel did clamp
        assert abs(r.q[2]) <= 1.0


def test_symsync_config():
    """the reference's test_symsync_config (symsync.rs:338-372)"""
    S, E = sr.SymSyncRef, sr.ConfigError
    z48, z47 = np.zeros(48, np.float32), np.zeros(47, np.float32)
    for args in [(0, 12, z48), (2, 0, z48), (2, 12, z48[:0]), (2, 12, z47)]:
        with pytest.raises(E):
            S(1, *args)
    rr = shape().Rrcos
    for args in [(rr, 0, 12, 0.2, 48), (rr, 2, 0, 0.2, 48), (rr, 2, 12, 7.2, 48), (rr, 2, 12, 0.2, 0)]:
        with pytest.raises(E):
            S.rnyquist(1, *args)
    for args in [(0, 12, 0.2, 48), (2, 0, 0.2, 48), (2, 12, 7.2, 48), (2, 12, 0.2, 0)]:
        with pytest.raises(E):
            S.kaiser(1, *args)
    q = S.kaiser(1, 2, 12, 0.2, 48)
    q.lock()
    assert q.locked
    q.unlock()
    assert not q.locked
    with pytest.raises(E):
        q.set_output_rate(0)
    with pytest.raises(E):
        q.set_lf_bw(-1.0)
    with pytest.raises(E):                                           # the deviation: hdh_max = 0
        S(1, 2, 12, np.ones(49, np.float32))


def test_symsync_copy():
    """the reference's test_symsync_copy (:289-335)"""
    q0 = sr.SymSyncRef.rnyquist(1, shape().Arkaiser, 5, 7, 0.25, 64)
    q0.set_lf_bw(0.02)
    q0.execute(sr.noise(1, 640, 1, np.sqrt(2.0)), 640)
    q1 = q0.clone()
    x = sr.noise(2, 640, 1, np.sqrt(2.0))
    a, b = q0.execute(x, 640), q1.execute(x, 640)
    assert a[1][0] == b[1][0] > 100 and sr.same_outputs(a, b)
    assert sr.same_words(q0.get_tau(), q1.get_tau())


def test_lock():
    """600 QPSK symbols at four fractional offsets, one channel each: the last 100 outputs are within the reference's
    bound of the symbols delayed by 2m"""
    k, m, nsym = 2, 7, 600
    streams = [sr.qpsk_stream(nsym, tau) for tau in sr.LOCK_TAUS]
    x = np.stack([xs for _, xs in streams], axis=1)
    q = sr.SymSyncRef.rnyquist(len(streams), shape().Arkaiser, k, m, 0.35, 32)
    q.set_lf_bw(0.02)
    z, nz, st = q.execute(x, nsym + 64)
    assert not st.any()
    for c, (s, _) in enumerate(streams):
        err = sr.lock_errors(z[:, c], int(nz[c]), s)
        print(f"tau {sr.LOCK_TAUS[c]}: nz {nz[c]}, max error over the last 100 outputs {err.max():.4f}")
        assert err.max() < sr.LOCK_TOL


def test_division_by_k_is_the_complex_one():
    k, npfb = 3, 8
    q = sr.SymSyncRef(1, k, npfb, taps(k, 3, npfb))
    x = sr.noise(7, 300, 1)
    y, ny, _ = q.execute(x, 400)
    # the same matched sums through the plain quotient mf.re / 3, mf.im / 3
    r = sr.SymSyncScalar(k, npfb, taps(k, 3, npfb))
    out = []
    orig = r.mf.execute
    r.mf.execute = lambda b: out.append(orig(b)) or out[-1]
    r.execute(x[:, 0], 400)
    mf = np.array(out[:int(ny[0])], np.complex64)
    plain = (mf.real / np.float32(3)) + 1j * (mf.imag / np.float32(3))
    differ = np.sum(sr.words(plain.astype(np.complex64)) != sr.words(y[:int(ny[0]), 0]))
    assert differ >= 1
    assert np.allclose(plain, y[:int(ny[0]), 0], rtol=1e-6)


def test_reset_keeps_the_derivative_window():
    k, m, npfb = 2, 7, 32
    h = taps(k, m, npfb, 0.35)
    x0, x1 = sr.noise(3, 100, 1, 2.0), sr.noise(4, 100, 1)
    used, fresh = sr.SymSyncRef(1, k, npfb, h), sr.SymSyncRef(1, k, npfb, h)
    for q in (used, fresh):
        q.set_lf_bw(0.2)                                            # wide enough for the timing error to move the branch at once
    used.execute(x0, 200)
    used.reset()
    a, b = used.execute(x1, 200), fresh.execute(x1, 200)
    ls = used.ls
    assert not sr.same_words(a[0][:ls, 0], b[0][:ls, 0])
    assert sr.same_words(a[0][0, 0], b[0][0, 0])                      # the matched window was cleared: the first word agrees
    scalar = sr.SymSyncScalar(k, npfb, h)                           # and the scalar form does the same
    scalar.set_lf_bw(0.2)
    scalar.execute(x0[:, 0], 200)
    scalar.reset()
    ys, ns, _ = scalar.execute(x1[:, 0], 200)
    assert ns == a[1][0] and sr.same_words(ys[:ns], a[0][:ns, 0])


def test_nan_stalls_its_channel_alone():
    k, npfb, C, ycap = 2, 8, 3, 40
    h = taps(k, 3, npfb)
    x = sr.noise(5, 60, C)
    clean = sr.SymSyncRef(C, k, npfb, h).execute(x, ycap)
    bad = x.copy()
    bad[20, 1] = np.nan
    q = sr.SymSyncRef(C, k, npfb, h)
    y, ny, st = q.execute(bad, ycap)
    assert list(st) == [0, 1, 0] and ny[1] == ycap
    assert np.array_equal(ny[[0, 2]], clean[1][[0, 2]])
    for c in (0, 2):
        assert sr.same_words(y[:ny[c], c], clean[0][:ny[c], c])
    before = int(clean[1][1] * 20 / 60) - 4                          # outputs well before the NaN are the clean ones
    assert sr.same_words(y[:before, 1], clean[0][:before, 1])
    tau = q.get_tau()
    y2, ny2, st2 = q.execute(x, ycap)                                # stalled: no output, tau kept
    assert ny2[1] == 0 and st2[1] == 1 and ny2[0] > 0 and sr.same_words(q.get_tau()[1], tau[1])
    # reset_channel revives it, but the NaN is still in the derivative window, which no reset clears (the reference's
    # quirk): the channel writes outputs again and stalls at its first loop update, until Ls samples have pushed the NaN out
    rounds = 0
    while True:
        q.reset_channel(1)
        y3, ny3, st3 = q.execute(x, ycap)
        assert ny3[1] > 0
        rounds += 1
        if not st3[1]:
            break
        assert ny3[1] == ycap and rounds <= q.ls
    assert rounds > 1 and np.isfinite(y3[:ny3[1], 1]).all()


def test_small_ycap_keeps_the_first_words():
    k, npfb = 2, 8
    h = taps(k, 3, npfb)
    x = sr.noise(6, 60, 2)
    full = sr.SymSyncRef(2, k, npfb, h).execute(x, 100)
    y, ny, st = sr.SymSyncRef(2, k, npfb, h).execute(x, 10)
    assert list(ny) == [10, 10] and list(st) == [1, 1] and sr.same_words(y, full[0][:10])
    y, ny, st = sr.SymSyncRef(2, k, npfb, h).execute(x, int(full[1].max()))     # exactly enough: no stall
    assert not st.any() and sr.same_outputs((y, ny, st), full)


@pytest.mark.parametrize("change", ["none", "bw", "lock", "rate"])
def test_cuts(change):
    k, m, npfb, C, n = 2, 3, 8, 3, 400
    h = taps(k, m, npfb)
    ls = sr.SymSyncRef(1, k, npfb, h).ls
    x = sr.noise(8, n, C, [0.5, 2.0, 0.5])
    at = 200

    def run(lens):
        q, outs, pos = sr.SymSyncRef(C, k, npfb, h), [[] for _ in range(C)], 0
        for ln in lens:
            if pos == at:
                {"none": lambda: None, "bw": lambda: q.set_lf_bw(0.05), "lock": q.lock,
                 "rate": lambda: q.set_output_rate(2)}[change]()
            y, ny, st = q.execute(x[pos:pos + ln], 2 * ln + 8)
            assert not st.any()
            for c in range(C):
                outs[c].append(y[:ny[c], c])
            pos += ln
        assert pos == n
        return [np.concatenate(o) for o in outs], q.get_tau()

    one, tau = run([at, n - at])
    for piece in (1, 2, ls - 1, ls, 97):
        lens = [piece] * (at // piece) + ([at % piece] if at % piece else [])
        lens += [piece] * ((n - at) // piece) + ([(n - at) % piece] if (n - at) % piece else [])
        got, t = run(lens)
        assert all(sr.same_words(a, b) for a, b in zip(got, one)) and sr.same_words(t, tau), piece
