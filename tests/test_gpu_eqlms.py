"""EqLms on the GPU against tests/eqlms_ref.py, bit for bit (a NaN matching a NaN): every word of y, get_coefficients
after every call, and so the state carried into the next call.  Channel counts 1, 63, 64, 65 and 200 (a lone lane, a
partial wave, the wave seam, several workgroups); h_len 1 and 2 (the ring wraps on every step), 29, and 65 and 128 (above
64 KiB of LDS: the launch sets the attribute); k in {1, 2, 5}, k > h_len included; decim_block in its four modes and
execute_block, through host pointers and through device pointers with pitches wider than C; streams cut into calls of 0,
1, h_len - 1 rows and the rest (0, 1, 2 symbols and the rest for decim_block), with the buf_full gate crossed inside a
call and exactly at a call boundary; clone, reset_channel, set_bw and a change of mode between calls; an all-zero channel
and a channel with a NaN and an Inf sample that change only their own column."""
import numpy as np
import pytest

import eqlms_ref as er
from test_eqlms_ref_cpu import MODES, run, taps

pytestmark = pytest.mark.gpu

#         C  h_len  k
SHAPES = [(1, 29, 2), (63, 1, 1), (63, 2, 5), (64, 29, 1), (65, 29, 5), (65, 65, 2), (200, 128, 2), (200, 2, 2),
          (65, 1, 5), (64, 128, 5), (200, 65, 1)]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def pair(ya, C, h_len, h, mu=0.2, table=er.QAM16_MAP):
    q, r = ya.EqLms(C, h_len, h), er.EqLmsRef(C, h_len, h)
    q.set_bw(mu), r.set_bw(mu)
    q.set_constellation(table), r.set_constellation(table)
    return q, r


def call(ya, q, k, mode, x, d, dev):
    """one block call on the object: host pointers, or device pointers with pitches C + 3; y[rows][C]"""
    C = x.shape[1]
    if dev:
        return er.run_dev(ya, q, k, x, mode, d, pad=3)[:, :C]
    return q.execute_block(k, x) if mode is None else q.decim_block(k, ya.EqLmsUpdate(mode), x, d)


def cuts(total, first):
    out, at = [], 0
    for c in first:
        c = min(c, total - at)
        out.append((at, at + c))
        at += c
    out.append((at, total))
    return out


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("C,h_len,k", SHAPES)
def test_every_call_equals_the_ref(ya, C, h_len, k, dev):
    nsym = 12 + -(-h_len // k)
    n = nsym * k
    x = er.streams(n, C, 300 + C + h_len + k, k=k)
    d = er.symbols(nsym, C, 5)
    h = taps(h_len)
    for mode in MODES:
        q, r = pair(ya, C, h_len, h)
        # rows for execute_block: 0, 1, h_len - 1 (the gate opens on that call's last row), the rest; symbols for decim_block
        parts = cuts(n, (0, 1, h_len - 1)) if mode is None else cuts(nsym, (0, 1, 2))
        for lo, hi in parts:
            rows = slice(lo, hi) if mode is None else slice(lo * k, hi * k)
            dd = d[lo:hi] if mode == er.TRAIN else None
            want = run(r, k, mode, x[rows], dd)
            got = call(ya, q, k, mode, x[rows], dd, dev)
            assert er.same_words(got, want), (mode, lo, hi)
            assert er.same_words(q.get_coefficients(), r.get_coefficients()), (mode, lo, hi)
        w = r.get_coefficients()
        if mode != er.NONE and C > 3:
            assert not np.isfinite(w[1]).all() and not np.isfinite(w[3]).all()     # 0 / 0, and the NaN sample
        assert er.same_words(q.get_weights(), r.get_weights())


@pytest.mark.parametrize("mode", MODES)
def test_the_gate_inside_a_call_and_at_a_call_boundary(ya, mode):
    C, h_len, k, nsym = 65, 6, 2, 14
    x, d = er.streams(nsym * k, C, 77, k=k), er.symbols(nsym, C, 6)
    whole = None
    # in rows: (6,) ends a call on the row that makes count = h_len; (4,) and (2, 4) open the gate inside a later call;
    # (8,) starts a call with the gate open; single rows serve execute_block alone
    for first in ((6,), (4,), (2, 4), (8,), (1, 1, 1, 1, 1, 1, 1, 1)):
        if mode is not None and any(c % k for c in first):
            continue
        q, r = pair(ya, C, h_len, None, mu=0.3, table=er.QPSK_MAP)
        got = []
        for lo, hi in cuts(nsym * k, first):
            dd = d[lo // k:hi // k] if mode == er.TRAIN else None
            got.append(call(ya, q, k, mode, x[lo:hi], dd, dev=True))
            run(r, k, mode, x[lo:hi], dd)
            assert er.same_words(q.get_coefficients(), r.get_coefficients()), (first, lo)
        got = np.concatenate(got)
        whole = got if whole is None else whole
        assert er.same_words(got, whole), first                # the result does not depend on the cuts
    r = er.EqLmsRef(C, h_len)
    r.set_bw(0.3), r.set_constellation(er.QPSK_MAP)
    assert er.same_words(whole, run(r, k, mode, x, d if mode == er.TRAIN else None))


def test_odd_cuts_of_execute_block(ya):
    """execute_block's update test runs on count, which carries across calls of any length"""
    C, h_len, k = 64, 5, 2
    x = er.streams(41, C, 13, k=k)
    q, r = pair(ya, C, h_len, None)
    for lo, hi in cuts(41, (1, 3, 4, 7)):
        assert er.same_words(call(ya, q, k, None, x[lo:hi], None, dev=lo % 2 == 0), r.execute_block(k, x[lo:hi])), lo
    assert er.same_words(q.get_coefficients(), r.get_coefficients())


def test_clone_reset_channel_set_bw_and_a_change_of_mode(ya):
    C, h_len, k = 65, 29, 2
    x, d = er.streams(200, C, 21, k=k), er.symbols(100, C, 8)
    q, r = pair(ya, C, h_len, taps(h_len), table=er.QPSK_MAP)

    def both(objs, mode, rows, dev):
        lo, hi = rows
        dd = d[lo // k:hi // k] if mode == er.TRAIN else None
        want = run(objs[1], k, mode, x[lo:hi], dd)
        assert er.same_words(call(ya, objs[0], k, mode, x[lo:hi], dd, dev), want), (mode, rows)
        assert er.same_words(objs[0].get_coefficients(), objs[1].get_coefficients()), (mode, rows)

    both((q, r), None, (0, 37), True)                          # an odd number of steps: count = 37
    q2, r2 = q.clone(), r.clone()
    for o in ((q, r), (q2, r2)):
        both(o, None, (37, 60), False)
    q2.set_bw(0.05), r2.set_bw(0.05)                            # the clone goes its own way
    both((q2, r2), er.TRAIN, (60, 100), True)
    both((q, r), er.BLIND, (60, 100), True)
    assert not er.same_words(q.get_coefficients(), q2.get_coefficients())
    for c in (0, 64):
        q.reset_channel(c), r.reset_channel(c)                  # count differs between the lanes of a wave from here on
    assert er.same_words(q.get_coefficients(), r.get_coefficients())
    both((q, r), er.DECISION, (100, 130), False)
    both((q, r), None, (130, 151), True)                        # per-lane update test and gate
    both((q, r), er.NONE, (151, 161), True)
    both((q, r), er.TRAIN, (161, 199), False)
    assert q.get_bw() == np.float32(0.2) and q2.get_bw() == np.float32(0.05) and q.get_length() == h_len
    q.reset(), r.reset()
    assert er.same_words(q.get_coefficients(), r.get_coefficients())
    both((q, r), er.BLIND, (0, 80), True)
    with pytest.raises(ya.ConfigError):
        q.set_bw(-1.0)
    with pytest.raises(ya.ConfigError):
        q.reset_channel(C)


@pytest.mark.parametrize("mode", MODES)
def test_non_finite_channels_change_only_their_own_column(ya, mode):
    C, h_len, k, nsym = 65, 29, 2, 40
    x, d = er.streams(nsym * k, C, 31, k=k), er.symbols(nsym, C, 9)
    clean = x.copy()
    clean[:, [1, 3]] = er.noise(4, nsym * k, 2)
    dd = d if mode == er.TRAIN else None
    qa, r = pair(ya, C, h_len, None, table=er.QPSK_MAP)
    qb, _ = pair(ya, C, h_len, None, table=er.QPSK_MAP)
    ya_, yb = call(ya, qa, k, mode, x, dd, True), call(ya, qb, k, mode, clean, dd, True)
    assert er.same_words(ya_, run(r, k, mode, x, dd))
    others = np.setdiff1d(np.arange(C), [1, 3])
    assert er.same_words(ya_[:, others], yb[:, others])
    wa, wb = qa.get_coefficients(), qb.get_coefficients()
    assert er.same_words(wa, r.get_coefficients()) and er.same_words(wa[others], wb[others])
    assert np.isnan(ya_[:, 3]).any()


def test_designs_are_the_restatements(ya):
    sh = ya.FirFilterShape
    for ft, k, m, beta, dt in [(sh.Arkaiser, 2, 7, 0.3, 0.0), (sh.Rrcos, 4, 3, 0.25, 0.5), (sh.Kaiser, 2, 3, 0.3, -0.25)]:
        q = ya.EqLms.rnyquist(3, ft, k, m, beta, dt)
        r = er.EqLmsRef(3, 2 * k * m + 1, er.rnyquist_h(ft, k, m, beta, dt))
        assert q.get_length() == 2 * k * m + 1 and q.get_bw() == 0.5
        assert er.same_words(q.get_coefficients(), r.get_coefficients())
        assert er.same_words(q.get_weights(), r.get_weights())
    for h_len, fc in [(21, 0.12345), (29, 0.25), (2, 0.5)]:
        q, r = ya.EqLms.lowpass(2, h_len, fc), er.EqLmsRef(2, h_len, er.lowpass_h(h_len, fc))
        assert er.same_words(q.get_coefficients(), r.get_coefficients())
    q = ya.EqLms(2, 13)
    want = np.zeros((2, 13), np.complex64)
    want[:, 6] = 1
    assert er.same_words(q.get_coefficients(), want) and er.same_words(q.get_weights(), np.conj(want))


def test_bad_block_arguments_are_config_errors(ya):
    C = 5
    q = ya.EqLms(C, 7)
    xd, yd = ya.DeviceArray(64, np.complex64), ya.DeviceArray(64, np.complex64)
    U = ya.EqLmsUpdate
    for args in [(1, xd.ptr, C - 1, 4, yd.ptr, C), (1, xd.ptr, C, 4, yd.ptr, C - 1), (0, xd.ptr, C, 4, yd.ptr, C),
                 (1, xd.ptr, C, 2 ** 31, yd.ptr, C), (1, None, C, 4, yd.ptr, C), (1, xd.ptr, C, 4, None, C)]:
        with pytest.raises(ya.ConfigError):
            q.execute_block_devptr(*args)
    for args in [(3, U.NONE, xd.ptr, C, 4, None, C, yd.ptr, C), (0, U.NONE, xd.ptr, C, 4, None, C, yd.ptr, C),
                 (2, U.TRAIN, xd.ptr, C, 4, None, C, yd.ptr, C), (2, U.TRAIN, xd.ptr, C, 4, xd.ptr, C - 1, yd.ptr, C),
                 (2, U.DECISION, xd.ptr, C, 4, None, C, yd.ptr, C), (2, 4, xd.ptr, C, 4, None, C, yd.ptr, C),
                 (2, 7, xd.ptr, C, 4, None, C, yd.ptr, C)]:
        with pytest.raises(ya.ConfigError):
            q.decim_block_devptr(*args)
    for table in (np.zeros(0, np.complex64), np.zeros(ya.EQLMS_TABLE_MAX + 1, np.complex64)):
        with pytest.raises(ya.ConfigError):
            q.set_constellation(table)
    with pytest.raises(ya.ConfigError):
        q.decim_block(2, U.TRAIN, np.zeros((4, C), np.complex64))
    with pytest.raises(ya.ConfigError):
        q.decim_block(3, U.NONE, np.zeros((4, C), np.complex64))
    want = np.zeros((C, 7), np.complex64)
    want[:, 3] = 1
    assert er.same_words(q.get_coefficients(), want)            # nothing ran
