"""yagi_amd.EqRls on the GPU against tests/eqrls_ref.py, bit for bit (a NaN matching a NaN): y of every call, and
get_coefficients, get_weights and get_matrix after every call.  Every admissible number of lanes per channel is run through
set_lanes, the planner's own choice among them; the channel counts sit at the seams of a wave of 64 / L channels and of the
grid, the orders p at the degenerate values, at one column per lane and one more, and at the limit (LDS above 64 KiB).
Streams are cut into calls of 0, 1 and 2 symbols and the rest, the mode and lambda change between calls, and host pointers
alternate with device pointers of pitch C + 3."""
import numpy as np
import pytest

import eqlms_ref as er
import eqrls_ref as rr

pytestmark = pytest.mark.gpu

ORDERS = [1, 2, 3, 8, 9, 32]
CUTS = [0, 1, 2]                                            # symbols per call; the rest of the stream follows
MODES = [rr.TRAIN, rr.DECISION, rr.NONE, rr.TRAIN]
KS = [1, 2, 5]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def admissible(p):
    import yagi_amd
    return yagi_amd.eqrls_plan(1, p)[2]


def taps(p):
    return er.noise(p, 1, p, 0.7)[0] if p % 2 else None


_WANT = {}


def want(C, p, k):
    """the reference's answers for the stream of (C, p, k), call by call: computed once, shared by every L"""
    key = (C, p, k)
    if key not in _WANT:
        nsym = 12 + p
        x, d = rr.streams(nsym * k, C, 7 * p + k, k), er.symbols(nsym, C, p + C)
        r = rr.EqRlsRef(C, p, taps(p))
        r.set_constellation(er.QAM16_MAP)
        calls, s0 = [], 0
        for i, cut in enumerate(CUTS + [nsym - sum(CUTS)]):
            if i == 2:
                r.set_bw(0.97)
            xs, ds = x[s0 * k:(s0 + cut) * k], d[s0:s0 + cut]
            y = r.step_block(k, MODES[i], xs, ds if MODES[i] == rr.TRAIN else None)
            calls.append((xs, ds, y, r.get_coefficients(), r.get_weights(), r.get_matrix()))
            s0 += cut
        _WANT[key] = calls
    return _WANT[key]


def run_dev(ya, q, k, mode, x, d, pad):
    """step_block_devptr on plain device buffers whose pitches are C + pad"""
    n, C = x.shape
    pitch, rows = C + pad, n // k

    def up(a, r):
        wide = np.full((max(r, 1), pitch), 5 - 3j, np.complex64)
        wide[:r, :C] = a
        return ya.DeviceArray.from_numpy(wide)
    xd, dd = up(x, n), up(d, rows) if mode == rr.TRAIN else None
    yd = ya.DeviceArray(max(rows, 1) * pitch, np.complex64)
    yd.zero()
    q.step_block_devptr(k, int(mode), xd.ptr, pitch, n, None if dd is None else dd.ptr, pitch, yd.ptr, pitch)
    ya.synchronize()
    y = yd.to_numpy()[:rows * pitch].reshape(rows, pitch).copy()
    for b in (xd, dd, yd):
        if b is not None:
            b.free()
    assert not y[:, C:].any(), "a pitch-gap column was written"
    return y[:, :C]


def stream_case(ya, C, p, k, L):
    q = ya.EqRls(C, p, taps(p))
    q.set_lanes(L)
    assert q.get_lanes() == L
    q.set_constellation(er.QAM16_MAP)
    for i, (xs, ds, y, w0, w1, P) in enumerate(want(C, p, k)):
        if i == 2:
            q.set_bw(0.97)
        mode = MODES[i]
        if (i + C) % 2:
            got = q.step_block(k, mode, xs, ds if mode == rr.TRAIN else None)
        else:
            got = run_dev(ya, q, k, mode, xs, ds, 3)
        where = (C, p, k, L, i)
        assert rr.same_words(got, y), where
        assert rr.same_words(q.get_coefficients(), w0), where
        assert rr.same_words(q.get_weights(), w1), where
        assert rr.same_words(q.get_matrix(), P), where


@pytest.mark.parametrize("p,L", [(p, L) for p in ORDERS for L in admissible(p)])
def test_streams_at_every_lane_count(ya, p, L):
    """C = 1, the seams of a wave of 64 / L channels, and 130 (several workgroups at every L)"""
    plan_L, lds, adm = ya.eqrls_plan(1, p)
    assert L in adm and plan_L in adm
    for j, C in enumerate(sorted(set([1, 130] + rr.lanes_around(L)))):
        stream_case(ya, C, p, KS[(j + p) % 3], L)


@pytest.mark.parametrize("p", ORDERS)
def test_the_planners_choice(ya, p):
    for C, k in ((1, 1), (5, 2), (130, 5 if p < 32 else 1)):
        L = ya.eqrls_plan(C, p)[0]
        q = ya.EqRls(C, p)
        assert q.get_lanes() == L
        stream_case(ya, C, p, k, L)
    q.set_lanes(0)
    assert q.get_lanes() == L
    for bad in (3, 128, max(admissible(p)) * 2):
        with pytest.raises(ya.ConfigError):
            q.set_lanes(bad)


@pytest.mark.parametrize("p", [3, 9, 32])
def test_train(ya, p):
    C, n = 5, p + 9
    x, d = er.noise(p, n, C), er.symbols(n, C, p)
    w = er.noise(p + 1, C, p, 0.3)
    for L in admissible(p):
        q, r = ya.EqRls(C, p), rr.EqRlsRef(C, p)
        q.set_lanes(L)
        q.step_block(1, rr.TRAIN, x[:4], d[:4]), r.step_block(1, rr.TRAIN, x[:4], d[:4])     # train resets this
        assert rr.same_words(q.train(w, x, d), r.train(w, x, d)), (p, L)
        assert rr.state_same(q, r)
        with pytest.raises(ya.ConfigError):
            q.train(w, x[:p - 1], d[:p - 1])
        xd, dd = ya.DeviceArray.from_numpy(x), ya.DeviceArray.from_numpy(d)
        q.train_devptr(w[:, ::-1], xd.ptr, C, n, dd.ptr, C)
        assert rr.same_words(q.get_weights(), r.train(w[:, ::-1], x, d)) and rr.state_same(q, r)
        xd.free(), dd.free()


def test_clone_reset_channel_and_recreate(ya):
    C, p, k = 9, 6, 2
    nsym = 10
    x, d = rr.streams(3 * nsym * k, C, 21, k), er.symbols(3 * nsym, C, 22)
    q, r = ya.EqRls(C, p), rr.EqRlsRef(C, p)
    seg = lambda i: (x[i * nsym * k:(i + 1) * nsym * k], d[i * nsym:(i + 1) * nsym])
    assert rr.same_words(q.step_block(k, rr.TRAIN, *seg(0)), r.step_block(k, rr.TRAIN, *seg(0)))
    q2, r2 = q.clone(), r.clone()                            # mid-stream: the clone continues with identical words
    q.reset_channel(2), r.reset_channel(2)
    before = q2.get_matrix()
    for a, b in ((q, r), (q2, r2)):
        assert rr.same_words(a.step_block(k, rr.TRAIN, *seg(1)), b.step_block(k, rr.TRAIN, *seg(1)))
        assert rr.state_same(a, b)
    keep = [c for c in range(C) if c != 2]                   # reset_channel left the other columns' words unchanged
    assert rr.same_words(q.get_matrix()[keep], q2.get_matrix()[keep]) and not rr.same_words(before, q2.get_matrix())
    assert rr.same_words(q.get_weights()[keep], q2.get_weights()[keep])
    assert not rr.same_words(q.get_matrix()[2], q2.get_matrix()[2])
    with pytest.raises(ya.ConfigError):
        q.reset_channel(C)
    # recreate with the same p: only h0 changes, nothing is reset until reset()
    h = er.noise(5, 1, p)[0]
    q.recreate(p, h), r.recreate(p, h)
    assert rr.state_same(q, r)
    q.reset(), r.reset()
    assert rr.state_same(q, r) and rr.same_words(q.get_coefficients()[0], h)
    assert rr.same_words(q.step_block(k, rr.TRAIN, *seg(2)), r.step_block(k, rr.TRAIN, *seg(2))) and rr.state_same(q, r)
    # recreate with another p: a new bank
    q.recreate(p + 3), r.recreate(p + 3)
    assert q.get_length() == p + 3 and q.get_bw() == np.float32(0.99) and rr.state_same(q, r)
    assert rr.same_words(q.step_block(k, rr.TRAIN, *seg(0)), r.step_block(k, rr.TRAIN, *seg(0))) and rr.state_same(q, r)
    with pytest.raises(ya.ConfigError):
        q.recreate(rr.LEN_MAX + 1)
    assert q.get_length() == p + 3 and rr.state_same(q, r)


def test_get_weights_is_w1_and_survives_reset(ya):
    C, p = 4, 5
    q = ya.EqRls(C, p)
    assert not q.get_weights().any()
    q.step_block(1, rr.NONE, er.noise(1, 3, C))
    assert not q.get_weights().any()
    q.step_block(1, rr.TRAIN, er.noise(2, 3, C), er.symbols(3, C, 1))
    w = q.get_weights()
    assert w.any() and rr.same_words(w, q.get_coefficients()[:, ::-1])
    q.reset()
    assert rr.same_words(q.get_weights(), w)
    q.step_block(1, rr.NONE, er.noise(3, 3, C))               # a call without an update leaves w1 alone on the device too
    assert rr.same_words(q.get_weights(), w)


@pytest.mark.parametrize("L", [1, 4])
def test_zero_nan_and_inf_channels_keep_to_themselves(ya, L):
    C, p, nsym = 70, 4, 16
    x, d = rr.streams(nsym, C, 31), er.symbols(nsym, C, 32)
    clean = x.copy()
    clean[~np.isfinite(clean)] = 0.25
    out = []
    for xs in (x, clean):
        q = ya.EqRls(C, p)
        q.set_lanes(L)
        y = q.step_block(1, rr.TRAIN, xs, d)
        out.append((y, q.get_coefficients(), q.get_matrix()))
    keep = [c for c in range(C) if c not in (3, 4)]
    (y, w0, P), (yc, w0c, Pc) = out
    assert rr.same_words(y[:, keep], yc[:, keep]) and rr.same_words(w0[keep], w0c[keep]) and rr.same_words(P[keep], Pc[keep])
    for c in (3, 4):
        assert not np.isfinite(P[c]).any() and not np.isfinite(w0[c]).any() and not np.isfinite(y[-1, c])
    assert np.isfinite(P[keep]).all() and not y[:, 1].any() and np.isfinite(P[1]).all()
