"""tests/eqrls_ref.py against itself and against the reference's own scenarios: the vectorised and the statement-by-
statement forms agree bit for bit, the reference's autotest passes through train, RLS converges through the reference's
7-tap channel, get_weights shows w1, and the configuration errors are those of yagi_hip.h.  No device is needed."""
import numpy as np
import pytest

import eqlms_ref as er
import eqrls_ref as rr
import yagi_amd as ya

MODES = [rr.NONE, rr.TRAIN, rr.DECISION]

# EQRLS_RRRF_AUTOTEST_DATA_SEQUENCE (eqrls.rs:187-196)
SEQUENCE = np.array([
    -1, -1, 1, -1, 1, -1, 1, -1, -1, 1, 1, -1, -1, 1, -1, 1, 1, -1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, -1, -1,
    1, 1, -1, -1, 1, -1, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 1, -1, -1, -1, 1, 1, -1, 1, -1, 1, 1, -1, 1, -1, 1, -1],
    np.complex64)
CHANNEL7 = np.array([1, -0.08, 0.32, 0.01, -0.06, 0.07, -0.03])          # eqrls.rs:252


def run(q, k, mode, x, d=None):
    return q.step_block(k, mode, x, d if mode == rr.TRAIN else None)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("p,k", [(1, 1), (2, 5), (3, 2), (9, 1), (32, 1)])
def test_the_two_forms_agree(p, k, mode):
    C, nsym = 6, 12 + p
    x, d = rr.streams(nsym * k, C, 10 + p, k), er.symbols(nsym, C, p)
    h = er.noise(p, 1, p)[0] if p % 2 else None
    r = rr.EqRlsRef(C, p, h)
    r.set_constellation(er.QAM16_MAP)
    r.set_bw(0.97)
    y = run(r, k, mode, x, d)
    for c in range(C):
        s = rr.EqRlsScalar(p, h)
        s.table = er.QAM16_MAP
        s.set_bw(0.97)
        ys = s.step_block(k, mode, x[:, c], d[:, c])
        assert rr.same_words(ys, y[:, c]), (p, k, mode, c)
        assert rr.same_words(s.get_coefficients(), r.get_coefficients()[c])
        assert rr.same_words(s.get_weights(), r.get_weights()[c])
        assert rr.same_words(s.get_matrix(), r.get_matrix()[c])


def test_autotest_eqrls_01_through_train():
    """autotest_eqrls_rrrf_01 (:198-239) with the real data as complex: the channel is a delta, p = 6, n = 64"""
    p, n, tol = 6, 64, 1e-2
    d = SEQUENCE[:n, None]
    x = d.copy()                                                 # h = [1, 0, 0, 0]
    w = rr.EqRlsRef(1, p).train(np.zeros((1, p), np.complex64), x, d)[0]
    assert abs(w[0] - 1) <= tol and (np.abs(w[1:]) <= tol).all(), w
    y, w0, w1, P0 = ya.EqRls.execute_host(1, p, np.zeros(p, np.complex64), 0.99, 1, x, mode=ya.EqRlsUpdate.TRAIN, d=d)
    assert rr.same_words(w1[:, ::-1], w[None, :])


def test_convergence_through_the_seven_tap_channel():
    """the reference's channel rotated by 0.3 rad, QPSK, noise 0.001, p = 16, 400 symbols: rms |y - d| over the last 16
    symbols is at least ten times smaller than over the first 16 (this seeded draw: 0.00137 against 0.1506)"""
    p, n = 16, 400
    r = np.random.default_rng(7)
    d = er.QPSK_MAP[r.integers(0, 4, n)]
    x = np.convolve(d, CHANNEL7 * np.exp(0.3j))[:n]
    x = (x + 0.001 * (r.standard_normal(n) + 1j * r.standard_normal(n)) * np.sqrt(0.5)).astype(np.complex64)
    q = rr.EqRlsRef(1, p)
    y = q.step_block(1, rr.TRAIN, x[:, None], d[:, None])[:, 0]
    e = np.abs(y.astype(np.complex128) - d)
    first, last = np.sqrt(np.mean(e[:16] ** 2)), np.sqrt(np.mean(e[-16:] ** 2))
    print(f"rms error: first 16 symbols {first:.4g}, last 16 symbols {last:.4g}")
    assert last * 10 <= first, (first, last)
    yh = ya.EqRls.execute_host(1, p, None, 0.99, 1, x[:, None], mode=ya.EqRlsUpdate.TRAIN, d=d[:, None])[0]
    assert rr.same_words(yh[:, 0], y)


def test_get_weights_is_w1():
    """zero between create and the first step, and kept across reset() (:76-88 does not touch w1)"""
    C, p = 3, 5
    q = rr.EqRlsRef(C, p)
    assert not q.get_weights().any() and q.get_coefficients()[:, p - 1].all()
    q.step_block(1, rr.NONE, er.noise(1, 4, C))
    assert not q.get_weights().any()
    q.step_block(1, rr.TRAIN, er.noise(2, 4, C), er.symbols(4, C, 3))
    w = q.get_weights()
    assert w.any() and rr.same_words(w, q.get_coefficients()[:, ::-1])
    q.reset()
    assert rr.same_words(q.get_weights(), w) and not rr.same_words(w, q.get_coefficients()[:, ::-1])
    q.reset_channel(1)
    assert rr.same_words(q.get_weights(), w)


def test_config_errors():
    x = np.zeros((6, 2), np.complex64)
    for p in (0, rr.LEN_MAX + 1):
        with pytest.raises(rr.ConfigError):
            rr.EqRlsRef(2, p)
        with pytest.raises(ya.ConfigError):
            ya.EqRls.execute_host(2, p, None, 0.99, 1, x)
        with pytest.raises(ya.ConfigError):
            ya.EqRls(2, p)                                       # decided before any device is asked for
        with pytest.raises(ya.ConfigError):
            ya.eqrls_plan(2, p)
    for lam in (-0.01, 1.01, float("nan")):
        with pytest.raises(rr.ConfigError):
            rr.EqRlsRef(2, 3).set_bw(lam)
        with pytest.raises(ya.ConfigError):
            ya.EqRls.execute_host(2, 3, None, lam, 1, x)
    for lam in (0.0, 1.0):
        rr.EqRlsRef(2, 3).set_bw(lam)
    with pytest.raises(rr.ConfigError):
        rr.EqRlsRef(2, 3).step_block(4, rr.NONE, x)              # n % k
    with pytest.raises(ya.ConfigError):
        ya.EqRls.execute_host(2, 3, None, 0.99, 4, x)
    with pytest.raises(ya.ConfigError):
        ya.EqRls.execute_host(2, 3, None, 0.99, 0, x)
    with pytest.raises(ya.ConfigError):
        ya.EqRls.execute_host(2, 3, None, 0.99, 1, x, mode=2)    # blind updates are not built
    with pytest.raises(ya.ConfigError):
        ya.EqRls.execute_host(2, 3, None, 0.99, 1, x, mode=ya.EqRlsUpdate.TRAIN)          # no d
    with pytest.raises(ya.ConfigError):
        ya.EqRls.execute_host(2, 3, None, 0.99, 1, x, mode=ya.EqRlsUpdate.DECISION)       # no table
    with pytest.raises(rr.ConfigError):
        rr.EqRlsRef(2, 7).train(np.zeros((2, 7), np.complex64), x, x)                      # n < p
    # channels p p <= 2^26
    C = rr.MATRIX_MAX // (32 * 32)
    assert ya.eqrls_plan(C, 32)[0] in ya.eqrls_plan(C, 32)[2]
    for make in (lambda: ya.eqrls_plan(C + 1, 32), lambda: ya.EqRls(C + 1, 32), lambda: ya.EqRls(rr.CHANNELS_MAX + 1, 1),
                 lambda: ya.EqRls(0, 1)):
        with pytest.raises(ya.ConfigError):
            make()
    with pytest.raises(rr.ConfigError):
        rr.check_design(C + 1, 32)
