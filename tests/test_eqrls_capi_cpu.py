"""yagi_hip_eqrls_cccf_execute_host (the library's host form of EqRls, no device) against tests/eqrls_ref.py, bit for bit:
y, w0, w1 and P0; and yagi_hip_eqrls_plan's answers."""
import numpy as np
import pytest

import eqlms_ref as er
import eqrls_ref as rr
import yagi_amd as ya

LDS_MAX = 160 * 1024


def host(C, p, h, lam, k, mode, x, d, **kw):
    return ya.EqRls.execute_host(C, p, h, lam, k, x, mode=mode, d=d if mode == rr.TRAIN else None,
                                 table=er.QPSK_MAP if mode == rr.DECISION else None, **kw)


def ref(C, p, h, lam, k, mode, x, d):
    r = rr.EqRlsRef(C, p, h)
    r.set_bw(lam)
    r.set_constellation(er.QPSK_MAP)
    y = r.step_block(k, mode, x, d if mode == rr.TRAIN else None)
    return y, r


@pytest.mark.parametrize("mode", [rr.NONE, rr.TRAIN, rr.DECISION])
@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("p", [1, 2, 3, 9, 32])
def test_execute_host_is_the_reference(p, k, mode):
    C, nsym = 7, 12 + p
    x, d = rr.streams(nsym * k, C, 100 * p + k, k), er.symbols(nsym, C, p + k)
    h = er.noise(p + 1, 1, p)[0] if k == 2 else None
    y, w0, w1, P0 = host(C, p, h, 0.99, k, mode, x, d)
    want, r = ref(C, p, h, 0.99, k, mode, x, d)
    assert rr.same_words(y, want)
    assert rr.same_words(w0, r.get_coefficients())
    assert rr.same_words(w1, r.get_weights()[:, ::-1])
    assert rr.same_words(P0, r.get_matrix())
    if mode != rr.NONE:
        # the zero channel stays finite, the NaN and the Inf sample spoil their own columns and no other
        bad = ~np.isfinite(P0).all(axis=(1, 2))
        assert bad.tolist() == [False, False, False, True, True, False, False]
        assert not np.isfinite(w0[3]).any() and not np.isfinite(w0[4]).any()
        assert rr.same_words(w0[1], r.h0) and not y[:, 1].any()


def test_pitches():
    C, p, k, nsym = 5, 3, 2, 9
    x, d = rr.streams(nsym * k, C, 3, k), er.symbols(nsym, C, 4)
    xw, dw = np.full((nsym * k, C + 2), 7 - 1j, np.complex64), np.full((nsym, C + 4), 2 + 2j, np.complex64)
    xw[:, :C], dw[:, :C] = x, d
    y, w0, w1, P0 = host(C, p, None, 0.98, k, rr.TRAIN, xw, dw, x_pitch=C + 2, d_pitch=C + 4, y_pitch=C + 1)
    want, r = ref(C, p, None, 0.98, k, rr.TRAIN, x, d)
    assert rr.same_words(y[:, :C], want) and not y[:, C:].any()
    assert rr.same_words(P0, r.get_matrix())


@pytest.mark.parametrize("lam", [1.0, 0.0])
def test_the_ends_of_lambda(lam):
    """lambda = 1 never forgets; lambda = 0 is accepted and gives the bank Inf / NaN, as in the reference"""
    C, p, nsym = 3, 4, 10
    x, d = er.noise(5, nsym, C), er.symbols(nsym, C, 6)
    y, w0, w1, P0 = host(C, p, None, lam, 1, rr.TRAIN, x, d)
    want, r = ref(C, p, None, lam, 1, rr.TRAIN, x, d)
    assert rr.same_words(y, want) and rr.same_words(w0, r.get_coefficients()) and rr.same_words(P0, r.get_matrix())
    assert np.isfinite(P0).all() == (lam == 1.0)


def test_plan():
    for p in range(1, rr.LEN_MAX + 1):
        for C in (1, 7, 64, 1024, 16384, 65536):
            L, lds, adm = ya.eqrls_plan(C, p)
            assert L in adm and lds <= LDS_MAX
            assert all(1 <= a <= 64 and a & (a - 1) == 0 for a in adm), adm
            assert lds == ya.eqrls_plan(C, p)[1]
        # per channel two matrices of pitch p | 1, six vectors and the staged rows; per wave the table
        need1 = (64 * (2 * p * (p | 1) + 6 * p + 8) + 256) * 8
        assert (1 in adm) == (need1 <= LDS_MAX), (p, need1)
    # the measured choice (profiles/r25_kbench_eqrls.txt): the largest admissible L at every channel count
    for C, p in ((1, 32), (1 << 16, 32), (1, 8), (1 << 20, 8), (64, 12)):
        L, lds, adm = ya.eqrls_plan(C, p)
        assert L == max(adm) and lds == (64 // L * (2 * p * (p | 1) + 6 * p + 8) + 256) * 8
