"""EqLms.execute_block_devptr and decim_block_devptr on tests/dev_arena.py arenas: x, d and y sit at offsets inside
guarded allocations filled with 0xFF, with pitches wider than C.  Afterwards the inputs are intact, the guards are
untouched, exactly the first n rows (n / k for decim_block) of the C channels of y are written and equal tests/eqlms_ref.py,
and every pitch-gap column is still the sentinel.  The streams are finite here: a sentinel word is a NaN pattern."""
import numpy as np
import pytest

import eqlms_ref as er
from dev_arena import SENTINEL, Arena
from test_eqlms_ref_cpu import MODES, run

pytestmark = pytest.mark.gpu

#        C  h_len  k  pad (pitch - C)
CASES = [(65, 29, 2, 0), (65, 29, 2, 7), (3, 2, 5, 5), (130, 65, 1, 1)]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def widen(a, pitch, fill):
    rows, C = a.shape
    wide = np.full((rows, pitch), fill, np.complex64)
    wide[:, :C] = a
    span = (rows - 1) * pitch + C                               # the last row ends at its last channel
    return wide.reshape(-1)[:span], span


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C,h_len,k,pad", CASES)
def test_block_calls_on_arenas(ya, C, h_len, k, pad, mode, off):
    pitch, nsym = C + pad, 10 + -(-h_len // k)
    n = nsym * k
    rows = n if mode is None else nsym
    x = er.noise(40 + C, 2 * n, C, np.array([0.5, 2.0, 1.0])[np.arange(C) % 3])
    d = er.symbols(2 * nsym, C, 1)
    q, r = ya.EqLms(C, h_len), er.EqLmsRef(C, h_len)
    q.set_bw(0.1), r.set_bw(0.1)
    q.set_constellation(er.QPSK_MAP), r.set_constellation(er.QPSK_MAP)
    for half in (0, 1):                                          # the second call reads the state the first left
        xs, ds = x[half * n:(half + 1) * n], d[half * nsym:(half + 1) * nsym]
        want = run(r, k, mode, xs, ds if mode == er.TRAIN else None)
        xflat, xspan = widen(xs, pitch, 3 - 2j)
        dflat, dspan = widen(ds, pitch, 2 - 3j)
        ax = Arena(ya, np.complex64, xspan, off=off).load(xflat)
        ad = Arena(ya, np.complex64, dspan, off=(off + 2) % 4).load(dflat)
        ay = Arena(ya, np.complex64, (rows - 1) * pitch + C, off=(off + 1) % 4)
        if mode is None:
            q.execute_block_devptr(k, ax.ptr, pitch, n, ay.ptr, pitch)
        else:
            q.decim_block_devptr(k, ya.EqLmsUpdate(mode), ax.ptr, pitch, n, ad.ptr if mode == er.TRAIN else None, pitch,
                                 ay.ptr, pitch)
        ax.assert_input_intact(xflat)
        ad.assert_input_intact(dflat)
        a, u, w = ay._words()
        ay._check_guards(u, w)
        body = np.zeros(rows * pitch, np.complex64)
        body[:ay.n] = a[ay.first:ay.first + ay.n]
        written = np.zeros((rows, pitch), bool)
        written[:, :C] = True
        flat = written.reshape(-1)[:ay.n]
        words = body.view(np.uint32).reshape(-1, 2)[:ay.n]
        assert (words[~flat] == SENTINEL).all(), "a pitch-gap column was written"
        assert (words[flat] != SENTINEL).all(), "an output was not written"
        assert er.same_words(body.reshape(rows, pitch)[:, :C], want), (C, h_len, k, mode, off, half)
        assert er.same_words(q.get_coefficients(), r.get_coefficients())
        for arena in (ax, ad, ay):
            arena.free()


def test_nothing_beyond_the_rows_of_the_call_is_touched(ya):
    """y has room for more rows than the call writes: the rows behind n (or n / k) keep the sentinel"""
    C, h_len, k, pitch, n, room = 70, 13, 2, 75, 40, 64
    x = er.noise(3, n, C)
    xflat, xspan = widen(x, pitch, 1 + 1j)
    for mode, rows in ((None, n), (er.BLIND, n // k)):
        q = ya.EqLms(C, h_len)
        ax = Arena(ya, np.complex64, xspan, off=1).load(xflat)
        ay = Arena(ya, np.complex64, room * pitch, off=3)
        if mode is None:
            q.execute_block_devptr(k, ax.ptr, pitch, n, ay.ptr, pitch)
        else:
            q.decim_block_devptr(k, ya.EqLmsUpdate(mode), ax.ptr, pitch, n, None, pitch, ay.ptr, pitch)
        a, u, w = ay._words()
        ay._check_guards(u, w)
        words = a[ay.first:ay.first + ay.n].view(np.uint32).reshape(room, pitch, 2)
        assert (words[:rows, :C] != SENTINEL).all() and (words[:rows, C:] == SENTINEL).all()
        assert (words[rows:] == SENTINEL).all(), "a row behind the call's last was written"
        ax.free(), ay.free()


def test_an_empty_call_touches_nothing(ya):
    C = 5
    q = ya.EqLms(C, 7)
    ay = Arena(ya, np.complex64, 4 * C, off=1)
    q.execute_block_devptr(2, None, C, 0, None, C)
    q.decim_block_devptr(2, ya.EqLmsUpdate.BLIND, None, C, 0, None, C, ay.ptr, C)
    a, u, w = ay._words()
    assert (u == SENTINEL).all()
    ay.free()
