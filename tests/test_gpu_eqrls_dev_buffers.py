"""EqRls.step_block_devptr and train_devptr on tests/dev_arena.py arenas: x, d and y sit at offsets inside guarded
allocations filled with 0xFF, with pitches wider than C.  Afterwards the inputs are intact, the guards are untouched,
exactly the first n / k rows of the C channels of y are written and equal tests/eqrls_ref.py, and every pitch-gap column is
still the sentinel.  One shape per number of lanes per channel.  The streams are finite here: a sentinel word is a NaN
pattern."""
import numpy as np
import pytest

import eqlms_ref as er
import eqrls_ref as rr
from dev_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

#        L   C   p  k  pad (pitch - C)
CASES = [(1, 65, 5, 2, 7), (2, 33, 2, 1, 0), (4, 17, 3, 5, 5), (8, 9, 8, 2, 1), (16, 130, 9, 1, 3), (32, 3, 32, 1, 2)]
MODES = [rr.NONE, rr.TRAIN, rr.DECISION]


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
@pytest.mark.parametrize("L,C,p,k,pad", CASES)
def test_step_block_on_arenas(ya, L, C, p, k, pad, mode, off):
    pitch, nsym = C + pad, 6 + p // 2
    n = nsym * k
    x = er.noise(40 + C, 2 * n, C, np.array([0.5, 2.0, 1.0])[np.arange(C) % 3])
    d = er.symbols(2 * nsym, C, 1)
    q, r = ya.EqRls(C, p), rr.EqRlsRef(C, p)
    q.set_lanes(L)
    q.set_constellation(er.QPSK_MAP), r.set_constellation(er.QPSK_MAP)
    for half in (0, 1):                                          # the second call reads the state the first left
        xs, ds = x[half * n:(half + 1) * n], d[half * nsym:(half + 1) * nsym]
        want = r.step_block(k, mode, xs, ds if mode == rr.TRAIN else None)
        xflat, xspan = widen(xs, pitch, 3 - 2j)
        dflat, dspan = widen(ds, pitch, 2 - 3j)
        ax = Arena(ya, np.complex64, xspan, off=off).load(xflat)
        ad = Arena(ya, np.complex64, dspan, off=(off + 2) % 4).load(dflat)
        ay = Arena(ya, np.complex64, (nsym - 1) * pitch + C, off=(off + 1) % 4)
        q.step_block_devptr(k, ya.EqRlsUpdate(mode), ax.ptr, pitch, n, ad.ptr if mode == rr.TRAIN else None, pitch,
                            ay.ptr, pitch)
        ax.assert_input_intact(xflat)
        ad.assert_input_intact(dflat)
        a, u, w = ay._words()
        ay._check_guards(u, w)
        body = np.zeros(nsym * pitch, np.complex64)
        body[:ay.n] = a[ay.first:ay.first + ay.n]
        written = np.zeros((nsym, pitch), bool)
        written[:, :C] = True
        flat = written.reshape(-1)[:ay.n]
        words = body.view(np.uint32).reshape(-1, 2)[:ay.n]
        assert (words[~flat] == SENTINEL).all(), "a pitch-gap column was written"
        assert (words[flat] != SENTINEL).all(), "an output was not written"
        assert rr.same_words(body.reshape(nsym, pitch)[:, :C], want), (L, C, p, k, mode, off, half)
        assert rr.state_same(q, r)
        for arena in (ax, ad, ay):
            arena.free()


@pytest.mark.parametrize("L,C,p,k,pad", CASES)
def test_train_on_arenas(ya, L, C, p, k, pad):
    pitch, n = C + pad, p + 5
    x, d = er.noise(50 + C, n, C), er.symbols(n, C, 2)
    w = er.noise(3, C, p, 0.2)
    q, r = ya.EqRls(C, p), rr.EqRlsRef(C, p)
    q.set_lanes(L)
    xflat, xspan = widen(x, pitch, 3 - 2j)
    dflat, dspan = widen(d, pitch + 1, 2 - 3j)
    ax = Arena(ya, np.complex64, xspan, off=1).load(xflat)
    ad = Arena(ya, np.complex64, dspan, off=3).load(dflat)
    q.train_devptr(w, ax.ptr, pitch, n, ad.ptr, pitch + 1)
    ax.assert_input_intact(xflat)
    ad.assert_input_intact(dflat)
    assert rr.same_words(q.get_weights(), r.train(w, x, d)) and rr.state_same(q, r)
    ax.free(), ad.free()


def test_nothing_beyond_the_rows_of_the_call_is_touched(ya):
    """y has room for more rows than the call writes: the rows behind n / k keep the sentinel"""
    C, p, k, pitch, n, room = 70, 7, 2, 75, 24, 40
    x = er.noise(3, n, C)
    xflat, xspan = widen(x, pitch, 1 + 1j)
    q = ya.EqRls(C, p)
    q.set_constellation(er.QPSK_MAP)
    ax = Arena(ya, np.complex64, xspan, off=1).load(xflat)
    ay = Arena(ya, np.complex64, room * pitch, off=3)
    q.step_block_devptr(k, ya.EqRlsUpdate.DECISION, ax.ptr, pitch, n, None, pitch, ay.ptr, pitch)
    a, u, w = ay._words()
    ay._check_guards(u, w)
    words = a[ay.first:ay.first + ay.n].view(np.uint32).reshape(room, pitch, 2)
    rows = n // k
    assert (words[:rows, :C] != SENTINEL).all() and (words[:rows, C:] == SENTINEL).all()
    assert (words[rows:] == SENTINEL).all(), "a row behind the call's last was written"
    ax.free(), ay.free()


def test_an_empty_call_touches_nothing(ya):
    C = 5
    q = ya.EqRls(C, 7)
    ay = Arena(ya, np.complex64, 4 * C, off=1)
    q.step_block_devptr(2, ya.EqRlsUpdate.NONE, None, C, 0, None, C, ay.ptr, C)
    a, u, w = ay._words()
    assert (u == SENTINEL).all()
    ay.free()
