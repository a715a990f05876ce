"""Channel.execute_devptr and execute_bcast_devptr on tests/dev_arena.py arenas: x and y sit at offsets inside guarded
allocations filled with 0xFF, with pitches wider than the channel count.  Afterwards the input is intact, the guards are
untouched, exactly the n x C words of y are written and equal tests/channel_ref.py, and every pitch-gap column is still
the sentinel.  The streams are finite here: a sentinel word is a NaN pattern.  One case runs on a caller's stream."""
import numpy as np
import pytest

import channel_ref as cr
from dev_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

#        C  L  pad (pitch - C)
CASES = [(65, 5, 0), (65, 17, 7), (3, 2, 5), (130, 1, 1), (1, cr.TAPS_MAX, 3)]
N = 40
SEED = 9


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def widen(a, pitch, fill):
    rows, C = a.shape
    wide = np.full((rows, pitch), fill, a.dtype)
    wide[:, :C] = a
    span = (rows - 1) * pitch + C                               # the last row ends at its last channel
    return wide.reshape(-1)[:span], span


def pair(ya, C, L):
    q, r = ya.Channel(C, L, ya.OscScheme.Vco), cr.ChannelRef(C, L, True)
    for o in (q, r):
        cr.configure(o, C, L)
    q.set_seed(SEED)
    r.seed = SEED
    return q, r


def check_output(ay, pitch, C, want):
    a, u, w = ay._words()
    ay._check_guards(u, w)
    body = np.zeros(N * pitch, np.complex64)
    body[:ay.n] = a[ay.first:ay.first + ay.n]
    written = np.zeros((N, pitch), bool)
    written[:, :C] = True
    flat = written.reshape(-1)[:ay.n]
    words = body.view(np.uint32).reshape(N * pitch, w)[:ay.n]
    assert (words[~flat] == SENTINEL).all(), "a pitch-gap column was written"
    assert (words[flat] != SENTINEL).all(), "an output was not written"
    assert cr.same_words(body.reshape(N, pitch)[:, :C], want)


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("C,L,pad", CASES)
def test_block_calls_on_arenas(ya, C, L, pad, off):
    pitch = C + pad
    x = cr.streams(2 * N, C, 40 + C)
    q, r = pair(ya, C, L)
    span = (N - 1) * pitch + C
    for half in (0, 1):                                          # the second call reads the window the first left
        xs = x[half * N:(half + 1) * N]
        want = r.execute_block(xs)
        xflat, _ = widen(xs, pitch, 3)
        ax = Arena(ya, np.complex64, span, off=off).load(xflat)
        ay = Arena(ya, np.complex64, span, off=(off + 1) % 4)
        q.execute_devptr(ax.ptr, pitch, N, ay.ptr, pitch)
        ax.assert_input_intact(xflat)
        check_output(ay, pitch, C, want)
        for arena in (ax, ay):
            arena.free()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("C,L,pad", CASES)
def test_bcast_calls_on_arenas(ya, C, L, pad, off):
    pitch = C + pad
    x = cr.streams(2 * N, 1, 50 + C)[:, 0]
    q, r = pair(ya, C, L)
    span = (N - 1) * pitch + C
    for half in (0, 1):
        xs = x[half * N:(half + 1) * N]
        want = r.execute_block(xs)
        ax = Arena(ya, np.complex64, N, off=off).load(xs)        # exactly n samples: nothing behind them is read
        ay = Arena(ya, np.complex64, span, off=(off + 2) % 4)
        q.execute_bcast_devptr(ax.ptr, N, ay.ptr, pitch)
        ax.assert_input_intact(xs)
        check_output(ay, pitch, C, want)
        for arena in (ax, ay):
            arena.free()


def test_an_empty_call_touches_nothing(ya):
    C = 5
    q, _ = pair(ya, C, 3)
    ay = Arena(ya, np.complex64, 4 * C, off=1)
    q.execute_devptr(None, C, 0, None, C)
    q.execute_devptr(None, C, 0, ay.ptr, C)
    q.execute_bcast_devptr(None, 0, ay.ptr, C)
    a, u, w = ay._words()
    assert (u == SENTINEL).all()
    assert list(q.get_position()) == [0] * C
    ay.free()


def test_a_callers_stream(ya):
    """the calls are ordered on the object's stream: two calls and the window between them, no synchronize in between"""
    import torch
    C, L, pitch = 70, 9, 72
    x = cr.streams(2 * N, C, 77)
    q, r = pair(ya, C, L)
    want = [r.execute_block(x[:N]), r.execute_block(x[N:])]
    span = (N - 1) * pitch + C
    st = torch.cuda.Stream()
    q.set_stream(st.cuda_stream)
    arenas = []
    for half in (0, 1):
        xflat, _ = widen(x[half * N:(half + 1) * N], pitch, 3)
        arenas.append((Arena(ya, np.complex64, span, off=1).load(xflat), Arena(ya, np.complex64, span, off=2), xflat))
    ya.synchronize()
    for ax, ay, _ in arenas:
        q.execute_devptr(ax.ptr, pitch, N, ay.ptr, pitch)
    st.synchronize()
    for (ax, ay, xflat), w in zip(arenas, want):
        ax.assert_input_intact(xflat)
        check_output(ay, pitch, C, w)
        ax.free(), ay.free()
    q.set_stream(0)
