"""Agc.execute_block_devptr on tests/dev_arena.py arenas: x, y and the status plane sit at offsets inside guarded
allocations filled with 0xFF, with pitches wider than C.  Afterwards the input is intact, the guards are untouched,
exactly the n x C words of y and bytes of status are written and equal tests/agc_ref.py, and every pitch-gap column is
still the sentinel.  The streams are finite here: a sentinel word is a NaN pattern."""
import numpy as np
import pytest

import agc_ref as ar
from dev_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

#        C  pad (pitch - C)
CASES = [(65, 0), (65, 7), (3, 5), (130, 1)]
N = 20


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


def pair(ya, C, kind):
    q, r = ya.Agc(C, kind), ar.AgcRef(C, kind)
    for o in (q, r):
        o.set_bandwidth(0.25), o.set_gain(100.0), o.squelch_enable(), o.squelch_set_threshold(-30.0), o.squelch_set_timeout(3)
    return q, r


class StatusArena(Arena):
    """the status plane is bytes: four to a 32-bit word of the arena, so the arena is sized in words and read as bytes"""

    def __init__(self, ya, nbytes, off):
        super().__init__(ya, np.uint32, -(-nbytes // 4) + 1, off=off)
        self.nbytes = nbytes

    def bytes(self, shift):
        """(all bytes of the allocation, the index of the operand's first byte): the operand starts `shift` bytes into
        its first word"""
        a, u, w = self._words()
        return u.view(np.uint8), self.first * 4 + shift


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("kind", ["crcf", "rrrf"])
@pytest.mark.parametrize("C,pad", CASES)
def test_block_calls_on_arenas(ya, C, pad, kind, off):
    pitch = C + pad
    x = ar.noise(40 + C, 2 * N, C, ar.amplitudes(C), kind)
    q, r = pair(ya, C, kind)
    span = (N - 1) * pitch + C
    for half in (0, 1):                                          # the second call reads the state the first left
        xs = x[half * N:(half + 1) * N]
        wy, wst = r.execute_block(xs)
        xflat, _ = widen(xs, pitch, 3)
        ax = Arena(ya, x.dtype, span, off=off).load(xflat)
        ay = Arena(ya, x.dtype, span, off=(off + 1) % 4)
        ast = StatusArena(ya, span, off=(off + 3) % 4)
        shift = off % 4                                          # the plane also starts off a word boundary
        q.execute_block_devptr(ax.ptr, pitch, N, ay.ptr, pitch, ast.ptr + shift, pitch)
        ax.assert_input_intact(xflat)
        a, u, w = ay._words()
        ay._check_guards(u, w)
        body = np.zeros(N * pitch, x.dtype)
        body[:ay.n] = a[ay.first:ay.first + ay.n]
        written = np.zeros((N, pitch), bool)
        written[:, :C] = True
        flat = written.reshape(-1)[:ay.n]
        words = body.view(np.uint32).reshape(N * pitch, w)[:ay.n]
        assert (words[~flat] == SENTINEL).all(), "a pitch-gap column was written"
        assert (words[flat] != SENTINEL).all(), "an output was not written"
        assert ar.same_words(body.reshape(N, pitch)[:, :C], wy), (C, pad, kind, off, half)
        b, first = ast.bytes(shift)
        assert (b[:first] == 0xFF).all() and (b[first + span:] == 0xFF).all(), "a status byte outside the plane"
        plane = np.full(N * pitch, 0xFF, np.uint8)
        plane[:span] = b[first:first + span]
        plane = plane.reshape(N, pitch)
        assert np.array_equal(plane[:, :C], wst) and (plane[:, C:] == 0xFF).all()
        assert ar.same_words(q.get_gain(), r.get_gain())
        for arena in (ax, ay, ast):
            arena.free()


def test_an_empty_call_touches_nothing(ya):
    C = 5
    q, _ = pair(ya, C, "crcf")
    ay = Arena(ya, np.complex64, 4 * C, off=1)
    ast = StatusArena(ya, 4 * C, off=2)
    q.execute_block_devptr(None, C, 0, None, C)
    q.execute_block_devptr(None, C, 0, ay.ptr, C, ast.ptr, C)
    for arena in (ay, ast):
        a, u, w = arena._words()
        assert (u == SENTINEL).all()
        arena.free()


def test_a_null_status_writes_no_byte(ya):
    C, pitch = 70, 72
    x = ar.noise(2, N, C, 1.0, "crcf")
    q, r = pair(ya, C, "crcf")
    xflat, span = widen(x, pitch, 1)
    ax = Arena(ya, np.complex64, span, off=1).load(xflat)
    ay = Arena(ya, np.complex64, span, off=3)
    spare = StatusArena(ya, span, off=0)                        # a plane the call is not given
    q.execute_block_devptr(ax.ptr, pitch, N, ay.ptr, pitch, None, 0)
    ax.assert_input_intact(xflat)
    a, u, w = ay._words()
    ay._check_guards(u, w)
    got = np.zeros(N * pitch, np.complex64)
    got[:span] = a[ay.first:ay.first + span]
    assert ar.same_words(got.reshape(N, pitch)[:, :C], r.execute_block(x)[0])
    assert (spare._words()[1] == SENTINEL).all()
    for arena in (ax, ay, spare):
        arena.free()
