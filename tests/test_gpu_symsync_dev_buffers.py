"""SymSync.execute_devptr on tests/dev_arena.py arenas: input, output and the status words sit at offsets inside guarded
allocations filled with 0xFF.  Afterwards the input is intact, the guards are untouched, every y[j][c] with j < ny[c] is
written (and equals tests/symsync_ref.py), and every row >= ny[c] of a channel and every pitch-gap column is still the
sentinel."""
import numpy as np
import pytest

import symsync_ref as sr
from dev_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

#        C   k  m  npfb  pad (pitch - C)  ycap (None: room for all)
CASES = [(65, 2, 7, 32, 0, None), (65, 2, 7, 32, 7, None), (3, 3, 3, 8, 5, None), (130, 5, 7, 64, 1, None),
         (65, 2, 7, 32, 3, 60)]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("C,k,m,npfb,pad,ycap", CASES)
def test_execute_dev_on_arenas(ya, C, k, m, npfb, pad, ycap, off):
    h = ya.SymSync.rnyquist_taps(ya.FirFilterShape.Arkaiser, k, m, 0.35, npfb)
    q, r = ya.SymSync(C, k, npfb, h), sr.SymSyncRef(C, k, npfb, h)
    pitch, n = C + pad, 120
    x = sr.streams(k, 2 * n, C, 40 + C)
    room = sr.default_ycap(n, k, 1) + 20 if ycap is None else ycap
    for part in (x[:n], x[n:]):                                    # the second call reads the state the first left
        want = r.execute(part, room)
        assert want[2].any() == (ycap is not None)
        wide = np.full((n, pitch), 3 - 2j, np.complex64)
        wide[:, :C] = part
        span = (n - 1) * pitch + C                                  # the last row ends at its last channel
        ax = Arena(ya, np.complex64, span, off=off).load(wide.reshape(-1)[:span])
        ay = Arena(ya, np.complex64, (room - 1) * pitch + C, off=(off + 1) % 4)
        ast = Arena(ya, np.uint32, 2 * C, off=(off + 2) % 4)
        q.execute_devptr(ax.ptr, pitch, n, ay.ptr, pitch, room, ast.ptr)
        status = ast.fetch_output()
        ny, st = status[:C], status[C:]
        ax.assert_input_intact(wide.reshape(-1)[:span])
        a, u, w = ay._words()
        ay._check_guards(u, w)
        body = np.full(room * pitch, np.complex64(0), np.complex64)
        body[:ay.n] = a[ay.first:ay.first + ay.n]
        words = body.view(np.uint32).reshape(room, pitch, 2)
        written = np.zeros((room, pitch), bool)
        for c in range(C):
            written[:ny[c], c] = True
        flat = written.reshape(-1)[:ay.n]
        got_words = words.reshape(-1, 2)[:ay.n]
        assert (got_words[~flat] == SENTINEL).all(), "a row >= ny[c] or a pitch-gap column was written"
        assert (got_words[flat] != SENTINEL).all(), "an output below ny[c] was not written"
        assert sr.same_outputs((body.reshape(room, pitch)[:, :C], ny, st), want), (C, k, off)
        assert sr.same_words(q.get_tau(), r.get_tau())
        for arena in (ax, ay, ast):
            arena.free()


def test_an_empty_call_writes_the_status_only(ya):
    C = 5
    h = ya.SymSync.rnyquist_taps(ya.FirFilterShape.Arkaiser, 2, 3, 0.35, 8)
    q = ya.SymSync(C, 2, 8, h)
    ast = Arena(ya, np.uint32, 2 * C, off=1)
    q.execute_devptr(None, C, 0, None, C, 0, ast.ptr)
    assert ast.fetch_output().tolist() == [0] * (2 * C)
    ast.free()


def test_bad_block_arguments_are_config_errors(ya):
    C = 5
    h = ya.SymSync.rnyquist_taps(ya.FirFilterShape.Arkaiser, 2, 3, 0.35, 8)
    q = ya.SymSync(C, 2, 8, h)
    xd, yd, sd = ya.DeviceArray(64, np.complex64), ya.DeviceArray(64, np.complex64), ya.DeviceArray(2 * C, np.uint32)
    for args in [(xd.ptr, C - 1, 4, yd.ptr, C, 8, sd.ptr), (xd.ptr, C, 4, yd.ptr, C - 1, 8, sd.ptr),
                 (xd.ptr, C, 2 ** 31, yd.ptr, C, 8, sd.ptr), (xd.ptr, C, 4, yd.ptr, C, 2 ** 31, sd.ptr),
                 (None, C, 4, yd.ptr, C, 8, sd.ptr), (xd.ptr, C, 4, None, C, 8, sd.ptr), (xd.ptr, C, 4, yd.ptr, C, 8, None)]:
        with pytest.raises(ya.ConfigError):
            q.execute_devptr(*args)
    with pytest.raises(ya.ConfigError):
        q.reset_channel(C)
    assert not q.get_stalled().any() and not q.get_tau().any()
