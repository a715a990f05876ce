"""SymTrack.execute_devptr on tests/dev_arena.py arenas: input, both outputs and the status words sit at offsets inside
guarded allocations filled with 0xFF.  Afterwards the input is intact, the guards are untouched, every y[j][c] and
sym[j][c] with j < ny[c] is written (and equals tests/symtrack_ref.py), and every row >= ny[c] of a channel and every
pad column is still the sentinel.  The symbol plane is bytes: its arena is one of 32-bit words read back as bytes, and
its operand starts at any byte.  sym_dev = NULL and a non-default stream are covered too."""
import numpy as np
import pytest

import symtrack_ref as sr
from dev_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

FT, BETA = sr.FT, sr.BETA
#        C   k  m  npfb  eq_len  pad  ycap (None: room for all)  symbols
CASES = [(65, 2, 2, 8, 9, 0, None, True), (65, 2, 2, 8, 9, 3, None, True), (3, 3, 2, 8, 2, 5, None, False),
         (130, 2, 2, 8, 2, 1, 14, True)]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("C,k,m,npfb,eq_len,pad,ycap,symbols", CASES)
def test_execute_dev_on_arenas(ya, oracle, C, k, m, npfb, eq_len, pad, ycap, symbols, off):
    q = ya.SymTrack(C, FT, k, m, BETA, ya.ModulationScheme.Qam16, ya.OscScheme.Nco, npfb, eq_len)
    r = sr.SymTrackRef(C, FT, k, m, BETA, "Qam16", False, npfb, eq_len)
    for o in (q, r):
        o.set_eq_holdoff(3)
    pitch, n = C + pad, 40
    x = sr.streams(40 + C, "Qam16", 2 * n, C, k, m, BETA)
    room = q.default_ycap(n) + 6 if ycap is None else ycap
    for part in (x[:n], x[n:]):                                    # the second call reads the state the first left
        want = r.execute(part, room)
        assert want[3].any() == (ycap is not None)
        wide = np.full((n, pitch), 3 - 2j, np.complex64)
        wide[:, :C] = part
        span = (n - 1) * pitch + C                                  # the last row ends at its last channel
        ax = Arena(ya, np.complex64, span, off=off).load(wide.reshape(-1)[:span])
        ay = Arena(ya, np.complex64, (room - 1) * pitch + C, off=(off + 1) % 4)
        ast = Arena(ya, np.uint32, 3 * C, off=(off + 2) % 4)
        nbytes = (room - 1) * pitch + C
        ab = Arena(ya, np.uint32, -(-(nbytes + off) // 4), off=off)   # the operand: nbytes bytes from byte `off` of it
        q.execute_devptr(ax.ptr, pitch, n, ay.ptr, pitch, ab.ptr + off if symbols else None, pitch, room, ast.ptr)
        status = ast.fetch_output()
        ny, st = status[:C], status[C:2 * C]
        assert np.array_equal(status[2 * C:], r.get_num_syms().astype(np.uint32))
        ax.assert_input_intact(wide.reshape(-1)[:span])
        written = np.zeros((room, pitch), bool)
        for c in range(C):
            written[:ny[c], c] = True
        flat = written.reshape(-1)[:ay.n]

        a, u, w = ay._words()
        ay._check_guards(u, w)
        body = np.full(room * pitch, np.complex64(0), np.complex64)
        body[:ay.n] = a[ay.first:ay.first + ay.n]
        got_words = body.view(np.uint32).reshape(-1, 2)[:ay.n]
        assert (got_words[~flat] == SENTINEL).all(), "a row >= ny[c] or a pad column of y was written"
        assert (got_words[flat] != SENTINEL).all(), "a symbol below ny[c] was not written"

        a, u, w = ab._words()
        ab._check_guards(u, w)
        by = u[ab.first:ab.first + ab.n].view(np.uint8)
        sym = None
        if symbols:
            assert (by[:off] == 0xFF).all() and (by[off + nbytes:] == 0xFF).all(), "a byte outside the symbol plane was written"
            plane = np.full(room * pitch, 0xFF, np.uint8)
            plane[:nbytes] = by[off:off + nbytes]
            assert (plane[:nbytes][~flat] == 0xFF).all(), "a row >= ny[c] or a pad column of sym was written"
            assert (plane[:nbytes][flat] < 16).all(), "a decision below ny[c] was not written"
            sym = plane.reshape(room, pitch)[:, :C]
        else:
            assert (by == 0xFF).all(), "sym_dev = NULL and the plane was written"
        bad = sr.same_outputs((body.reshape(room, pitch)[:, :C], sym, ny, st), (want[0], want[1] if symbols else None, want[2], want[3]))
        assert not bad, (C, k, off, bad)
        assert not sr.same_getters(q, r)
        for arena in (ax, ay, ast, ab):
            arena.free()


def test_a_non_default_stream(ya, oracle):
    import torch
    C, k, m, npfb, n = 65, 2, 2, 8, 40
    q = ya.SymTrack(C, FT, k, m, BETA, ya.ModulationScheme.Qpsk, ya.OscScheme.Vco, npfb, 9)
    r = sr.SymTrackRef(C, FT, k, m, BETA, "Qpsk", True, npfb, 9)
    stream = torch.cuda.Stream()
    q.set_stream(stream.cuda_stream)
    x = sr.streams(7, "Qpsk", 2 * n, C, k, m, BETA)
    room = q.default_ycap(n)
    for part in (x[:n], x[n:]):
        want = r.execute(part, room)
        xd = ya.DeviceArray.from_numpy(part)
        yd, bd, sd = ya.DeviceArray(room * C, np.complex64), ya.DeviceArray(room * C, np.uint8), ya.DeviceArray(3 * C, np.uint32)
        q.execute_devptr(xd.ptr, C, n, yd.ptr, C, bd.ptr, C, room, sd.ptr)
        stream.synchronize()
        status = sd.to_numpy()
        got = (yd.to_numpy().reshape(room, C), bd.to_numpy().reshape(room, C), status[:C], status[C:2 * C])
        assert not sr.same_outputs(got, want)
        assert not sr.same_getters(q, r)                             # the getters synchronise on the object's stream
    q.set_stream(0)


def test_an_empty_call_writes_the_status_only(ya):
    C = 5
    q = ya.SymTrack(C, FT, 2, 3, BETA, ya.ModulationScheme.Qpsk)
    ast = Arena(ya, np.uint32, 3 * C, off=1)
    q.execute_devptr(None, C, 0, None, C, None, C, 0, ast.ptr)
    assert ast.fetch_output().tolist() == [0] * (3 * C)
    ast.free()


def test_bad_block_arguments_are_config_errors(ya):
    C = 5
    q = ya.SymTrack(C, FT, 2, 3, BETA, ya.ModulationScheme.Qpsk)
    xd, yd, bd, sd = (ya.DeviceArray(64, np.complex64), ya.DeviceArray(64, np.complex64), ya.DeviceArray(64, np.uint8),
                      ya.DeviceArray(3 * C, np.uint32))
    for args in [(xd.ptr, C - 1, 4, yd.ptr, C, bd.ptr, C, 8, sd.ptr), (xd.ptr, C, 4, yd.ptr, C - 1, bd.ptr, C, 8, sd.ptr),
                 (xd.ptr, C, 4, yd.ptr, C, bd.ptr, C - 1, 8, sd.ptr), (xd.ptr, C, 2 ** 31, yd.ptr, C, bd.ptr, C, 8, sd.ptr),
                 (xd.ptr, C, 4, yd.ptr, C, bd.ptr, C, 2 ** 31, sd.ptr), (None, C, 4, yd.ptr, C, bd.ptr, C, 8, sd.ptr),
                 (xd.ptr, C, 4, None, C, bd.ptr, C, 8, sd.ptr), (xd.ptr, C, 4, yd.ptr, C, bd.ptr, C, 8, None)]:
        with pytest.raises(ya.ConfigError):
            q.execute_devptr(*args)
    for call in (lambda: q.reset_channel(C), lambda: q.set_nco(C, 0.0), lambda: q.set_nco(0, float("inf")),
                 lambda: q.set_nco(0, 0.0, float("-inf")), lambda: q.set_nco_all(np.full(C, 1e30, np.float32)),
                 lambda: q.set_bandwidth(-1.0), lambda: q.set_bandwidths(2.0, 0.0, 0.0, 0.0),
                 lambda: q.set_bandwidths(0.0, 0.0, 0.0, -1.0)):
        with pytest.raises(ya.ConfigError):
            call()
    with pytest.raises(ValueError):
        q.set_eq_strategy(3)
    assert q.get_bandwidth() == np.float32(0.9) and not q.get_stalled().any() and not q.get_nco_state()[1].any()
