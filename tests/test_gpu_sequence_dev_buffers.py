"""The three device-pointer forms of MSequence and BSequence on tests/dev_arena.py arenas, as
tests/test_gpu_ordfilt_dev_buffers.py does for OrdFilt: every operand sits at an offset inside a guarded allocation
filled with 0xFF; afterwards the input is intact, every output element is written, the guards are untouched, the result
equals tests/sequence_ref.py and a second call reads the state the first one left.

The byte operands (bits, symbols) are carved out of uint32 arenas at a BYTE offset, so their sentinel check is made here
on bytes: 0xFF is no symbol below 8 bits per symbol; at 8 an unwritten byte shows as a mismatch with the expected value
instead.  A correlation is at most 8192, so no int32 output is the sentinel word."""
import numpy as np
import pytest

import sequence_ref as sr
from dev_arena import GUARD_MIN, Arena

pytestmark = pytest.mark.gpu
MT, BT, NMAX = sr.MSEQUENCE_TILE, sr.BSEQUENCE_TILE, sr.BSEQUENCE_NMAX
GUARD = max(GUARD_MIN, MT + NMAX)                                   # elements of 4 bytes: more than a tile plus NMAX


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


class ByteArena:
    """n bytes `off` bytes behind an Arena's operand start"""

    def __init__(self, ya, n, off):
        self.n, self.off = n, off
        self.a = Arena(ya, np.uint32, (n + off + 3) // 4 + 1, off=1, guard=GUARD)
        self.ptr = self.a.ptr + off
        self.lo = self.a.first * 4 + off

    def load(self, host):
        host = np.ascontiguousarray(host, np.uint8)
        assert host.size == self.n
        raw = self.a.dev.to_numpy().view(np.uint8).copy()
        raw[self.lo:self.lo + self.n] = host
        rc = self.a.ya.lib.yagi_hip_memcpy_h2d(self.a.dev.ptr, raw.ctypes.data, raw.nbytes)
        assert rc == 0
        return self

    def fetch(self, sentinel_free=True):
        self.a.ya.synchronize()
        raw = self.a.dev.to_numpy().view(np.uint8)
        assert np.all(raw[:self.lo] == 0xFF), "wrote in front of the operand"
        assert np.all(raw[self.lo + self.n:] == 0xFF), "wrote behind the operand"
        y = raw[self.lo:self.lo + self.n].copy()
        if sentinel_free:
            assert not np.any(y == 0xFF), "an output byte was never written"
        return y

    def free(self):
        self.a.free()


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("m,g,bps,n", [(7, 0x60, 0, 17), (16, 0xD008, 3, MT + 1), (31, 0x40000004, 8, 3 * MT + 17),
                                       (3, 0x6, 1, MT - 1)])
def test_generate_devptr_on_arenas(ya, m, g, bps, n, off):
    """bps = 0 stands for generate_bits_block_devptr"""
    q, r = ya.MSequence(m, g), sr.MSequence(m, g)
    for _ in range(2):                                              # the second call continues the first's stream
        ay = ByteArena(ya, n, off)
        if bps == 0:
            q.generate_bits_block_devptr(n, ay.ptr)
        else:
            q.generate_symbols_block_devptr(bps, n, ay.ptr)
        want = r.symbols(max(bps, 1), n)
        assert ay.fetch(sentinel_free=bps < 8).tobytes() == want.tobytes(), (m, bps, n, off)
        assert q.get_state() == r.state
        ay.free()


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("N,bps,n", [(5, 1, 17), (64, 8, BT + 1), (255, 2, 3 * BT + 17), (NMAX, 3, BT - 1), (1023, 1, 2 * BT)])
def test_push_correlate_devptr_on_arenas(ya, N, bps, n, off):
    rng = np.random.default_rng(N * 10 + off)
    v = rng.integers(0, 256, (N + 7) // 8).astype(np.uint8)
    ref, rref, q, rq = ya.BSequence(N), sr.BSequence(N), ya.BSequence(N), sr.BSequence(N)
    ref.init(v)
    rref.load(v)
    sym = rng.integers(0, 256, 2 * n).astype(np.uint8)
    for part in (sym[:n], sym[n:]):                                 # the second call reads the window of the first
        ax = ByteArena(ya, n, off).load(part)
        ay = Arena(ya, np.int32, n, off=(off + 2) % 4, guard=GUARD)
        q.push_correlate_block_devptr(ref, ax.ptr, n, bps, ay.ptr)
        got = ay.fetch_output()
        assert ax.fetch(sentinel_free=False).tobytes() == part.tobytes()
        assert got.tobytes() == sr.push_correlate(rq, rref, part, bps).tobytes(), (N, bps, n, off)
        ax.free()
        ay.free()
    assert np.array([q.index(i) for i in range(N)], np.uint8).tobytes() == rq.all_bits().tobytes()
    # without rxy: only the input and the state are touched
    ax = ByteArena(ya, n, off).load(sym[:n])
    q.push_correlate_block_devptr(ref, ax.ptr, n, bps, None)
    assert ax.fetch(sentinel_free=False).tobytes() == sym[:n].tobytes()
    sr.push_correlate(rq, rref, sym[:n], bps, want_rxy=False)
    assert np.array([q.index(i) for i in range(N)], np.uint8).tobytes() == rq.all_bits().tobytes()


def test_overlapping_operands_are_config_errors(ya):
    q, ref = ya.BSequence(64), ya.BSequence(64)
    buf = ya.DeviceArray(4096, np.int32)
    with pytest.raises(ya.ConfigError):
        q.push_correlate_block_devptr(ref, buf.ptr + 16, 64, 1, buf.ptr)
