"""ConvCode's `_dev` entry points on tests/dev_arena.py arenas, as tests/test_gpu_modem_dev_buffers.py handles byte
buffers: every operand sits at a byte offset of 0, 1 or 3 inside a guarded allocation filled with 0xFF, with pitches wider
than the rows.  Afterwards the inputs are intact, the guards and the pitch gaps are untouched, and exactly the expected
bytes and metric words are written.  Coded bytes are 0 / 1, so a surviving 0xFF there is an unwritten byte; message and
soft bytes may be 0xFF and are compared with the expected values instead."""
import numpy as np
import pytest
import torch

import convcode_ref as cc
from dev_arena import Arena

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


class BytePlane:
    """F rows of `width` bytes at `pitch`, `off` bytes behind an Arena's operand start"""

    def __init__(self, ya, F, width, pitch, off):
        self.F, self.width, self.pitch = F, width, pitch
        self.n = (F - 1) * pitch + width
        self.a = Arena(ya, np.uint32, (self.n + off + 3) // 4 + 1, off=1)
        self.ptr = self.a.ptr + off
        self.lo = self.a.first * 4 + off

    def _rows(self, raw):
        idx = self.lo + np.arange(self.F)[:, None] * self.pitch + np.arange(self.width)[None, :]
        return idx, raw[idx]

    def load(self, rows):
        rows = np.ascontiguousarray(rows, np.uint8)
        assert rows.shape == (self.F, self.width)
        raw = self.a.dev.to_numpy().view(np.uint8).copy()
        raw[self._rows(raw)[0]] = rows
        assert self.a.ya.lib.yagi_hip_memcpy_h2d(self.a.dev.ptr, raw.ctypes.data, raw.nbytes) == 0
        return self

    def fetch(self):
        """the rows; every byte outside them (guards, the offset, the pitch gaps) is still 0xFF"""
        self.a.ya.synchronize()
        raw = self.a.dev.to_numpy().view(np.uint8)
        idx, rows = self._rows(raw)
        outside = np.ones(raw.size, bool)
        outside[idx] = False
        assert np.all(raw[outside] == 0xFF), "wrote outside the rows"
        return rows.copy()


CASES = [(cc.V27, True, 100, 3, 0), (cc.V27, False, 65, 5, 1), (cc.V29, True, 40, 2, 3), (cc.V27P34, True, 77, 6, 1),
         ((3, (7, 5), None), True, 30, 17, 3), (cc.V27P23, False, 9, 1, 0)]


@pytest.mark.parametrize("spec,terminated,n,F,off", CASES)
def test_encode_and_decode_dev_on_arenas(ya, spec, terminated, n, F, off):
    code = cc.Code(*spec, terminated)
    q = ya.ConvCode(*code.args())
    rng = np.random.default_rng(n + off)
    nb, nc = (n + 7) // 8, code.ncoded(n)
    msg = cc.messages(rng, F, n)
    pm, pc = nb + 1 + off, nc + 2 + off
    amsg = BytePlane(ya, F, nb, pm, off).load(msg)
    acoded = BytePlane(ya, F, nc, pc, (off + 1) % 4)
    q.encode_block_devptr(amsg.ptr, pm, n, F, acoded.ptr, pc)
    coded = acoded.fetch()
    assert not np.any(coded == 0xFF), "a coded byte was never written"
    assert np.array_equal(coded, cc.encode(code, msg, n))
    assert np.array_equal(amsg.fetch(), msg)

    soft = np.concatenate([cc.soft_bytes(rng, cc.SOFT_KINDS[f % len(cc.SOFT_KINDS)], 1, nc) for f in range(F)])
    want_msg, want_metric = cc.decode(code, soft, n)
    asoft = BytePlane(ya, F, nc, pc, off).load(soft)
    aout = BytePlane(ya, F, nb, pm, (off + 2) % 4)
    ametric = Arena(ya, np.uint32, F, off=off)
    q.decode_block_devptr(asoft.ptr, pc, n, F, aout.ptr, pm, ametric.ptr)
    assert np.array_equal(aout.fetch(), want_msg)
    assert np.array_equal(ametric.fetch_output(), want_metric)
    assert np.array_equal(asoft.fetch(), soft)
    aout2 = BytePlane(ya, F, nb, pm, off)                                 # without the optional output
    q.decode_block_devptr(asoft.ptr, pc, n, F, aout2.ptr, pm, None)
    assert np.array_equal(aout2.fetch(), want_msg)


def test_on_a_callers_stream(ya):
    code = cc.Code(*cc.V27)
    q = ya.ConvCode.v27()
    n, F = 500, 9
    rng = np.random.default_rng(0)
    nb, nc = (n + 7) // 8, code.ncoded(n)
    soft = rng.integers(0, 256, (F, nc)).astype(np.uint8)
    want_msg, want_metric = cc.decode(code, soft, n)
    asoft = BytePlane(ya, F, nc, nc + 3, 1).load(soft)
    aout = BytePlane(ya, F, nb, nb + 1, 3)
    ametric = Arena(ya, np.uint32, F, off=1)
    stream = torch.cuda.Stream()
    q.set_stream(stream.cuda_stream)
    q.decode_block_devptr(asoft.ptr, nc + 3, n, F, aout.ptr, nb + 1, ametric.ptr)
    stream.synchronize()
    assert np.array_equal(aout.fetch(), want_msg)
    assert np.array_equal(ametric.fetch_output(), want_metric)
    msg = cc.messages(rng, F, n)
    amsg = BytePlane(ya, F, nb, nb, 0).load(msg)
    acoded = BytePlane(ya, F, nc, nc, 1)
    q.encode_block_devptr(amsg.ptr, nb, n, F, acoded.ptr, nc)
    stream.synchronize()
    assert np.array_equal(acoded.fetch(), cc.encode(code, msg, n))
    q.set_stream(None)


def test_overlapping_or_misplaced_operands_are_config_errors(ya):
    q = ya.ConvCode.v27()
    buf = ya.DeviceArray(8192, np.uint8)
    n, F = 10, 4                                                          # rows of 2 and 32 bytes
    with pytest.raises(ya.ConfigError):
        q.encode_block_devptr(buf.ptr, 2, n, F, buf.ptr + 4, 32)
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(buf.ptr, 32, n, F, buf.ptr + 127, 2, None)
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(buf.ptr, 32, n, F, buf.ptr + 1024, 2, buf.ptr + 1028)      # the metric inside msg
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(buf.ptr, 32, n, F, buf.ptr + 1024, 2, buf.ptr + 2049)      # the metric not 4-byte aligned
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(buf.ptr, 31, n, F, buf.ptr + 1024, 2, None)                # a pitch below the row
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(None, 32, n, F, buf.ptr + 1024, 2, None)
    q.decode_block_devptr(buf.ptr, 32, n, F, buf.ptr + 1024, 2, buf.ptr + 2048)          # the good call
    ya.synchronize()
