"""Packetizer's `_dev` entry points on tests/dev_arena.py arenas, as tests/test_gpu_convcode_dev_buffers.py does for
ConvCode: every operand sits at a byte offset of 0, 1 or 3 inside a guarded allocation filled with 0xFF, with pitches wider
than the rows.  Afterwards the inputs are intact, the guards and the pitch gaps are untouched, and exactly the expected
bytes and words are written.  Transmit bytes at bps < 8 and valid flags cannot be 0xFF, so a surviving 0xFF there is an
unwritten byte; payload and soft bytes may be 0xFF and are compared with the expected values instead.  The last soft row
ends flush with the guard behind it in one case: the decoder loads bytes, so a read past a row would meet the guard's 0xFF
and change the metric."""
import numpy as np
import pytest
import torch

import convcode_ref as cc
import packetizer_ref as pr
from dev_arena import Arena
from test_gpu_convcode_dev_buffers import BytePlane

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def soft_rows(rng, pk, payload, F):
    """transmit-order soft rows: convcode_ref's kinds, and every third row a codeword of this packet"""
    clean = pr.encode(pk, payload) * np.uint8(255)
    rows = [clean[f] if f % 3 == 2 else cc.soft_bytes(rng, cc.SOFT_KINDS[f % len(cc.SOFT_KINDS)], 1, pk.N)[0] for f in range(F)]
    return np.stack(rows)


#         code, terminated, n, crc, columns, scramble, F, off, bps, soft gap
CASES = [(cc.V27, True, 12, pr.CRC_32, 14, True, 3, 0, 2, 2),
         (cc.V27, False, 9, pr.CRC_16, 1, False, 5, 1, 1, 0),            # soft rows back to back, the last flush with the guard
         (cc.V29, True, 5, pr.CRC_24, 9, True, 2, 3, 3, 1),
         (cc.V27P34, True, 10, pr.CRC_8, 13, True, 6, 1, 7, 3),
         ((3, (7, 5), None), True, 4, pr.CRC_NONE, 5, True, 17, 3, 2, 1),
         (cc.V27P23, False, 1, pr.CRC_32, 100, False, 1, 0, 1, 0)]


@pytest.mark.parametrize("spec,terminated,n,scheme,C,scramble,F,off,bps,gap", CASES)
def test_encode_and_decode_dev_on_arenas(ya, spec, terminated, n, scheme, C, scramble, F, off, bps, gap):
    pk = pr.Packet(cc.Code(*spec, terminated), n, scheme, C, scramble)
    q = ya.Packetizer(*pk.args())
    rng = np.random.default_rng(n + off)
    payload = rng.integers(0, 256, (F, n)).astype(np.uint8)
    ns = pk.nsym(bps)
    pp, pt, ps = n + 1 + off, ns + 2 + off, pk.N + gap
    apay = BytePlane(ya, F, n, pp, off).load(payload)
    atx = BytePlane(ya, F, ns, pt, (off + 1) % 4)
    q.encode_block_devptr(apay.ptr, pp, F, bps, atx.ptr, pt)
    tx = atx.fetch()
    assert not np.any(tx == 0xFF), "a transmit byte was never written"
    assert np.array_equal(tx, pr.encode(pk, payload, bps))
    assert np.array_equal(apay.fetch(), payload)

    soft = soft_rows(rng, pk, payload, F)
    want = pr.decode(pk, soft)
    asoft = BytePlane(ya, F, pk.N, ps, off).load(soft)
    aout = BytePlane(ya, F, n, pp, (off + 2) % 4)
    avalid = BytePlane(ya, 1, F, F, (off + 3) % 4)
    acrc, ametric = Arena(ya, np.uint32, F, off=off), Arena(ya, np.uint32, F, off=off + 1)
    q.decode_block_devptr(asoft.ptr, ps, F, aout.ptr, pp, avalid.ptr, acrc.ptr, ametric.ptr)
    assert np.array_equal(aout.fetch(), want[0])
    valid = avalid.fetch()[0]
    assert not np.any(valid == 0xFF) and np.array_equal(valid, want[1])
    assert np.array_equal(acrc.fetch_output(), want[2])
    assert np.array_equal(ametric.fetch_output(), want[3])
    assert np.array_equal(asoft.fetch(), soft)
    aout2, avalid2 = BytePlane(ya, F, n, pp, off), BytePlane(ya, 1, F, F, off)      # without the optional outputs
    q.decode_block_devptr(asoft.ptr, ps, F, aout2.ptr, pp, avalid2.ptr, None, None)
    assert np.array_equal(aout2.fetch(), want[0]) and np.array_equal(avalid2.fetch()[0], want[1])


def test_on_a_callers_stream(ya):
    pk = pr.Packet(cc.Code(*cc.V27), 60, pr.CRC_32, 31, True)
    q = ya.Packetizer(*pk.args())
    F = 9
    rng = np.random.default_rng(0)
    payload = rng.integers(0, 256, (F, pk.n)).astype(np.uint8)
    soft = soft_rows(rng, pk, payload, F)
    want = pr.decode(pk, soft)
    asoft = BytePlane(ya, F, pk.N, pk.N + 3, 1).load(soft)
    aout = BytePlane(ya, F, pk.n, pk.n + 1, 3)
    avalid = BytePlane(ya, 1, F, F, 1)
    acrc, ametric = Arena(ya, np.uint32, F, off=1), Arena(ya, np.uint32, F, off=2)
    stream = torch.cuda.Stream()
    q.set_stream(stream.cuda_stream)
    q.decode_block_devptr(asoft.ptr, pk.N + 3, F, aout.ptr, pk.n + 1, avalid.ptr, acrc.ptr, ametric.ptr)
    stream.synchronize()
    assert np.array_equal(aout.fetch(), want[0]) and np.array_equal(avalid.fetch()[0], want[1])
    assert np.array_equal(acrc.fetch_output(), want[2]) and np.array_equal(ametric.fetch_output(), want[3])
    apay = BytePlane(ya, F, pk.n, pk.n, 0).load(payload)
    atx = BytePlane(ya, F, pk.nsym(2), pk.nsym(2), 1)
    q.encode_block_devptr(apay.ptr, pk.n, F, 2, atx.ptr, pk.nsym(2))
    stream.synchronize()
    assert np.array_equal(atx.fetch(), pr.encode(pk, payload, 2))
    q.set_stream(None)


def test_overlapping_or_misplaced_operands_are_config_errors(ya):
    q = ya.Packetizer.v27(4)                                              # rows of 4 payload and 140 soft bytes
    assert q.enc_len() == 140
    buf = ya.DeviceArray(16384, np.uint8)
    F, b = 4, buf.ptr
    with pytest.raises(ya.ConfigError):
        q.encode_block_devptr(b, 4, F, 1, b + 8, 140)
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(b, 140, F, b + 559, 4, b + 4096)                      # the payload inside the soft plane
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(b, 140, F, b + 1024, 4, b + 1030)                     # valid inside the payload
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(b, 140, F, b + 1024, 4, b + 4096, b + 4096)           # crc on valid
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(b, 140, F, b + 1024, 4, b + 4096, b + 8192, b + 8200)  # metric inside crc
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(b, 140, F, b + 1024, 4, b + 4096, b + 8193)           # crc not 4-byte aligned
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(b, 140, F, b + 1024, 4, b + 4096, None, b + 8194)     # metric not 4-byte aligned
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(b, 139, F, b + 1024, 4, b + 4096)                     # a pitch below the row
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(b, 140, F, b + 1024, 4, None)                         # valid is not optional
    with pytest.raises(ya.ConfigError):
        q.decode_block_devptr(None, 140, F, b + 1024, 4, b + 4096)
    q.decode_block_devptr(b, 140, F, b + 1024, 4, b + 4096, b + 8192, b + 12288)    # the good call
    ya.synchronize()
