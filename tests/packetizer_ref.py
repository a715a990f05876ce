"""Packetizer restated in numpy (include/yagi_hip.h, "Packetizer: the definition"; a helper, not a test module), built on
convcode_ref.py: a CRC over the payload, ConvCode's encoder, a block interleaver of C columns and the reference's scrambler
(src/random/scramble.rs), and the same stages backwards.  Everything is integer arithmetic, so there is no tolerance."""
import numpy as np

import convcode_ref as cc

CRC_NONE, CRC_8, CRC_16, CRC_24, CRC_32 = range(5)
# scheme: (width, poly, init, reflected, xorout, the check value on b"123456789")
CRC_PARAMS = {
    CRC_NONE: (0, 0, 0, False, 0, 0),
    CRC_8: (8, 0x07, 0x00, False, 0x00, 0xF4),
    CRC_16: (16, 0x1021, 0xFFFF, False, 0x0000, 0x29B1),
    CRC_24: (24, 0x864CFB, 0xB704CE, False, 0x000000, 0x21CF02),
    CRC_32: (32, 0x04C11DB7, 0xFFFFFFFF, True, 0xFFFFFFFF, 0xCBF43926),
}
SCHEMES = tuple(CRC_PARAMS)
COLUMNS_MAX = 1 << 20
SCRAMBLE_MASK = (0xCA, 0xCC, 0x53, 0x5F)


def reflect(v, width):
    return int(format(v, "0%db" % width)[::-1], 2)


def crc(scheme, data):
    """the Rocksoft model bit by bit: most significant bit first, input bytes and the result reflected where the scheme says"""
    width, poly, reg, reflected, xorout, _ = CRC_PARAMS[scheme]
    if width == 0:
        return 0
    top, mask = 1 << (width - 1), (1 << width) - 1
    for byte in bytes(data):
        if reflected:
            byte = reflect(byte, 8)
        reg ^= byte << (width - 8)
        for _ in range(8):
            reg = ((reg << 1) ^ poly) & mask if reg & top else (reg << 1) & mask
    if reflected:
        reg = reflect(reg, width)
    return reg ^ xorout


def crc_len(scheme):
    return CRC_PARAMS[scheme][0] // 8


def perm(N, C):
    """pi[i]: the transmit position of coder-order bit i, by the closed form"""
    i = np.arange(N, dtype=np.int64)
    q, r = N // C, N % C
    return (i % C) * q + np.minimum(i % C, r) + i // C


def perm_inverse(N, C):
    """inv[j]: the coder-order bit sent at transmit position j, by the closed form"""
    j = np.arange(N, dtype=np.int64)
    q, r = N // C, N % C
    head = j < r * (q + 1)
    c = np.where(head, j // (q + 1), r + (j - r * (q + 1)) // max(q, 1))
    rho = np.where(head, j % (q + 1), (j - r * (q + 1)) % max(q, 1))
    return rho * C + c


def perm_matrix(N, C):
    """inv[j] by construction: bit i at row i div C, column i mod C; sent column by column, the missing cells skipped"""
    rows = -(-N // C)
    order = [rho * C + c for c in range(C) for rho in range(rows) if rho * C + c < N]
    return np.array(order, np.int64)


def scramble_mask(N):
    """m(j) for j < N"""
    j = np.arange(N)
    return (np.array(SCRAMBLE_MASK)[(j // 8) % 4] >> (7 - j % 8)) & 1


def scramble_data(x):
    """scramble.rs scramble_data on a copy: every byte, the last partial group of four included"""
    x = np.array(x, np.uint8)
    return x ^ np.array(SCRAMBLE_MASK, np.uint8)[np.arange(x.size) % 4]


unscramble_data = scramble_data


def unscramble_data_soft(x):
    """scramble.rs unscramble_data_soft on a copy: whole groups of eight soft bytes; a shorter tail stays (chunks_exact)"""
    x = np.array(x, np.uint8)
    whole = x.size & ~7
    m = scramble_mask(whole).astype(bool)
    x[:whole][m] = 255 - x[:whole][m]
    return x


def entropy(x):
    """scramble.rs scramble_test_entropy"""
    p1 = np.float32(np.unpackbits(np.asarray(x, np.uint8)).sum()) / np.float32(8 * len(x)) + np.float32(1e-12)
    p0 = np.float32(1) - p1
    return float(-(p0 * np.log2(p0) + p1 * np.log2(p1)))


class Packet:
    """Packetizer(n, crc, code, columns, scramble): the sizes of the definition"""

    def __init__(self, code, n, scheme=CRC_32, columns=1, scramble=True):
        self.code, self.n, self.scheme, self.columns, self.scramble = code, int(n), int(scheme), int(columns), bool(scramble)
        self.w = crc_len(scheme)
        self.msg_bits = 8 * (self.n + self.w)
        self.N = code.ncoded(self.msg_bits)

    def nsym(self, bps):
        return -(-self.N // bps)

    def args(self):
        """(n, crc, K, polys, puncture, terminated, columns, scramble) for yagi_amd.Packetizer and its host forms"""
        return (self.n, self.scheme) + self.code.args() + (self.columns, self.scramble)


def message(pk, payload):
    """payload [F, >= n] -> payload || crc, [F, n + w]"""
    payload = np.asarray(payload, np.uint8)[:, :pk.n]
    tail = np.array([[(crc(pk.scheme, row) >> (8 * (pk.w - 1 - k))) & 0xff for k in range(pk.w)] for row in payload], np.uint8)
    return np.concatenate([payload, tail.reshape(len(payload), pk.w)], axis=1)


def transmit(pk, coded, bps=1):
    """coded [F, N] of 0 / 1 in coder order -> the transmit plane [F, ceil(N / bps)]: interleaved, scrambled, bps bits per
    byte with the first uppermost, the missing bits of the last byte 0"""
    coded = np.asarray(coded, np.uint8)
    F, N = coded.shape
    assert N == pk.N
    tx = np.zeros((F, pk.nsym(bps) * bps), np.uint8)
    tx[:, perm(N, pk.columns)] = coded
    if pk.scramble:
        tx[:, :N] ^= scramble_mask(N).astype(np.uint8)
    weights = 1 << np.arange(bps - 1, -1, -1)
    return (tx.reshape(F, -1, bps) * weights).sum(axis=2).astype(np.uint8)


def receive(pk, soft):
    """soft [F, >= N] in transmit order -> [F, N] in coder order, descrambled: what the code's decoder is given"""
    soft = np.array(np.asarray(soft, np.uint8)[:, :pk.N])
    if pk.scramble:
        m = scramble_mask(pk.N).astype(bool)
        soft[:, m] = 255 - soft[:, m]
    return soft[:, perm(pk.N, pk.columns)]


def sent(pk, ordered):
    """receive backwards: the transmit-order soft bytes that receive() turns into `ordered` [F, N]"""
    ordered = np.asarray(ordered, np.uint8)
    soft = np.zeros_like(ordered)
    soft[:, perm(pk.N, pk.columns)] = ordered
    if pk.scramble:
        m = scramble_mask(pk.N).astype(bool)
        soft[:, m] = 255 - soft[:, m]
    return soft


def encode(pk, payload, bps=1):
    """payload [F, >= n] -> the transmit plane [F, ceil(N / bps)], bps transmit bits per byte, the first uppermost"""
    return transmit(pk, cc.encode(pk.code, message(pk, payload), pk.msg_bits), bps)


def decode(pk, soft):
    """soft [F, >= N] in transmit order -> payload [F, n], valid [F] u8, crc [F] u32, metric [F] u32"""
    msg, metric = cc.decode(pk.code, receive(pk, soft), pk.msg_bits)
    payload = msg[:, :pk.n]
    got = np.array([crc(pk.scheme, row) for row in payload], np.uint32)
    field = np.zeros(len(msg), np.uint32)
    for k in range(pk.w):
        field = (field << np.uint32(8)) | msg[:, pk.n + k].astype(np.uint32)
    return payload, (got == field).astype(np.uint8), got, metric
