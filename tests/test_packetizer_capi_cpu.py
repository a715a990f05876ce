"""Packetizer through the C ABI without a GPU: encode_host and decode_host (the library's sequential loops) equal
tests/packetizer_ref.py byte for byte with the gap bytes untouched, the helper functions equal the restatement's, the
header's constants equal the package's, and every argument check answers YAGI_ERR_CONFIG before any device is asked for."""
import re

import numpy as np
import pytest

import convcode_ref as cc
import packetizer_ref as pr
from conftest import ROOT, has_gpu

import yagi_amd as ya

CODES = {"k3": (3, (7, 5), None), "k5": (5, (0x17, 0x19), None), "v27": cc.V27, "v27p34": cc.V27P34,
         "k9r4": (9, (0x1ed, 0x19b, 0x127, 0x1af), None)}
V27G = (0x6d, 0x4f)


def soft_bank(rng, pk, payload):
    """rows of every kind: the soft kinds of convcode_ref (no codewords) and codewords with none, few and many flips"""
    rows = [cc.soft_bytes(rng, kind, 1, pk.N)[0] for kind in cc.SOFT_KINDS]
    clean = pr.encode(pk, payload) * np.uint8(255)
    for f, flips in enumerate((0, 2, pk.N // 3)):
        row = clean[f % len(clean)].copy()
        at = rng.choice(pk.N, flips, replace=False)
        row[at] = 255 - row[at]
        rows.append(row)
    return np.stack(rows)


@pytest.mark.parametrize("terminated", [True, False])
@pytest.mark.parametrize("name", sorted(CODES))
def test_host_forms_equal_the_restatement(name, terminated):
    code = cc.Code(*CODES[name], terminated)
    rng = np.random.default_rng(code.K + 2 * terminated)
    both = set()
    for n, scheme, scramble in ((1, pr.CRC_NONE, True), (2, pr.CRC_8, False), (3, pr.CRC_16, True), (9, pr.CRC_24, True),
                                (9, pr.CRC_32, True), (33, pr.CRC_32, False)):
        N = pr.Packet(code, n, scheme).N
        for C in (1, 2, 7, int(np.sqrt(N)), N - 1, N, N + 1):
            pk = pr.Packet(code, n, scheme, C, scramble)
            payload = rng.integers(0, 256, (3, n + 2)).astype(np.uint8)             # two junk columns behind the payload
            for bps in (1, 2, 3, 8):
                want = pr.encode(pk, payload, bps)
                out = np.full((3, want.shape[1] + 3), 0xEE, np.uint8)
                got = ya.Packetizer.encode_host(*pk.args()[:4], payload, bps, *pk.args()[4:], out=out)
                assert np.array_equal(got[:, :want.shape[1]], want) and (got[:, want.shape[1]:] == 0xEE).all(), (n, C, bps)
            soft = np.full((9, N + 1), 77, np.uint8)
            soft[:, :N] = soft_bank(rng, pk, payload)
            wpay, wvalid, wcrc, wmetric = pr.decode(pk, soft)
            both |= set(wvalid.tolist()) if scheme else set()
            out = np.full((9, n + 2), 0xEE, np.uint8)
            gpay, gvalid, gcrc, gmetric = ya.Packetizer.decode_host(*pk.args()[:4], soft, *pk.args()[4:], out=out)
            assert np.array_equal(gpay[:, :n], wpay) and (gpay[:, n:] == 0xEE).all(), (n, C)
            assert np.array_equal(gvalid, wvalid) and np.array_equal(gcrc, wcrc) and np.array_equal(gmetric, wmetric), (n, C)
            alone = ya.Packetizer.decode_host(*pk.args()[:4], soft, *pk.args()[4:], want_crc=False, metric=False)
            assert np.array_equal(alone[0], wpay) and alone[2] is None and alone[3] is None
    assert both == {0, 1}, "the bank holds frames of both verdicts"


def test_the_helpers_equal_the_restatement():
    rng = np.random.default_rng(5)
    for scheme in pr.SCHEMES:
        assert ya.crc(scheme, b"123456789") == pr.CRC_PARAMS[scheme][5]
        for n in (0, 1, 2, 70, 300):
            data = rng.integers(0, 256, n).astype(np.uint8)
            assert ya.crc(ya.CrcScheme(scheme), data) == pr.crc(scheme, data), (scheme, n)
    for N in (1, 2, 7, 68, 69):
        for C in (1, 2, 3, 7, 8, 68, 69, 70, 79, ya.PACKETIZER_COLUMNS_MAX):
            assert np.array_equal(ya.packetizer_permutation(N, C), pr.perm(N, C)), (N, C)
    assert ya.packetizer_permutation(0, 3).size == 0
    for n in (0, 1, 3, 4, 5, 11, 16, 33, 277):
        x = rng.integers(0, 256, n).astype(np.uint8)
        assert np.array_equal(ya.scramble_data(x), pr.scramble_data(x))
        assert np.array_equal(ya.unscramble_data(ya.scramble_data(x)), x)
        for m in (8 * n, max(0, 8 * n - 3)):
            s = rng.integers(0, 256, m).astype(np.uint8)
            assert np.array_equal(ya.unscramble_data_soft(s), pr.unscramble_data_soft(s)), m


def test_the_header_constants():
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    for name, ours, theirs in (("NONE", ya.CrcScheme.NONE, pr.CRC_NONE), ("8", ya.CrcScheme.CRC_8, pr.CRC_8),
                               ("16", ya.CrcScheme.CRC_16, pr.CRC_16), ("24", ya.CrcScheme.CRC_24, pr.CRC_24),
                               ("32", ya.CrcScheme.CRC_32, pr.CRC_32)):
        assert int(re.search(rf"#define YAGI_CRC_{name} (\d+)", hdr).group(1)) == int(ours) == theirs
    assert int(re.search(r"#define YAGI_PACKETIZER_COLUMNS_MAX (\d+)", hdr).group(1)) == ya.PACKETIZER_COLUMNS_MAX == pr.COLUMNS_MAX


def test_the_plan_is_convcodes_arrangement():
    for K, n, scheme, F in ((3, 1, 0, 1), (5, 33, 4, 1000), (7, 125, 4, 1 << 16), (7, 2040, 4, 4096), (9, 500, 2, 64)):
        w = pr.crc_len(scheme)
        p, c = ya.packetizer_plan(K, n, scheme, F), ya.convcode_plan(K, 8 * (n + w), F)
        assert {k: p[k] for k in p if k != "lds_bytes"} == {k: c[k] for k in c if k != "lds_bytes"}
        # no staged raw words (4 bytes a step and 8 per frame, per wave); the CRC's table of 256 pairs
        raw = p["waves"] * (256 * 4 + 8 * p["frames_per_wave"])
        assert p["lds_bytes"] == c["lds_bytes"] - raw + (2048 if w else 0)


def bad_calls():
    pay, soft = np.zeros((2, 4), np.uint8), np.zeros((2, 2 * (8 * 8 + 6)), np.uint8)
    tx = np.zeros((2, soft.shape[1]), np.uint8)
    enc = lambda n=4, crc=4, K=7, g=V27G, bps=1, **kw: ya.Packetizer.encode_host(n, crc, K, g, pay, bps, out=tx, **kw)
    dec = lambda n=4, crc=4, K=7, g=V27G, **kw: ya.Packetizer.decode_host(n, crc, K, g, soft, **kw)
    nmax = ya.ConvCode.nmax_host(7)
    return enc, dec, [
        ("n = 0", dict(n=0)),
        ("a message beyond nmax", dict(n=nmax // 8 - 3)),                 # 8 (n + 4) bits are more than nmax
        ("C = 0", dict(columns=0)),
        ("C beyond the limit", dict(columns=ya.PACKETIZER_COLUMNS_MAX + 1)),
        ("a bad scheme", dict(crc=5)),
        ("a negative scheme", dict(crc=-1)),
        ("a bad code", dict(K=10)),
    ]


def test_bad_arguments_are_config_errors_without_a_device():
    enc, dec, cases = bad_calls()
    enc()                                                                  # the good calls
    dec()
    assert 8 * (ya.ConvCode.nmax_host(7) // 8 - 3 + 4) > ya.ConvCode.nmax_host(7)
    for what, kw in cases:
        with pytest.raises(ya.ConfigError):
            enc(**kw)
        with pytest.raises(ya.ConfigError):
            dec(**kw)
        with pytest.raises(ya.ConfigError):                                # create decides before it asks for a device
            ya.Packetizer(kw.get("n", 4), kw.get("crc", 4), kw.get("K", 7), V27G, columns=kw.get("columns", 1))
    for bps in (0, 9):
        with pytest.raises(ya.ConfigError):
            enc(bps=bps)
    for kw in (dict(payload_pitch=3), dict(tx_pitch=139)):                 # a pitch below the row
        with pytest.raises(ya.ConfigError):
            enc(**kw)
    for kw in (dict(soft_pitch=139), dict(payload_pitch=3)):
        with pytest.raises(ya.ConfigError):
            dec(**kw)
    with pytest.raises(ya.ConfigError):
        ya.packetizer_plan(7, 0, 4, 1)
    with pytest.raises(ya.ConfigError):
        ya.packetizer_plan(7, 4, 4, ya.CONVCODE_FRAMES_MAX + 1)
    with pytest.raises(ya.ConfigError):
        ya.crc(5, b"1")
    with pytest.raises(ya.ConfigError):
        ya.packetizer_permutation(7, 0)


@pytest.mark.skipif(has_gpu(), reason="the answer without a device")
def test_a_valid_create_without_a_device_is_a_device_error():
    with pytest.raises(ya.DeviceError):
        ya.Packetizer.v27(125)
