"""The Packetizer's restatement (tests/packetizer_ref.py) against what is known from elsewhere: the published CRC check
values, zlib's and binascii's CRCs, the interleaver's closed forms against the matrix it abbreviates, the reference's
scramble tests (src/random/scramble.rs :55-202) restated, the noise-free round trip, and the one thing the interleaver is
for: a burst that breaks a frame at C = 1 and does not at a larger C."""
import binascii
import zlib

import numpy as np
import pytest

import convcode_ref as cc
import packetizer_ref as pr

import yagi_amd as ya                                     # the feature under test: the restatement alone proves nothing

SCRAMBLE_NS = (16, 64, 256, 11, 33, 277)


def test_the_package_has_the_object():
    assert ya.Packetizer.__name__ == "Packetizer" and [int(s) for s in ya.CrcScheme] == list(pr.SCHEMES)


def test_crc_check_values():
    for scheme in pr.SCHEMES[1:]:
        assert pr.crc(scheme, b"123456789") == pr.CRC_PARAMS[scheme][5], scheme
    assert pr.crc(pr.CRC_NONE, b"123456789") == 0 and pr.crc_len(pr.CRC_NONE) == 0
    assert [pr.crc_len(s) for s in pr.SCHEMES] == [0, 1, 2, 3, 4]


def test_crc_32_and_16_equal_the_standard_library():
    rng = np.random.default_rng(32)
    for n in range(71):
        data = bytes(rng.integers(0, 256, n).astype(np.uint8))
        assert pr.crc(pr.CRC_32, data) == zlib.crc32(data), n
        assert pr.crc(pr.CRC_16, data) == binascii.crc_hqx(data, 0xFFFF), n


def test_permutation_closed_forms_equal_the_matrix():
    assert list(pr.perm_inverse(7, 3)) == [0, 3, 6, 1, 4, 2, 5]
    for N in range(1, 70):
        for C in range(1, 80):
            pi, inv, built = pr.perm(N, C), pr.perm_inverse(N, C), pr.perm_matrix(N, C)
            assert np.array_equal(inv, built), (N, C)
            assert np.array_equal(pi[inv], np.arange(N)) and np.array_equal(inv[pi], np.arange(N)), (N, C)
            if C == 1 or C >= N:
                assert np.array_equal(pi, np.arange(N)), (N, C)


@pytest.mark.parametrize("n", SCRAMBLE_NS)
def test_scramble_round_trip_and_entropy(n):
    """scramble_test: zeros scrambled and unscrambled come back, and the scrambled zeros have an entropy above 0.8"""
    x = np.zeros(n, np.uint8)
    y = pr.scramble_data(x)
    assert np.array_equal(pr.unscramble_data(y), x)
    assert pr.entropy(y) > 0.8
    assert np.array_equal(np.unpackbits(y), pr.scramble_mask(8 * n))       # the mask bit by bit is the packed mask


@pytest.mark.parametrize("n", SCRAMBLE_NS)
def test_scramble_soft_round_trip(n):
    """scramble_soft_test: random bytes, scrambled, as soft bits 0 / 255, unscrambled softly, sliced at 127"""
    org = np.random.default_rng(n).integers(0, 256, n).astype(np.uint8)
    soft = np.unpackbits(pr.scramble_data(org)) * np.uint8(255)
    back = pr.unscramble_data_soft(soft)
    assert np.array_equal(np.packbits(back > 127), org)
    tail = pr.unscramble_data_soft(soft[:8 * n - 3])                      # chunks_exact: the last five bytes stay
    assert np.array_equal(tail[-5:], soft[8 * n - 8:8 * n - 3]) and np.array_equal(tail[:-5], back[:8 * n - 8])


@pytest.mark.parametrize("scheme", pr.SCHEMES)
@pytest.mark.parametrize("spec", [cc.V27, cc.V27P34, (3, (7, 5), None)], ids=["v27", "v27p34", "k3"])
def test_noise_free_round_trip(spec, scheme):
    rng = np.random.default_rng(scheme)
    for terminated in (True, False):
        code = cc.Code(*spec, terminated)
        n = 9
        N = pr.Packet(code, n, scheme).N
        payload = rng.integers(0, 256, (3, n)).astype(np.uint8)
        for C in (1, 5, N):
            for scramble in (True, False):
                pk = pr.Packet(code, n, scheme, C, scramble)
                tx = pr.encode(pk, payload)
                assert tx.shape == (3, N) and tx.max() <= 1
                got, valid, crc, metric = pr.decode(pk, tx * np.uint8(255))
                assert np.array_equal(got, payload) and valid.all() and not metric.any(), (C, scramble)
                assert list(crc) == [pr.crc(scheme, row) for row in payload]
                for bps in (2, 3, 8):                                     # the packed planes hold the same bits
                    sym = pr.encode(pk, payload, bps)
                    bits = np.unpackbits(sym[:, :, None], axis=2)[:, :, 8 - bps:].reshape(3, -1)
                    assert np.array_equal(bits[:, :N], tx) and not bits[:, N:].any(), bps


def test_a_burst_breaks_the_frame_without_the_interleaver_only():
    """v27 at 125 payload bytes, CRC-32: B consecutive transmit soft bytes turned over.  A run of 40 inverted coded bits is
    far beyond what the code's free distance of 10 corrects within a few constraint lengths, so at C = 1 the frame is lost;
    at C = floor(sqrt(N)) = 45 the run falls on bits 45 apart in coder order, 40 isolated errors over 2076 bits"""
    code = cc.Code(*cc.V27)
    n, B = 125, 40
    rng = np.random.default_rng(125)
    payload = rng.integers(0, 256, (4, n)).astype(np.uint8)
    N = pr.Packet(code, n).N
    C = int(np.sqrt(N))
    assert (N, C) == (2 * (8 * 129 + 6), 45)
    verdict = {}
    for cols in (1, C):
        pk = pr.Packet(code, n, pr.CRC_32, cols, True)
        soft = pr.encode(pk, payload) * np.uint8(255)
        soft[:, 700:700 + B] = 255 - soft[:, 700:700 + B]
        got, valid, _, metric = pr.decode(pk, soft)
        verdict[cols] = valid
        assert (np.array_equal(got, payload)) == bool(valid.all())
    assert not verdict[1].any() and verdict[C].all()
