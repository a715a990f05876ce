"""tests/convcode_ref.py pins ConvCode's definition (include/yagi_hip.h): its two forms agree byte for byte, the bit and
generator conventions give the known free distances of the public codes, and the decoder corrects what those distances
promise.  No library code runs here."""
import numpy as np
import pytest

import convcode_ref as cc


def all_messages(n, first_one):
    """every nonzero n-bit message (with the first bit set where asked), packed"""
    v = np.arange(1 << (n - 1), 1 << n) if first_one else np.arange(1, 1 << n)
    bits = ((v[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
    return cc.pack(bits)


def min_weight(code, lengths, first_one):
    return min(int(cc.encode(code, all_messages(n, first_one), n).sum(axis=1).min()) for n in lengths)


@pytest.mark.parametrize("K,g,P", [cc.V27, cc.V27P23, cc.V27P34, (3, (7, 5), None), (5, (0x17, 0x19, 0x1d, 0x1f), None),
                                   (9, (0x1ed, 0x19b, 0x127), None), (4, (0xf, 0xb), ((1, 0, 1, 1, 0), (0, 1, 1, 0, 1)))])
@pytest.mark.parametrize("terminated", [True, False])
def test_the_two_forms_agree(K, g, P, terminated):
    code = cc.Code(K, g, P, terminated)
    rng = np.random.default_rng(K * 100 + len(g) + terminated)
    for n in (1, 7, 8, 9, 33):
        nc = code.ncoded(n)
        for kind in cc.SOFT_KINDS:
            soft = cc.soft_bytes(rng, kind, 3, nc)
            msg, metric = cc.decode(code, soft, n)
            assert msg.shape == (3, (n + 7) // 8) and metric.dtype == np.uint32
            for f in range(3):
                m1, k1 = cc.decode_loop(code, soft[f], n)
                assert np.array_equal(m1, msg[f]) and k1 == metric[f], (n, kind, f)


@pytest.mark.parametrize("spec,dfree", [(cc.V27, 10), (cc.V29, 12), (cc.V39, 18), ((3, (7, 5), None), 5)])
def test_free_distance_pins_the_convention(spec, dfree):
    code = cc.Code(*spec)
    assert min_weight(code, range(1, code.K + 7), True) == dfree


@pytest.mark.parametrize("spec,dfree", [(cc.V27P23, 6), (cc.V27P34, 5)])
def test_free_distance_of_the_punctured_codes(spec, dfree):
    assert min_weight(cc.Code(*spec), range(1, 15), False) == dfree


def test_v27_corrects_four_flipped_bits():
    code = cc.Code(*cc.V27)
    rng = np.random.default_rng(27)
    trials = 0
    for n in range(1, 80):
        F = 4
        msg = cc.messages(rng, F, n)
        coded = cc.encode(code, msg, n)
        flips = rng.integers(0, 5, F)
        soft = coded * 255
        for f in range(F):
            soft[f, rng.choice(coded.shape[1], flips[f], replace=False)] ^= 255
        got, metric = cc.decode(code, soft, n)
        assert np.array_equal(got, msg), n
        assert np.array_equal(metric, 255 * flips), (n, metric, flips)
        trials += F
    assert trials >= 300


@pytest.mark.parametrize("spec", [cc.V27P23, cc.V27P34])
def test_noise_free_punctured_round_trip(spec):
    code = cc.Code(*spec)
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 4, 17, 64, 65, 100, 130, 200):
        msg = cc.messages(rng, 10, n)
        coded = cc.encode(code, msg, n)
        assert coded.shape[1] == code.ncoded(n)
        got, metric = cc.decode(code, coded * 255, n)
        assert np.array_equal(got, msg) and not metric.any(), n


def test_pad_bits_and_junk_columns():
    code = cc.Code(*cc.V27)
    rng = np.random.default_rng(1)
    wide = cc.messages(rng, 3, 13, pitch=5)
    assert np.array_equal(cc.encode(code, wide, 13), cc.encode(code, wide[:, :2] & np.array([0xff, 0xf8], np.uint8), 13))
    got, _ = cc.decode(code, cc.encode(code, wide, 13) * 255, 13)
    assert np.array_equal(got, wide[:, :2] & np.array([0xff, 0xf8], np.uint8))
