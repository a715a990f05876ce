"""ConvCode through the C ABI without a GPU: encode_host and decode_host (the library's sequential loops) equal
tests/convcode_ref.py byte for byte, message, pad bits and metric included; ncoded's closed form equals a count by loop; and
every argument check answers YAGI_ERR_CONFIG before any device is asked for."""
import re

import numpy as np
import pytest

import convcode_ref as cc
from conftest import ROOT, has_gpu

import yagi_amd as ya

GENS = {(3, 2): (7, 5), (3, 3): (7, 5, 6), (3, 4): (7, 5, 6, 3),
        (5, 2): (0x17, 0x19), (5, 3): (0x1f, 0x1b, 0x15), (5, 4): (0x17, 0x19, 0x1d, 0x1f),
        (7, 2): (0x6d, 0x4f), (7, 3): (0x6d, 0x4f, 0x57), (7, 4): (0x6d, 0x4f, 0x57, 0x73),
        (9, 2): (0x1af, 0x11d), (9, 3): (0x1ed, 0x19b, 0x127), (9, 4): (0x1ed, 0x19b, 0x127, 0x1af)}
CODES = [(K, g, None) for (K, R), g in sorted(GENS.items())] + [cc.V27P23, cc.V27P34]
NS = (1, 7, 8, 9, 64, 65)


def code_id(spec):
    K, g, P = spec
    return f"K{K}R{len(g)}" + ("" if P is None else f"p{len(P[0])}")


@pytest.mark.parametrize("terminated", [True, False])
@pytest.mark.parametrize("spec", CODES, ids=code_id)
def test_host_forms_equal_the_restatement(spec, terminated):
    code = cc.Code(*spec, terminated)
    rng = np.random.default_rng(code.K * 10 + code.R)
    for n in NS:
        nb, nc = (n + 7) // 8, code.ncoded(n)
        msg = cc.messages(rng, 3, n, pitch=nb + 2)
        msg[:, nb - 1] |= rng.integers(0, 256, 3).astype(np.uint8) & ((1 << (8 * nb - n)) - 1)     # junk in the pad bits too
        want = cc.encode(code, msg, n)
        out = np.full((3, nc + 3), 9, np.uint8)
        got = ya.ConvCode.encode_host(*code.args()[:2], msg, n, code.puncture, terminated, out=out)
        assert np.array_equal(got[:, :nc], want) and (got[:, nc:] == 9).all(), n
        for kind in cc.SOFT_KINDS:
            soft = np.full((3, nc + 1), 77, np.uint8)
            soft[:, :nc] = cc.soft_bytes(rng, kind, 3, nc)
            wmsg, wmetric = cc.decode(code, soft[:, :nc], n)
            out = np.full((3, nb + 2), 0xEE, np.uint8)
            gmsg, gmetric = ya.ConvCode.decode_host(*code.args()[:2], soft, n, code.puncture, terminated, out=out)
            assert np.array_equal(gmsg[:, :nb], wmsg) and (gmsg[:, nb:] == 0xEE).all(), (n, kind)
            assert np.array_equal(gmetric, wmetric), (n, kind)
            alone = ya.ConvCode.decode_host(*code.args()[:2], soft, n, code.puncture, terminated, metric=False)
            assert np.array_equal(alone, wmsg)


@pytest.mark.parametrize("spec", CODES + [(4, (0xf, 0xb), ((1, 0, 1, 1, 0), (0, 1, 1, 0, 1)))], ids=code_id)
def test_ncoded_is_the_count_by_loop(spec):
    for terminated in (True, False):
        code = cc.Code(*spec, terminated)
        for n in list(range(1, 40)) + [64, 65, 1000]:
            assert ya.ConvCode.ncoded_host(code.K, code.R, n, code.puncture, terminated) == code.ncoded(n), n
        assert ya.ConvCode.nmax_host(code.K, code.R, code.puncture, terminated) == code.nmax()


def test_the_limits_and_the_header_constants():
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    for name, ours, theirs in (("DECISION_BYTES", ya.CONVCODE_DECISION_BYTES, cc.DECISION_BYTES),
                               ("STEPS_MAX", ya.CONVCODE_STEPS_MAX, cc.STEPS_MAX),
                               ("PERIOD_MAX", ya.CONVCODE_PERIOD_MAX, cc.PERIOD_MAX)):
        assert int(re.search(rf"#define YAGI_CONVCODE_{name} (\d+)", hdr).group(1)) == ours == theirs
    assert int(re.search(r"#define YAGI_CONVCODE_FRAMES_MAX (\d+)", hdr).group(1)) == ya.CONVCODE_FRAMES_MAX
    assert ya.ConvCode.nmax_host(7) + 6 == 16384 and ya.ConvCode.nmax_host(9) + 8 == 4096
    assert ya.ConvCode.nmax_host(7, terminated=False) == 16384


def test_the_plan():
    for K in range(3, 10):
        S = 1 << (K - 1)
        fmin, fmax = max(1, 8 // S), max(1, 64 // S)
        for n, F in ((1, 1), (100, 1), (100, 3), (100, 1000), (1000, 1 << 16), (ya.ConvCode.nmax_host(K), 4096)):
            p = ya.convcode_plan(K, n, F)
            fpw = p["frames_per_wave"]
            assert p["states_per_lane"] == max(1, S // 64) and fmin <= fpw <= fmax and fpw & (fpw - 1) == 0
            assert p["chunk_steps"] * fpw == 256 and p["waves"] in (1, 2, 4)
            assert p["frames_per_wg"] == fpw * p["waves"] and p["lds_bytes"] <= 160 * 1024
            assert p["waves"] == 1 or (p["lds_bytes"] <= 64 * 1024 and p["frames_per_wg"] // 2 < F)
        # as many frames per wave as the lanes hold, unless that leaves the chip short of waves
        assert ya.convcode_plan(K, 1000, 1 << 16)["frames_per_wave"] == fmax
        assert ya.convcode_plan(K, 100, 1)["frames_per_wave"] == fmin
    assert ya.convcode_plan(5, 8192, 1 << 16)["frames_per_wave"] == 1      # long frames: more waves, not wider ones


V27G = (0x6d, 0x4f)
BAD_CODES = [
    (2, (3, 1), None),                                     # K = 2
    (10, (0x3ff, 0x201), None),                            # K = 10
    (7, (0x6d,), None),                                    # R = 1
    (7, (0x6d, 0x4f, 0x57, 0x73, 0x5b), None),             # R = 5
    (7, (0x6d, 0), None),                                  # g = 0
    (7, (0x6d, 0x80), None),                               # g >= 2^K
    (7, V27G, ((1, 0, 1), (1, 0, 1))),                     # a column that keeps nothing
    (7, V27G, ((1,) * 33, (1,) * 33)),                     # p = 33
]


@pytest.mark.parametrize("K,g,P", BAD_CODES)
def test_bad_codes_are_config_errors_without_a_device(K, g, P):
    with pytest.raises(ya.ConfigError):
        ya.ConvCode(K, g, P)
    with pytest.raises(ya.ConfigError):
        ya.ConvCode.encode_host(K, g, np.zeros((1, 1), np.uint8), 8, P, out=np.zeros((1, 64), np.uint8))
    with pytest.raises(ya.ConfigError):
        ya.ConvCode.decode_host(K, g, np.zeros((1, 64), np.uint8), 8, P)


def test_bad_blocks_are_config_errors():
    msg, coded = np.zeros((2, 2), np.uint8), np.zeros((2, 32), np.uint8)
    ya.ConvCode.encode_host(7, V27G, msg, 10, out=coded)                  # the good call: 2 (10 + 6) = 32 bytes a row
    ya.ConvCode.decode_host(7, V27G, coded, 10)
    for n in (0, ya.ConvCode.nmax_host(7) + 1):                            # n = 0; T over the limit
        with pytest.raises(ya.ConfigError):
            ya.ConvCode.encode_host(7, V27G, msg, n, out=coded)
        with pytest.raises(ya.ConfigError):
            ya.ConvCode.decode_host(7, V27G, coded, n)
        with pytest.raises(ya.ConfigError):
            ya.convcode_plan(7, n, 1)
    with pytest.raises(ya.ConfigError, match="YAGI_CONVCODE_DECISION_BYTES"):
        ya.ConvCode.ncoded_host(9, 2, 4089)
    with pytest.raises(ya.ConfigError):                                    # pitches shorter than a row
        ya.ConvCode.encode_host(7, V27G, msg, 10, out=coded, msg_pitch=1)
    with pytest.raises(ya.ConfigError):
        ya.ConvCode.encode_host(7, V27G, msg, 10, out=coded, coded_pitch=31)
    with pytest.raises(ya.ConfigError):
        ya.ConvCode.decode_host(7, V27G, coded, 10, soft_pitch=31)
    with pytest.raises(ya.ConfigError):
        ya.ConvCode.decode_host(7, V27G, coded, 10, msg_pitch=1)
    with pytest.raises(ya.ConfigError):                                    # operands that overlap
        ya.ConvCode.decode_host(7, V27G, coded, 10, out=coded)
    with pytest.raises(ya.ConfigError):
        ya.convcode_plan(7, 10, ya.CONVCODE_FRAMES_MAX + 1)


@pytest.mark.skipif(has_gpu(), reason="the answer without a device")
def test_a_valid_create_without_a_device_is_a_device_error():
    with pytest.raises(ya.DeviceError):
        ya.ConvCode.v27()
