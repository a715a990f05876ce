"""ConvCode on the device: every byte of encode_block and decode_block (message, pad bits, metric) equals
tests/convcode_ref.py, at the smallest shapes that can break each mechanism of convcode_kernels.hip.  The soft inputs are
random and tie-heavy bytes, not codewords, so that every survivor decision matters.  Shapes that depend on the launch
arrangement (frames per wave and per workgroup, the soft-staging chunk) are read from get_shape, never written down."""
import numpy as np
import pytest

import convcode_ref as cc

pytestmark = pytest.mark.gpu

GENS = {(3, 2): (7, 5), (4, 2): (0xf, 0xb), (5, 2): (0x17, 0x19), (6, 2): (0x35, 0x2b), (7, 2): (0x6d, 0x4f),
        (8, 2): (0xf7, 0xb9), (9, 2): (0x1af, 0x11d), (7, 3): (0x6d, 0x4f, 0x57), (7, 4): (0x6d, 0x4f, 0x57, 0x73),
        (9, 3): (0x1ed, 0x19b, 0x127), (9, 4): (0x1ed, 0x19b, 0x127, 0x1af)}
NS = (1, 7, 8, 9, 63, 64, 65, 1000)


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def make(ya, code):
    return ya.ConvCode(*code.args())


def soft_rows(rng, F, nc, shift):
    """F rows of soft bytes, the kinds of convcode_ref.SOFT_KINDS in turn"""
    return np.concatenate([cc.soft_bytes(rng, cc.SOFT_KINDS[(f + shift) % len(cc.SOFT_KINDS)], 1, nc) for f in range(F)])


def check_decode(q, soft, n, want_msg, want_metric, F, pad=3):
    """the first F frames through decode_block, with pitches wider than the rows on both sides"""
    nb, nc = (n + 7) // 8, soft.shape[1]
    wide = np.full((F, nc + pad), 0x5A, np.uint8)
    wide[:, :nc] = soft[:F]
    out = np.full((F, nb + pad), 0xEE, np.uint8)
    msg, metric = q.decode_block(wide, n, out=out)
    assert np.array_equal(msg[:, :nb], want_msg[:F]), (n, F)
    assert (msg[:, nb:] == 0xEE).all(), "a gap byte of msg was written"
    assert np.array_equal(metric, want_metric[:F]), (n, F)


def check_encode(q, msg, n, want, F, pad=2):
    nc = want.shape[1]
    out = np.full((F, nc + pad), 0xEE, np.uint8)
    got = q.encode_block(msg[:F], n, out=out)
    assert np.array_equal(got[:, :nc], want[:F]), (n, F)
    assert (got[:, nc:] == 0xEE).all(), "a gap byte of coded was written"


def full_shape(q, n):
    """the arrangement of a bank large enough to fill the chip: as many frames per wave as the planner ever uses at n"""
    return q.get_shape(n, 1 << 16)


def frame_counts(q, code, n):
    """F around every seam of the plan: the frames of a wave and of a workgroup, each - 1, exact and + 1"""
    full = full_shape(q, n)
    fpw, G = full["frames_per_wave"], full["frames_per_wg"]
    assert fpw == max(1, 64 // code.S) and full["states_per_lane"] == max(1, code.S // 64)
    base = {1, fpw - 1, fpw, fpw + 1} if code.S < 64 else {1, 2, 5}
    return sorted(F for F in base | {G - 1, G, G + 1} if F >= 1)


@pytest.mark.parametrize("terminated", [True, False])
@pytest.mark.parametrize("K,R", sorted(GENS))
def test_every_code_at_every_seam(ya, K, R, terminated):
    code = cc.Code(K, GENS[(K, R)], None, terminated)
    q = make(ya, code)
    assert (q.get_K(), q.get_R(), q.rate(), q.nmax()) == (K, R, (R, 1), code.nmax())
    rng = np.random.default_rng(K * 16 + R * 2 + terminated)
    tail = code.steps(0)
    chunks = {full_shape(q, 64)["chunk_steps"], q.get_shape(64, 1)["chunk_steps"]}      # a full bank's and one frame's
    seams = [c - tail + d for c in chunks for d in (-1, 0, 1)] + [2 * max(chunks) - tail + 1]      # T at the chunk -1, 0, +1
    for n in sorted(set(NS) | {n for n in seams if n >= 1}):
        assert q.ncoded(n) == code.ncoded(n)
        counts = frame_counts(q, code, n)
        soft = soft_rows(rng, counts[-1], code.ncoded(n), n)
        want_msg, want_metric = cc.decode(code, soft, n)
        msg = cc.messages(rng, counts[-1], n, pitch=(n + 7) // 8 + 1)
        want_coded = cc.encode(code, msg, n)
        full = full_shape(q, n)
        for F in counts:
            check_decode(q, soft, n, want_msg, want_metric, F)                          # the planner's shape for F frames
            q.set_shape(full["frames_per_wave"], full["waves"])                        # the full bank's shape on F frames
            check_decode(q, soft, n, want_msg, want_metric, F)
            q.set_shape(0, 0)
            check_encode(q, msg, n, want_coded, F)


@pytest.mark.parametrize("terminated", [True, False])
@pytest.mark.parametrize("spec", [cc.V27P23, cc.V27P34], ids=["p23", "p34"])
def test_punctured_codes(ya, spec, terminated):
    code = cc.Code(*spec, terminated)
    q = make(ya, code)
    assert q.rate() == (int(code.P.sum()), code.p)
    rng = np.random.default_rng(code.p)
    chunk = q.get_shape(64, 5)["chunk_steps"]
    for n in (1, code.p, code.p + 1, chunk - code.steps(0), chunk + 1, 1000):
        assert q.ncoded(n) == code.ncoded(n)
        soft = soft_rows(rng, 5, code.ncoded(n), n)
        want_msg, want_metric = cc.decode(code, soft, n)
        msg = cc.messages(rng, 5, n)
        want_coded = cc.encode(code, msg, n)
        for F in (1, 2, 5):
            check_decode(q, soft, n, want_msg, want_metric, F, pad=F)      # rows at every alignment
            check_encode(q, msg, n, want_coded, F)
        got, metric = q.decode_block(want_coded * 255, n)                  # the noise-free round trip
        assert np.array_equal(got, msg[:, :(n + 7) // 8]) and not metric.any()


@pytest.mark.parametrize("K", [3, 5, 7, 9])
def test_every_admissible_shape_gives_the_same_bytes(ya, K):
    code = cc.Code(K, GENS[(K, 2)])
    q = make(ya, code)
    rng = np.random.default_rng(K)
    fmax = max(1, 64 // code.S)
    n, F = 300, 4 * fmax + 1
    soft = soft_rows(rng, F, code.ncoded(n), 0)
    want_msg, want_metric = cc.decode(code, soft, n)
    planned = q.decode_block(soft, n)
    assert np.array_equal(planned[0], want_msg) and np.array_equal(planned[1], want_metric)
    shapes = 0
    for fpw in (1, 2, 4, 8, 16, 32):
        for waves in (1, 2, 3, 4, 8):
            ok = max(1, 8 // code.S) <= fpw <= fmax and waves in (1, 2, 4)
            if not ok:
                with pytest.raises(ya.ConfigError):
                    q.set_shape(fpw, waves)
                continue
            q.set_shape(fpw, waves)
            s = q.get_shape(n, F)
            assert (s["frames_per_wave"], s["waves"], s["frames_per_wg"]) == (fpw, waves, fpw * waves)
            assert s["chunk_steps"] * fpw == 256
            got = q.decode_block(soft, n)
            assert np.array_equal(got[0], planned[0]) and np.array_equal(got[1], planned[1]), (fpw, waves)
            shapes += 1
    assert shapes == 3 * len([f for f in (1, 2, 4, 8, 16) if max(1, 8 // code.S) <= f <= fmax])
    q.set_shape(0, 0)
    assert q.get_shape(n, F) == ya.convcode_plan(K, n, F)


@pytest.mark.parametrize("spec", [cc.V27, cc.V29], ids=["v27", "v29"])
def test_the_longest_frame(ya, spec):
    code = cc.Code(*spec)
    q = make(ya, code)
    n = q.nmax()
    assert code.steps(n) == {7: 16384, 9: 4096}[code.K]
    rng = np.random.default_rng(n)
    soft = cc.soft_bytes(rng, "random", 1, code.ncoded(n))
    want_msg, want_metric = cc.decode(code, soft, n)
    check_decode(q, soft, n, want_msg, want_metric, 1)
    msg = cc.messages(rng, 1, n)
    check_encode(q, msg, n, cc.encode(code, msg, n), 1)
    with pytest.raises(ya.ConfigError):
        q.decode_block(np.zeros((1, code.ncoded(n) + code.R), np.uint8), n + 1)


def test_without_the_metric_and_on_a_clone(ya):
    code = cc.Code(*cc.V27)
    q = ya.ConvCode.v27()
    rng = np.random.default_rng(3)
    n, F = 100, 7
    soft = soft_rows(rng, F, code.ncoded(n), 1)
    want_msg, want_metric = cc.decode(code, soft, n)
    assert np.array_equal(q.decode_block(soft, n, metric=False), want_msg)
    c = q.clone()
    del q
    got = c.decode_block(soft, n)
    assert np.array_equal(got[0], want_msg) and np.array_equal(got[1], want_metric)
    assert np.array_equal(c.decode_block(soft[0], n)[0], want_msg[:1])             # one frame as a 1-D row


def test_the_named_codes(ya):
    for name, spec in (("v27", cc.V27), ("v29", cc.V29), ("v39", cc.V39), ("v27p23", cc.V27P23), ("v27p34", cc.V27P34)):
        code = cc.Code(*spec)
        q = getattr(ya.ConvCode, name)()
        msg = cc.messages(np.random.default_rng(1), 2, 50)
        assert (q.get_K(), q.get_R(), q.terminated) == (code.K, code.R, True)
        assert np.array_equal(q.encode_block(msg, 50), cc.encode(code, msg, 50)), name


def test_config_errors_of_a_built_object(ya):
    q = ya.ConvCode.v27()
    soft = np.zeros((2, 32), np.uint8)
    with pytest.raises(ya.ConfigError):
        q.decode_block(soft, 0)
    with pytest.raises(ya.ConfigError):
        q.ncoded(q.nmax() + 1)
    with pytest.raises(ya.ConfigError):
        q.decode_block(soft, 11)                                                    # rows shorter than ncoded(11) = 34
    with pytest.raises(ya.ConfigError):
        q.encode_block(np.zeros((2, 1), np.uint8), 10)
    assert q.decode_block(np.zeros((0, 32), np.uint8), 10)[0].shape == (0, 2)      # no frames: nothing to do


def test_end_to_end_through_modem_and_channel(ya):
    """encode -> QPSK -> Channel (one tap) -> soft demodulation -> decode, one link per frame: with the noise off the
    message comes back, so Modem's soft bytes are ConvCode's (255 a confident 1, most significant bit first); with noise
    the decoder equals the restatement on the same soft bytes, whatever the error rate"""
    code = cc.Code(*cc.V27)
    q = ya.ConvCode.v27()
    F, n = 8, 200
    rng = np.random.default_rng(8)
    msg = cc.messages(rng, F, n)
    coded = q.encode_block(msg, n)
    nc = coded.shape[1]
    sym = (coded[:, 0::2] << 1) | coded[:, 1::2]                                    # bit pairs, first bit the upper one
    modem = ya.Modem(ya.ModulationScheme.Qpsk)
    tx = modem.modulate_block(sym.reshape(-1)).reshape(F, nc // 2)
    for snr_db in (None, 3.0):
        ch = ya.Channel(F, 1)
        ch.set_seed(1234)
        if snr_db is not None:
            ch.set_awgn_all(np.full(F, -snr_db, np.float32), np.full(F, snr_db, np.float32))      # unit gain
        rx = ch.execute(np.ascontiguousarray(tx.T)).T
        _, soft = modem.demodulate_soft_block(np.ascontiguousarray(rx).reshape(-1))
        soft = soft.reshape(F, nc)
        got, metric = q.decode_block(soft, n)
        want, want_metric = cc.decode(code, soft, n)
        assert np.array_equal(got, want) and np.array_equal(metric, want_metric)
        if snr_db is None:
            assert np.array_equal(got, msg) and not metric.any()
            assert np.array_equal(soft, coded * 255)
        else:
            assert ((soft > 0) & (soft < 255)).any(), "the noise reached the soft bytes"
