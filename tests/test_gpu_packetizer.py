"""Packetizer on the device: every byte of encode_block (0xEE sentinels intact in the pitch gaps) and every byte and word
of decode_block (payload, valid, crc, metric) equals tests/packetizer_ref.py, at the smallest shapes that can break each
mechanism of packetizer_kernels.hip.  Shapes that depend on the launch arrangement are read from get_shape, never written
down.  The restatement decodes a bank once per (code, n, CRC): its decoder works on coder-order bytes, so the same bank
serves every column count and both scrambler settings through packetizer_ref.sent, and the expected words do not change."""
import numpy as np
import pytest

import convcode_ref as cc
import packetizer_ref as pr

pytestmark = pytest.mark.gpu

CODES = {"k3": (3, (7, 5), None), "k5": (5, (0x17, 0x19), None), "v27": cc.V27, "v27p34": cc.V27P34,
         "k9r4": (9, (0x1ed, 0x19b, 0x127, 0x1af), None)}
NS = (1, 2, 3, 8, 31, 32, 33, 125)
BPS = (1, 2, 3, 8)


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def make(ya, pk):
    return ya.Packetizer(*pk.args())


def columns(N):
    """1, 2, 7, 8, floor(sqrt N), a divisor of N, a non-divisor, N - 1, N, N + 1"""
    divisor = next((c for c in range(3, N) if N % c == 0), N)
    other = next(c for c in range(3, N + 2) if N % c)
    return sorted({1, 2, 7, 8, int(np.sqrt(N)), divisor, other, max(1, N - 1), N, N + 1})


def ordered_bank(rng, pk, payload, F):
    """F rows of coder-order soft bytes: convcode_ref's kinds (no codewords: every decision matters, and crc carries the
    check) and this packet's codewords x 255 with no, a few and many positions turned over"""
    plain = pr.Packet(pk.code, pk.n, pk.scheme, 1, False)
    clean = pr.encode(plain, payload) * np.uint8(255)
    rows = []
    for f in range(F):
        k = f % (len(cc.SOFT_KINDS) + 3)
        if k < len(cc.SOFT_KINDS):
            rows.append(cc.soft_bytes(rng, cc.SOFT_KINDS[k], 1, pk.N)[0])
        else:
            row = clean[f % len(clean)].copy()
            at = rng.choice(pk.N, (0, min(2, pk.N), pk.N // 3)[k - len(cc.SOFT_KINDS)], replace=False)
            row[at] = 255 - row[at]
            rows.append(row)
    return np.stack(rows), plain


def check_decode(q, pk, ordered, want, F, pad=3):
    """the first F frames through decode_block at pk's columns and scrambler, pitches wider than the rows on both sides"""
    wide = np.full((F, pk.N + pad), 0x5A, np.uint8)
    wide[:, :pk.N] = pr.sent(pk, ordered[:F])
    out = np.full((F, pk.n + pad), 0xEE, np.uint8)
    payload, valid, crc, metric = q.decode_block(wide, out=out)
    assert np.array_equal(payload[:, :pk.n], want[0][:F]), (pk.args(), F)
    assert (payload[:, pk.n:] == 0xEE).all(), "a byte behind the payload was written"
    for got, exp, what in zip((valid, crc, metric), want[1:], ("valid", "crc", "metric")):
        assert np.array_equal(got, exp[:F]), (what, pk.args(), F)


def check_encode(q, pk, payload, coded, F, bps, pad=2):
    want = pr.transmit(pk, coded[:F], bps)
    out = np.full((F, want.shape[1] + pad), 0xEE, np.uint8)
    got = q.encode_block(payload[:F], bps, out=out)
    assert np.array_equal(got[:, :want.shape[1]], want), (pk.args(), F, bps)
    assert (got[:, want.shape[1]:] == 0xEE).all(), "a gap byte of the transmit plane was written"


def reference(rng, pk, F):
    """payloads (one junk column behind them), their coded bits, a bank of coder-order soft rows and what it decodes to"""
    payload = rng.integers(0, 256, (F, pk.n + 1)).astype(np.uint8)
    ordered, plain = ordered_bank(rng, pk, payload, F)
    coded = cc.encode(pk.code, pr.message(pk, payload), pk.msg_bits)
    return payload, coded, ordered, pr.decode(plain, ordered)


@pytest.mark.parametrize("terminated", [True, False])
@pytest.mark.parametrize("name", sorted(CODES))
def test_every_payload_length_crc_and_column_count(ya, name, terminated):
    code = cc.Code(*CODES[name], terminated)
    rng = np.random.default_rng(code.K * 4 + terminated)
    verdicts = set()
    for k, n in enumerate(NS):
        scheme = pr.SCHEMES[k % len(pr.SCHEMES)]
        probe = pr.Packet(code, n, scheme)
        F = 9
        payload, coded, ordered, want = reference(rng, probe, F)
        if scheme:
            verdicts |= set(want[1].tolist())
        for c, C in enumerate(columns(probe.N)):
            pk = pr.Packet(code, n, scheme, C, bool((c + k) & 1))
            q = make(ya, pk)
            assert (q.payload_len(), q.crc_len(), q.msg_bits(), q.enc_len(), q.get_columns()) == (n, pk.w, pk.msg_bits, pk.N, C)
            assert [q.nsym(b) for b in BPS] == [pk.nsym(b) for b in BPS]
            check_decode(q, pk, ordered, want, F)
            check_encode(q, pk, payload, coded, F, BPS[c % len(BPS)])
    assert verdicts == {0, 1}, "the banks hold frames of both verdicts"


@pytest.mark.parametrize("name", sorted(CODES))
def test_every_crc_scheme_scrambler_and_symbol_width(ya, name):
    code = cc.Code(*CODES[name])
    rng = np.random.default_rng(code.K)
    for scheme in pr.SCHEMES:
        probe = pr.Packet(code, 33, scheme)
        payload, coded, ordered, want = reference(rng, probe, 9)
        for scramble in (True, False):
            pk = pr.Packet(code, 33, scheme, int(np.sqrt(probe.N)), scramble)
            q = make(ya, pk)
            check_decode(q, pk, ordered, want, 9)
            direct = pr.decode(pk, pr.sent(pk, ordered))                   # the restatement itself at this C and mask
            assert all(np.array_equal(a, b) for a, b in zip(direct, want))
            for bps in BPS:
                check_encode(q, pk, payload, coded, 9, bps)
            assert np.array_equal(pr.transmit(pk, coded), pr.encode(pk, payload))
        if scheme:
            assert set(want[1].tolist()) == {0, 1}
        else:
            assert want[1].all() and not want[2].any()


def frame_counts(q, code):
    """F around every seam of the plan: the frames of a wave and of a workgroup, each - 1, exact and + 1"""
    full = q.get_shape(1 << 16)
    fpw, G = full["frames_per_wave"], full["frames_per_wg"]
    assert fpw == max(1, 64 // code.S) and full["states_per_lane"] == max(1, code.S // 64)
    base = {1, fpw - 1, fpw, fpw + 1} if code.S < 64 else {1, 2, 5}
    return sorted(F for F in base | {G - 1, G, G + 1} if F >= 1), full


@pytest.mark.parametrize("terminated", [True, False])
@pytest.mark.parametrize("name", sorted(CODES))
def test_frame_counts_at_every_seam_and_steps_around_the_chunk(ya, name, terminated):
    code = cc.Code(*CODES[name], terminated)
    rng = np.random.default_rng(code.K * 8 + terminated)
    scheme, w, tail = pr.CRC_16, 2, code.steps(0)
    probe = make(ya, pr.Packet(code, 1, scheme))
    chunks = {probe.get_shape(1 << 16)["chunk_steps"], probe.get_shape(1)["chunk_steps"]}      # a full bank's and one frame's
    # message bytes m with T = 8 m + tail below one chunk, just above one, and above two
    ms = {(c - tail) // 8 for c in chunks} | {(c - tail) // 8 + 1 for c in chunks} | {(2 * max(chunks) - tail) // 8 + 1}
    for n in sorted(m - w for m in ms if m - w >= 1):
        pk0 = pr.Packet(code, n, scheme)
        pk = pr.Packet(code, n, scheme, int(np.sqrt(pk0.N)) + 1, True)
        q = make(ya, pk)
        counts, full = frame_counts(q, code)
        payload, coded, ordered, want = reference(rng, pk, counts[-1])
        for F in counts:
            check_decode(q, pk, ordered, want, F)                          # the planner's shape for F frames
            q.set_shape(full["frames_per_wave"], full["waves"])            # the full bank's shape on F frames
            check_decode(q, pk, ordered, want, F, pad=F % 4)
            q.set_shape(0, 0)
            check_encode(q, pk, payload, coded, F, 1 + F % 3)


@pytest.mark.parametrize("K", [3, 5, 7, 9])
def test_every_admissible_shape_gives_the_same_bytes(ya, K):
    gens = {3: (7, 5), 5: (0x17, 0x19), 7: (0x6d, 0x4f), 9: (0x1af, 0x11d)}
    code = cc.Code(K, gens[K])
    rng = np.random.default_rng(K)
    fmax = max(1, 64 // code.S)
    n, F = 36, 4 * fmax + 1
    pk = pr.Packet(code, n, pr.CRC_32, 17, True)
    q = make(ya, pk)
    payload, coded, ordered, want = reference(rng, pk, F)
    check_decode(q, pk, ordered, want, F)
    shapes = 0
    for fpw in (1, 2, 4, 8, 16, 32):
        for waves in (1, 2, 3, 4, 8):
            ok = max(1, 8 // code.S) <= fpw <= fmax and waves in (1, 2, 4)
            if not ok:
                with pytest.raises(ya.ConfigError):
                    q.set_shape(fpw, waves)
                continue
            q.set_shape(fpw, waves)
            s = q.get_shape(F)
            assert (s["frames_per_wave"], s["waves"], s["frames_per_wg"]) == (fpw, waves, fpw * waves)
            assert s["chunk_steps"] * fpw == 256
            check_decode(q, pk, ordered, want, F)
            shapes += 1
    assert shapes == 3 * len([f for f in (1, 2, 4, 8, 16) if max(1, 8 // code.S) <= f <= fmax])
    q.set_shape(0, 0)
    assert q.get_shape(F) == ya.packetizer_plan(K, n, pr.CRC_32, F)


def test_the_named_codes_a_clone_and_the_optional_outputs(ya):
    rng = np.random.default_rng(2)
    for name, spec in (("v27", cc.V27), ("v29", cc.V29), ("v39", cc.V39), ("v27p23", cc.V27P23), ("v27p34", cc.V27P34)):
        pk = pr.Packet(cc.Code(*spec), 20, pr.CRC_32, 11, True)
        q = getattr(ya.Packetizer, name)(20, columns=11)
        assert (q.crc, q.K, q.terminated, q.columns, q.scramble) == (ya.CrcScheme.CRC_32, pk.code.K, True, 11, True)
        payload = rng.integers(0, 256, (3, 20)).astype(np.uint8)
        tx = q.encode_block(payload)
        assert np.array_equal(tx, pr.encode(pk, payload)), name
        c = q.clone()
        del q
        got = c.decode_block(tx * np.uint8(255), crc=False, metric=False)
        assert np.array_equal(got[0], payload) and got[1].all() and got[2] is None and got[3] is None
        one = c.decode_block(tx[0] * np.uint8(255))                        # one frame as a 1-D row
        assert np.array_equal(one[0], payload[:1]) and one[1][0] == 1 and one[3][0] == 0
    assert c.decode_block(np.zeros((0, pk.N), np.uint8))[0].shape == (0, 20)      # no frames: nothing to do


def test_config_errors_of_a_built_object(ya):
    q = ya.Packetizer.v27(4)
    N = q.enc_len()
    with pytest.raises(ya.ConfigError):
        q.decode_block(np.zeros((2, N - 1), np.uint8))                    # rows shorter than N
    with pytest.raises(ya.ConfigError):
        q.encode_block(np.zeros((2, 3), np.uint8))
    for bps in (0, 9):
        with pytest.raises(ya.ConfigError):
            q.encode_block(np.zeros((2, 4), np.uint8), bps)
        with pytest.raises(ya.ConfigError):
            q.nsym(bps)
    with pytest.raises(ya.ConfigError):
        ya.Packetizer.v27(ya.ConvCode.v27().nmax() // 8 - 3)              # the message is longer than the code's nmax
    assert ya.Packetizer.v27(ya.ConvCode.v27().nmax() // 8 - 4).msg_bits() <= ya.ConvCode.v27().nmax()


def test_the_longest_frame(ya):
    code = cc.Code(*cc.V27)
    n = code.nmax() // 8 - 4
    pk = pr.Packet(code, n, pr.CRC_32, 181, True)
    q = make(ya, pk)
    rng = np.random.default_rng(n)
    payload, coded, ordered, want = reference(rng, pk, 2)
    check_decode(q, pk, ordered, want, 2)
    check_encode(q, pk, payload, coded, 2, 2)


def test_end_to_end_through_modem_and_channel(ya):
    """encode_block(bps = 2) -> Modem(Qpsk) -> Channel (one tap) -> soft demodulation -> decode_block, one link per frame
    and no host work on the planes: with the noise off every frame is valid; with noise everything equals the restatement
    on the same soft bytes, whatever the error rate"""
    code = cc.Code(*cc.V27)
    F, n = 8, 25
    pk = pr.Packet(code, n, pr.CRC_32, 20, True)
    q = make(ya, pk)
    rng = np.random.default_rng(8)
    payload = rng.integers(0, 256, (F, n)).astype(np.uint8)
    sym = q.encode_block(payload, 2)
    assert pk.N % 2 == 0 and sym.shape == (F, pk.N // 2)
    modem = ya.Modem(ya.ModulationScheme.Qpsk)
    tx = modem.modulate_block(sym.reshape(-1)).reshape(F, pk.N // 2)
    for snr_db in (None, 3.0):
        ch = ya.Channel(F, 1)
        ch.set_seed(1234)
        if snr_db is not None:
            ch.set_awgn_all(np.full(F, -snr_db, np.float32), np.full(F, snr_db, np.float32))      # unit gain
        rx = ch.execute(np.ascontiguousarray(tx.T)).T
        _, soft = modem.demodulate_soft_block(np.ascontiguousarray(rx).reshape(-1))
        soft = soft.reshape(F, pk.N)
        got = q.decode_block(soft)
        want = pr.decode(pk, soft)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        if snr_db is None:
            assert np.array_equal(got[0], payload) and got[1].all() and not got[3].any()
            assert np.array_equal(soft, pr.encode(pk, payload) * np.uint8(255))
        else:
            assert ((soft > 0) & (soft < 255)).any(), "the noise reached the soft bytes"
