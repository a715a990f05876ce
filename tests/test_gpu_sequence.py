"""MSequence and BSequence on the GPU against tests/sequence_ref.py: every comparison is tobytes() equality (the outputs
are integers).  The generator polynomials come from tests/golden/sequence.npz; the correlator's (N, bps, n) grid and its
expected results are sequence_ref.grid_case, shared with tests/test_sequence_ref_cpu.py."""
import functools

import numpy as np
import pytest

import sequence_ref as sr
from conftest import load_golden

pytestmark = pytest.mark.gpu
MT, BT = sr.MSEQUENCE_TILE, sr.BSEQUENCE_TILE
G = {int(m): int(g) for m, g in zip(*(load_golden("sequence")[k] for k in ("genpoly_m", "genpoly_g")))}


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert (yagi_amd.MSEQUENCE_TILE, yagi_amd.BSEQUENCE_TILE, yagi_amd.BSEQUENCE_NMAX) == (MT, BT, sr.BSEQUENCE_NMAX)
    return yagi_amd


# ---- MSequence -------------------------------------------------------------------------------------------------------
MSEQ_N = (0, 1, MT - 1, MT, MT + 1, 3 * MT + 17)


@functools.lru_cache(maxsize=None)
def ref_stream(m, g, a, bps, nmax, marks):
    """nmax symbols from a fresh MSequence(m, g, a), and the state after the first n of them for every n in marks"""
    q = sr.MSequence(m, g, a)
    out, states = np.zeros(nmax, np.uint8), {}
    for i in range(nmax + 1):
        if i in marks:
            states[i] = q.state
        if i < nmax:
            out[i] = q.generate_symbol(bps)
    return out, states


@pytest.mark.parametrize("form,bps", [("bits", 1), ("sym", 1), ("sym", 3), ("sym", 8)])
@pytest.mark.parametrize("m", [2, 3, 7, 16, 31])
def test_msequence_blocks_equal_the_serial_stream(ya, m, form, bps):
    want, states = ref_stream(m, G[m], 1, bps, max(MSEQ_N), MSEQ_N)
    for n in MSEQ_N:
        q = ya.MSequence(m, G[m])
        got = q.generate_bits_block(n) if form == "bits" else q.generate_symbols_block(bps, n)
        assert got.dtype == np.uint8 and got.tobytes() == want[:n].tobytes(), (m, form, bps, n)
        assert q.get_state() == states[n], (m, form, bps, n)


def test_msequence_m2_wraps_its_period_a_thousand_times(ya):
    q, r = ya.MSequence(2, G[2]), sr.MSequence(2, G[2])
    assert q.generate_bits_block(4099).tobytes() == r.bits(4099).tobytes()
    assert q.get_state() == r.state


def test_msequence_scalar_and_block_calls_interleave_on_one_stream(ya):
    m = 16
    q, r = ya.MSequence(m, G[m]), sr.MSequence(m, G[m])
    assert (q.get_genpoly(), q.get_genpoly_length(), q.get_length(), q.get_state()) == (G[m], m, (1 << m) - 1, 1)
    assert q.generate_symbols_block(3, MT + 5).tobytes() == r.symbols(3, MT + 5).tobytes()
    assert q.get_state() == r.state
    assert q.advance() == r.advance() and q.get_state() == r.state
    assert q.generate_symbol(5) == r.generate_symbol(5) and q.get_state() == r.state
    assert q.generate_symbol(32) == r.generate_symbol(32) and q.generate_symbol(0) == 0
    assert q.generate_bits_block(2 * MT + 3).tobytes() == r.bits(2 * MT + 3).tobytes()
    assert q.get_state() == r.state
    q.reset()
    r.reset()
    assert q.get_state() == 1
    assert q.generate_symbols_block(8, 100).tobytes() == r.symbols(8, 100).tobytes()


@pytest.mark.parametrize("m,g,a", [(7, 0x60 | 0xABCD0000, 0xFFFF0001), (16, 0xD008 | 0x5A5A0000, 0x80000001),
                                   (31, 0x40000004 | 0x80000000, 0xFFFFFFFF)])
def test_msequence_state_and_polynomial_with_high_bits(ya, m, g, a):
    """neither create nor set_state masks: the first advance() sees the whole state and the whole of g"""
    q, r = ya.MSequence(m, g, a), sr.MSequence(m, g, a)
    assert q.get_state() == a
    assert q.generate_symbols_block(3, MT + 9).tobytes() == r.symbols(3, MT + 9).tobytes()
    assert q.get_state() == r.state
    q.set_state(a ^ 0x40000000)
    r.set_state(a ^ 0x40000000)
    assert q.get_state() == a ^ 0x40000000
    assert q.generate_bits_block(MT + 1).tobytes() == r.bits(MT + 1).tobytes()
    q.set_state(a)
    r.set_state(a)
    assert q.advance() == r.advance() and q.get_state() == r.state


def test_msequence_clone_continues_identically(ya):
    q = ya.MSequence.from_genpoly(G[11])
    assert q.get_genpoly_length() == 11
    q.generate_bits_block(777)
    c = q.clone()
    assert c.get_state() == q.get_state() and c.get_genpoly() == q.get_genpoly()
    assert c.generate_symbols_block(4, MT + 3).tobytes() == q.generate_symbols_block(4, MT + 3).tobytes()
    assert c.get_state() == q.get_state()
    c.reset()
    assert c.get_state() == 1


def test_msequence_skip(ya):
    rng = np.random.default_rng(3)
    for m in (2, 5, 13, 24, 31):
        q, r = ya.MSequence(m, G[m]), sr.MSequence(m, G[m])
        for k in [0, 1, 2, (1 << 16) - 1] + [int(k) for k in rng.integers(0, 1 << 16, 4)]:
            q.skip(k)
            for _ in range(k):
                r.advance()
            assert q.get_state() == r.state, (m, k)
        # the upper matrices: the sequence has period 2^m - 1 from state 1 on
        k = (1 << 40) + 12345
        a, b = ya.MSequence(m, G[m]), ya.MSequence(m, G[m])
        a.skip(k)
        b.skip(k % ((1 << m) - 1))
        assert a.get_state() == b.get_state(), m
        k = (1 << 63) + (1 << 50) + 99
        a.skip(k)
        b.skip(k % ((1 << m) - 1))
        assert a.get_state() == b.get_state(), m


@pytest.mark.parametrize("m", [2, 3, 8, 13, 16, 20, 24])
def test_msequence_measure_period(ya, m):
    q = ya.MSequence.from_genpoly(G[m])
    assert q.measure_period() == (1 << m) - 1
    assert q.get_state() == 1


def test_msequence_config_errors(ya):
    for m in (0, 1, 32, 100):
        with pytest.raises(ya.ConfigError):
            ya.MSequence(m, 3, 1)
    for g in (0, 1, 0x80000001):
        with pytest.raises(ya.ConfigError):
            ya.MSequence.from_genpoly(g)
    q = ya.MSequence(7, G[7])
    for bps in (0, 9, 33):
        with pytest.raises(ya.ConfigError):
            q.generate_symbols_block(bps, 16)
    with pytest.raises(ya.ConfigError):
        q.generate_symbol(33)
    assert q.get_state() == 1                                       # a rejected call leaves the state alone
    assert q.generate_symbols_block(8, 0).size == 0


# ---- BSequence -------------------------------------------------------------------------------------------------------
def gpu_bits(q):
    return np.array([q.index(i) for i in range(q.get_length())], np.uint8)


@pytest.mark.parametrize("bps", sr.GRID_BPS)
@pytest.mark.parametrize("N", sr.GRID_N)
def test_push_correlate_block_grid(ya, N, bps):
    q0, r0, calls = sr.grid_case(N, bps)
    q, ref = ya.BSequence(N), ya.BSequence(N)
    q.init(q0)
    ref.init(r0)
    for n, sym, rxy, bits in calls:                                 # every call reads the history of the one before
        got = q.push_correlate_block(ref, sym, bps)
        assert got.dtype == np.int32 and got.tobytes() == rxy.tobytes(), (N, bps, n)
        assert gpu_bits(q).tobytes() == bits.tobytes(), (N, bps, n)


def test_two_block_calls_with_scalar_pushes_between(ya):
    N, bps = 100, 3
    rng = np.random.default_rng(11)
    v, w = rng.integers(0, 256, 13).astype(np.uint8), rng.integers(0, 256, 13).astype(np.uint8)
    q, ref, rq, rref = ya.BSequence(N), ya.BSequence(N), sr.BSequence(N), sr.BSequence(N)
    ref.init(w)
    rref.init(w)
    q.init(v)
    rq.init(v)
    s1, s2 = rng.integers(0, 8, BT + 7).astype(np.uint8), rng.integers(0, 8, 50).astype(np.uint8)
    assert q.push_correlate_block(ref, s1, bps).tobytes() == sr.push_correlate(rq, rref, s1, bps).tobytes()
    for b in (1, 0, 1, 1):
        q.push(b)
        rq.push(b)
    q.circshift()
    rq.circshift()
    assert ref.correlate(q) == rref.correlate(rq) and q.accumulate() == rq.accumulate()
    assert q.push_correlate_block(ref, s2, bps).tobytes() == sr.push_correlate(rq, rref, s2, bps).tobytes()
    assert gpu_bits(q).tobytes() == rq.all_bits().tobytes()
    # ref is read as it stands when the call is made
    ref.push(1)
    rref.push(1)
    assert q.push_correlate_block(ref, s2, bps).tobytes() == sr.push_correlate(rq, rref, s2, bps).tobytes()
    c = q.clone()
    assert gpu_bits(c).tobytes() == rq.all_bits().tobytes()
    q.reset()
    assert q.accumulate() == 0 and c.accumulate() == rq.accumulate()


def test_symbol_bits_above_bps_are_ignored(ya):
    N = 77
    ref, q1, q2 = ya.BSequence(N), ya.BSequence(N), ya.BSequence(N)
    ref.init(np.arange(10, dtype=np.uint8) * 37)
    a = q1.push_correlate_block(ref, np.full(BT + 3, 0xFF, np.uint8), 3)
    b = q2.push_correlate_block(ref, np.full(BT + 3, 7, np.uint8), 3)
    assert a.tobytes() == b.tobytes() and gpu_bits(q1).tobytes() == gpu_bits(q2).tobytes()
    rq, rref = sr.BSequence(N), sr.BSequence(N)
    rref.init(np.arange(10, dtype=np.uint8) * 37)
    assert a.tobytes() == sr.push_correlate(rq, rref, np.full(BT + 3, 7, np.uint8), 3).tobytes()


def test_unequal_masks_take_the_receivers_correction(ya):
    """40 bits against 50: the same word count.  With 30 ones pushed into the 40-bit one alone, a.correlate(b) = 10 and
    b.correlate(a) = 20 (tests/test_sequence_ref_cpu.py derives both); the block form has ref as the receiver."""
    a, b, ra, rb = ya.BSequence(40), ya.BSequence(50), sr.BSequence(40), sr.BSequence(50)
    for _ in range(30):
        a.push(1)
        ra.push(1)
    assert (a.correlate(b), b.correlate(a)) == (10, 20) == (ra.correlate(rb), rb.correlate(ra))
    rng = np.random.default_rng(4)
    sym = rng.integers(0, 256, BT + 11).astype(np.uint8)
    qa, qb = a.clone(), b.clone()
    assert qb.push_correlate_block(a, sym, 2).tobytes() == sr.push_correlate(rb.clone(), ra, sym, 2).tobytes()
    assert qa.push_correlate_block(b, sym, 2).tobytes() == sr.push_correlate(ra.clone(), rb, sym, 2).tobytes()


def test_bsequence_config_errors(ya):
    with pytest.raises(ya.ConfigError):
        ya.BSequence(0)
    with pytest.raises(ya.ConfigError):
        ya.BSequence(sr.BSEQUENCE_NMAX + 1)
    a, b, c = ya.BSequence(32), ya.BSequence(33), ya.BSequence(64)
    sym = np.zeros(4, np.uint8)
    with pytest.raises(ya.ConfigError):
        a.push_correlate_block(b, sym, 1)                           # unequal word counts
    with pytest.raises(ya.ConfigError):
        a.push_correlate_block(a, sym, 1)                           # ref is q
    for bps in (0, 9):
        with pytest.raises(ya.ConfigError):
            b.push_correlate_block(c, sym, bps)
    with pytest.raises(ya.ConfigError):
        a.correlate(b)
    assert b.correlate(c) == 33                                     # equal word counts: accepted, b's correction
    with pytest.raises(ya.ConfigError):
        a.add(a, b)
    with pytest.raises(ya.ConfigError):
        a.index(32)
    with pytest.raises(ya.ConfigError):
        a.init(np.zeros(3, np.uint8))
    for n in (4, 12):
        with pytest.raises(ya.ConfigError):
            ya.BSequence.ccodes(n)
    x, y = ya.BSequence(16), ya.BSequence(24)
    with pytest.raises(ya.ConfigError):
        ya._check(ya.lib.yagi_hip_bsequence_create_ccodes(x._h, y._h))
    assert b.push_correlate_block(c, np.zeros(0, np.uint8), 1).size == 0


def test_rxy_none_leaves_the_same_state(ya):
    N, bps = 255, 2
    rng = np.random.default_rng(8)
    sym = rng.integers(0, 4, 2 * BT + 9).astype(np.uint8)
    ref, q1, q2 = ya.BSequence(N), ya.BSequence(N), ya.BSequence(N)
    ref.init(rng.integers(0, 256, 32).astype(np.uint8))
    q1.push_correlate_block(ref, sym, bps)
    assert q2.push_correlate_block(ref, sym, bps, rxy=None) is None
    rq = sr.BSequence(N)
    sr.push_correlate(rq, sr.BSequence(N), sym, bps, want_rxy=False)
    assert gpu_bits(q1).tobytes() == gpu_bits(q2).tobytes() == rq.all_bits().tobytes()


def test_reference_known_answers_through_the_library(ya):
    gold = load_golden("sequence")
    q = ya.BSequence(16)
    q.init(gold["init_v"])
    assert gpu_bits(q).tobytes() == gold["init_bits"].tobytes()
    q0, q1, r = ya.BSequence(16), ya.BSequence(16), ya.BSequence(16)
    q0.init(gold["v0"])
    q1.init(gold["v1"])
    assert q0.correlate(q1) == int(gold["correlate"][0])
    q0.add(q1, r)
    assert gpu_bits(r).tobytes() == gold["add_bits"].tobytes()
    q0.mul(q1, r)
    assert gpu_bits(r).tobytes() == gold["mul_bits"].tobytes()
    q.init(gold["accumulate_v"])
    assert q.accumulate() == int(gold["accumulate"][0])
    for n in (8, 64, 512):                                          # complementary codes, as the reference's test
        a, b = ya.BSequence.ccodes(n)
        ra, rb = sr.BSequence.ccodes(n)
        assert gpu_bits(a).tobytes() == ra.all_bits().tobytes() and gpu_bits(b).tobytes() == rb.all_bits().tobytes()


# ---- properties through the block form -------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(2, 13))
def test_msequence_autocorrelation_through_the_block_forms(ya, m):
    ms = ya.MSequence.from_genpoly(G[m])
    n = ms.get_length()
    bs1 = ya.BSequence.from_msequence(ms)
    bs2 = ya.BSequence.from_msequence(ms)
    assert bs1.get_length() == n == bs2.get_length()
    assert bs1.correlate(bs2) == n
    rxy = bs2.push_correlate_block(bs1, ms.generate_bits_block(n - 1), 1)
    assert np.all(2 * rxy - n == -1)
    assert bs2.push_correlate_block(bs1, ms.generate_bits_block(1), 1)[0] == n      # a whole period later: aligned again


def test_device_resident_chain_generator_modem_correlator(ya):
    """MSequence -> Modem(QPSK) modulate -> demodulate -> BSequence correlate, all on device buffers.  The preamble is
    the 255 bits of the same m = 8 sequence; where the peaks are is taken from the reference loop (255 is odd, so the
    period does not line up with the 2-bit symbols every time)."""
    m, bps, n = 8, 2, 3 * BT + 17
    ms, rms = ya.MSequence.from_genpoly(G[m]), sr.MSequence.from_genpoly(G[m])
    ref, rref = ya.BSequence.from_msequence(ms), sr.BSequence.from_msequence(rms)
    assert ms.get_state() == rms.state
    sym = ya.DeviceArray(n, np.uint8)
    x = ya.DeviceArray(n, np.complex64)
    dem = ya.DeviceArray(n, np.uint8)
    rxy = ya.DeviceArray(n, np.int32)
    mod, q = ya.Modem(ya.ModulationScheme.Qpsk), ya.BSequence(255)
    ms.generate_symbols_block_devptr(bps, n, sym)
    mod.modulate_block_devptr(sym, n, x)
    mod.demodulate_block_devptr(x, n, dem, None)
    q.push_correlate_block_devptr(ref, dem, n, bps, rxy)
    ya.synchronize()
    want_sym = rms.symbols(bps, n)
    assert sym.to_numpy().tobytes() == want_sym.tobytes() == dem.to_numpy().tobytes()
    want = sr.push_correlate(sr.BSequence(255), rref, want_sym, bps)
    got = rxy.to_numpy()
    assert got.tobytes() == want.tobytes()
    peaks = np.flatnonzero(want == 255)
    assert peaks.size >= n * bps // 255 // 2 - 1 and np.array_equal(np.flatnonzero(got == 255), peaks)
    assert np.all(np.diff(peaks) == 255)                            # every second period ends on a symbol boundary
