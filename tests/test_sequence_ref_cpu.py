"""tests/sequence_ref.py passes the reference's own sequence tests (msequence.rs:173-388, bsequence.rs:204-418, their
numbers from tests/golden/sequence.npz), and its models of the kernels' schemes equal its plain loops: jumps by GF(2)
matrices equal repeated advance(), the fast push loop equals the word-array push loop, and the packed stream with
funnel shifts equals the push loop over the (N, bps, n) grid the GPU tests use."""
import numpy as np
import pytest

import sequence_ref as sr
from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("sequence")


def genpolys(gold):
    return {int(m): int(g) for m, g in zip(gold["genpoly_m"], gold["genpoly_g"])}


def test_fixture_has_the_thirty_polynomials(gold):
    G = genpolys(gold)
    assert sorted(G) == list(range(2, 32))
    assert all(g.bit_length() == m for m, g in G.items())          # create_genpoly recovers m


@pytest.mark.parametrize("m", range(2, 17))
def test_period(gold, m):                                           # msequence_test_period
    q = sr.MSequence.from_genpoly(genpolys(gold)[m])
    assert q.m == m and q.measure_period() == (1 << m) - 1


@pytest.mark.parametrize("m", range(2, 13))
def test_autocorrelation(gold, m):                                  # msequence_test_autocorrelation
    ms = sr.MSequence.from_genpoly(genpolys(gold)[m])
    n = ms.n
    bs1 = sr.BSequence.from_msequence(ms)
    bs2 = sr.BSequence.from_msequence(ms)
    assert bs1.num_bits == n and bs2.num_bits == n
    assert bs1.correlate(bs2) == n
    sym = ms.bits(n - 1)
    rxy = sr.push_correlate(bs2, bs1, sym, 1)
    assert np.all(2 * rxy - n == -1)


def test_msequence_config(gold):                                    # test_msequence_config
    with pytest.raises(sr.ConfigError):
        sr.MSequence(100, 0, 0)
    with pytest.raises(sr.ConfigError):
        sr.MSequence(1, 1, 1)
    with pytest.raises(sr.ConfigError):
        sr.MSequence(32, 1, 1)
    with pytest.raises(sr.ConfigError):
        sr.MSequence.from_genpoly(0)
    with pytest.raises(sr.ConfigError):
        sr.MSequence.from_genpoly(1)
    q = sr.MSequence.from_genpoly(genpolys(gold)[11])
    assert q.state == 1
    q.set_state(0x8A)
    assert q.state == 0x8A


def test_bsequence_init_index_correlate_add_mul_accumulate(gold):
    q = sr.BSequence(16)
    q.init(gold["init_v"])
    assert np.array_equal(q.all_bits(), gold["init_bits"])
    q0, q1, r = sr.BSequence(16), sr.BSequence(16), sr.BSequence(16)
    q0.init(gold["v0"])
    q1.init(gold["v1"])
    assert q0.correlate(q1) == int(gold["correlate"][0])
    q0.add(q1, r)
    assert np.array_equal(r.all_bits(), gold["add_bits"])
    q0.mul(q1, r)
    assert np.array_equal(r.all_bits(), gold["mul_bits"])
    q.init(gold["accumulate_v"])
    assert q.accumulate() == int(gold["accumulate"][0])


@pytest.mark.parametrize("n", [8, 16, 32, 64, 128, 256, 512])
def test_complementary_codes(n):                                    # complementary_codes_test
    a, b = sr.BSequence.ccodes(n)
    ax, bx = sr.BSequence.ccodes(n)
    for i in range(n):
        raa = 2 * a.correlate(ax) - n
        rbb = 2 * b.correlate(bx) - n
        assert raa + rbb == (2 * n if i == 0 else 0), (n, i)
        ax.circshift()
        bx.circshift()


def test_bsequence_config():
    with pytest.raises(sr.ConfigError):
        sr.BSequence(0)
    with pytest.raises(sr.ConfigError):
        sr.BSequence(sr.BSEQUENCE_NMAX + 1)
    sr.BSequence(sr.BSEQUENCE_NMAX)
    with pytest.raises(sr.ConfigError):
        sr.create_ccodes(sr.BSequence(16), sr.BSequence(24))
    with pytest.raises(sr.ConfigError):
        sr.create_ccodes(sr.BSequence(4), sr.BSequence(4))
    with pytest.raises(sr.ConfigError):
        sr.create_ccodes(sr.BSequence(12), sr.BSequence(12))
    a, b, c = sr.BSequence(32), sr.BSequence(33), sr.BSequence(64)
    with pytest.raises(sr.ConfigError):
        a.correlate(b)
    b.correlate(c)                                                  # equal word counts, unequal bit counts: accepted
    with pytest.raises(sr.ConfigError):
        a.add(a, b)
    with pytest.raises(sr.ConfigError):
        b.mul(a, b)
    with pytest.raises(sr.ConfigError):
        a.index(32)
    with pytest.raises(sr.ConfigError):
        sr.push_correlate(a, a, [1], 1)
    with pytest.raises(sr.ConfigError):
        sr.push_correlate(a, b, [1], 1)
    with pytest.raises(sr.ConfigError):
        sr.push_correlate(b, c, [1], 9)


def test_unequal_masks_use_the_receivers_correction():
    """40 bits against 50: two words each.  On all-zero windows every one of the 64 xnor bits is set, so a.correlate(b)
    = 64 - (32 - 8) = 40 and b.correlate(a) = 64 - (32 - 18) = 50; with 30 ones pushed into a alone 30 bits differ:
    34 - 24 = 10 and 34 - 14 = 20; with b's 50 bits all set and a's 40 bits all set the words differ in b's bits
    40 .. 49 alone: 54 - 24 = 30 and 54 - 14 = 40."""
    a, b = sr.BSequence(40), sr.BSequence(50)
    assert (a.correlate(b), b.correlate(a)) == (40, 50)
    for _ in range(30):
        a.push(1)
    assert (a.correlate(b), b.correlate(a)) == (10, 20)
    for _ in range(50):
        a.push(1)
        b.push(1)
    assert (a.correlate(b), b.correlate(a)) == (30, 40)


# ---- the models ------------------------------------------------------------------------------------------------------
def test_advance_is_linear_and_matrix_jumps_equal_repeated_advance(gold):
    rng = np.random.default_rng(5)
    for m, g in genpolys(gold).items():
        for hi in (False, True):                                    # a and g with bits above m - 1
            gg = g | (int(rng.integers(1, 1 << 31)) << m if hi else 0)
            gg &= sr.M32
            a = int(rng.integers(1, 1 << 32)) if hi else int(rng.integers(1, 1 << m))
            P = sr.mat_powers(gg, (1 << m) - 1, 21)
            q = sr.MSequence(m, gg, a)
            x, y = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
            assert sr.mat_apply(P[0], x ^ y) == sr.mat_apply(P[0], x) ^ sr.mat_apply(P[0], y)
            k = int(2.0 ** rng.uniform(0, 20))                      # up to 2^20, every magnitude alike
            want = sr.MSequence(m, gg, a)
            for _ in range(k):
                want.advance()
            assert sr.skip(P, q.state, k) == want.state, (m, hi, k)
            assert sr.skip(P, q.state, 0) == a


@pytest.mark.parametrize("m,g,a", [(2, 0x3, 1), (7, 0x60, 1), (16, 0xD008, 0xFFFF0001), (31, 0x40000004, 0x80000001)])
@pytest.mark.parametrize("bps", [1, 3, 8])
def test_block_model_of_the_generator_equals_the_serial_stream(m, g, a, bps):
    tile = 1024                                                     # the same split into tiles, waves and lanes, smaller
    for n in (1, tile - 1, tile + 1, 2 * tile + 17):
        q, want = sr.MSequence(m, g, a), sr.MSequence(m, g, a)
        got = sr.mseq_block_model(q, bps, n, tile)
        assert got.tobytes() == want.symbols(bps, n).tobytes(), (m, bps, n)
        assert q.state == want.state


@pytest.mark.parametrize("N,bps", [(1, 1), (31, 3), (33, 2), (64, 8), (100, 5), (255, 7)])
def test_fast_push_loop_equals_the_word_array_push_loop(N, bps):
    rng = np.random.default_rng(N)
    q, ref = sr.BSequence(N), sr.BSequence(N)
    q.init(rng.integers(0, 256, (N + 7) // 8))
    ref.init(rng.integers(0, 256, (N + 7) // 8))
    q2 = q.clone()
    q2.load(rng.integers(0, 256, (N + 7) // 8))                     # load() and all_bits() against init() and index()
    v = rng.integers(0, 256, (N + 7) // 8)
    q.init(v)
    q2.load(v)
    assert q.s == q2.s and q.all_bits().tolist() == [q.index(i) for i in range(N)]
    sym = rng.integers(0, 256, 300).astype(np.uint8)
    assert np.array_equal(sr.push_correlate(q, ref, sym, bps), sr.push_correlate_plain(q2, ref, sym, bps))
    assert q.s == q2.s
    sr.push_correlate(q, ref, sym, bps, want_rxy=False)
    sr.push_correlate_plain(q2, ref, sym, bps, want_rxy=False)
    assert q.s == q2.s


@pytest.mark.parametrize("bps", sr.GRID_BPS)
@pytest.mark.parametrize("N", sr.GRID_N)
def test_packed_window_model_equals_the_push_loop(N, bps):
    q0, r0, calls = sr.grid_case(N, bps)
    q, ref = sr.BSequence(N), sr.BSequence(N)
    q.load(q0)
    ref.load(r0)
    for n, sym, rxy, bits in calls:
        got = sr.packed_model(q, ref, sym, bps)
        assert got.tobytes() == rxy.tobytes(), (N, bps, n)
        assert q.all_bits().tobytes() == bits.tobytes(), (N, bps, n)


def test_packed_window_model_with_unequal_masks():
    rng = np.random.default_rng(9)
    for nq, nr in ((50, 40), (40, 50)):
        q, ref = sr.BSequence(nq), sr.BSequence(nr)
        ref.init(rng.integers(0, 256, 7))
        q2 = q.clone()
        sym = rng.integers(0, 256, 200).astype(np.uint8)
        assert np.array_equal(sr.packed_model(q, ref, sym, 3), sr.push_correlate_plain(q2, ref, sym, 3))
        assert q.s == q2.s
