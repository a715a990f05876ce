"""SymStream on the GPU against the composition that defines it (tests/symstream_ref.py): MSequence.generate_symbols_block
-> Modem.modulate_block -> x gain per component -> FirInterpolationFilter("crcf").execute_block, with a Python model of
buf_index.  Every comparison is tobytes() equality.  Generators come from tests/golden/sequence.npz."""
import numpy as np
import pytest

from gpu_util import rand_taps
from osc_ref import validate_psd_spectrum
from symstream_ref import SymStreamParts, golden_generator

pytestmark = pytest.mark.gpu
PLAN_FEW, PLAN_TAPS_LDS, PLAN_TAPS_GLOBAL = 0, 1, 2


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def same(a, b):
    a, b = np.ascontiguousarray(a, np.complex64), np.ascontiguousarray(b, np.complex64)
    return a.size == b.size and a.tobytes() == b.tobytes()


def make(ya, k, m, scheme, seed, gen_m=23, modem=None):
    """(SymStream from random taps, its composition): 2km+1 taps, so Ls = 2m+1"""
    S = ya.ModulationScheme
    h = rand_taps(np.random.default_rng(seed), "crcf", 2 * k * m + 1)
    src = ya.MSequence(*golden_generator(gen_m))
    src.skip(1000 + seed)                                   # created from a source in mid-sequence
    state = src.get_state()
    q = ya.SymStream.from_taps(k, h, S.Qpsk if modem is not None else scheme, src)
    md = modem if modem is not None else ya.Modem(scheme)
    if modem is not None:
        q.set_modem(modem)
    assert src.get_state() == state == q.source_get_state()  # copied, not touched
    return q, SymStreamParts(ya, k, h, md, src), src


def check_source(ya, q, ref, src):
    """the object's source stands where a host MSequence stands after the bits the composition consumed"""
    host = src.clone()
    host.skip(ref.bits)
    assert q.source_get_state() == host.get_state() == ref.src.get_state()


@pytest.mark.parametrize("m", [1, 7, 31])
@pytest.mark.parametrize("k", [2, 5, 16])
def test_few_branch_plan(ya, k, m):
    S = ya.ModulationScheme
    assert ya.plan_firpfb_all(8, 4, k, 2 * m + 1).kind == PLAN_FEW
    q, ref, src = make(ya, k, m, S.Qam16, 100 * k + m)
    assert q.is_fused() and q.get_k() == k and q.get_m() == m and q.get_delay() == k * m
    assert q.get_ftype() == ya.FirFilterShape.Unknown
    for nsym in (1, 255, 256, 257, 515):
        assert same(q.write_samples(nsym * k), ref.write_samples(nsym * k)), (k, m, nsym)
        assert q.get_buf_index() == 0
    check_source(ya, q, ref, src)


def test_all_branches_plan_with_taps_in_lds(ya):
    S = ya.ModulationScheme
    k, m = 17, 3
    assert ya.plan_firpfb_all(8, 4, k, 2 * m + 1).kind == PLAN_TAPS_LDS
    q, ref, src = make(ya, k, m, S.Qam64, 7)
    assert q.is_fused()
    for nsym in (63, 64, 65, 130):
        assert same(q.write_samples(nsym * k), ref.write_samples(nsym * k)), nsym
    assert same(q.write_samples(3 * k + 5), ref.write_samples(3 * k + 5))       # ends inside a symbol
    assert same(q.write_samples(100), ref.write_samples(100))                   # starts inside one
    check_source(ya, q, ref, src)


def test_all_branches_plan_with_taps_global(ya):
    S = ya.ModulationScheme
    k, m = 64, 100
    assert ya.plan_firpfb_all(8, 4, k, 2 * m + 1).kind == PLAN_TAPS_GLOBAL
    q, ref, src = make(ya, k, m, S.Psk8, 8)
    assert q.is_fused()
    assert same(q.write_samples(70 * k), ref.write_samples(70 * k))
    assert same(q.write_samples(3 * k + 63), ref.write_samples(3 * k + 63))
    assert same(q.write_samples(66), ref.write_samples(66))
    check_source(ya, q, ref, src)


@pytest.mark.parametrize("k,m,tile,scheme", [(2, 7, 256, "Qpsk"), (17, 3, 64, "Qam64")])
def test_long_calls_stage_several_tiles_per_workgroup(ya, k, m, tile, scheme):
    """a call of more than 1024 tiles gives a workgroup several of them (one LFSR jump for all): 2050 tiles and a ragged
    end, from inside a symbol, then the caller's symbols at the same length"""
    S = ya.ModulationScheme
    q, ref, src = make(ya, k, m, S[scheme], 31)
    assert q.is_fused()
    assert same(q.write_samples(k + 1), ref.write_samples(k + 1))
    n = (2050 * tile + 77) * k + 1
    assert same(q.write_samples(n), ref.write_samples(n))
    assert same(q.write_samples(k - 2), ref.write_samples(k - 2)) and q.get_buf_index() == 0
    sym = np.random.default_rng(32).integers(0, 1 << ya.Modem(S[scheme]).get_bps(), 2050 * tile + 77).astype(np.uint8)
    assert same(q.modulate_symbols(sym), ref.modulate_symbols(sym))
    assert same(q.write_samples(1337), ref.write_samples(1337))
    check_source(ya, q, ref, src)


@pytest.mark.parametrize("name", ["Bpsk", "Qpsk", "Psk8", "Qam16", "Qam256", "Ask4", "Ook", "from_table", "Dpsk4"])
def test_schemes(ya, name):
    S = ya.ModulationScheme
    k, m = 4, 5
    if name == "from_table":
        rng = np.random.default_rng(11)
        table = (rng.standard_normal(32) + 1j * rng.standard_normal(32)).astype(np.complex64)
        q, ref, src = make(ya, k, m, None, 12, modem=ya.Modem.from_table(table))
        assert q.get_scheme() == S.Arb
    else:
        q, ref, src = make(ya, k, m, S[name], 12)
        assert q.get_scheme() == S[name]
    assert q.is_fused() == (name != "Dpsk4")
    q.set_gain(0.7)
    ref.set_gain(0.7)
    for n in (1337, 1337, 2):
        assert same(q.write_samples(n), ref.write_samples(n)), (name, n)
    check_source(ya, q, ref, src)


def test_cuts_of_the_stream(ya):
    """k = 5, m = 17, the reference's clone-test shape (symstream.rs:307-313): the calls sample by sample against one
    call of their sum, and against the composition"""
    S = ya.ModulationScheme
    cuts = [1, 4, 5, 6, 1337, 3, 1337]
    q, ref, src = make(ya, 5, 17, S.Qpsk, 21)
    whole = q.clone()
    assert same(q.write_samples(0), np.zeros(0, np.complex64)) and q.get_buf_index() == 0
    parts = []
    for n in cuts:
        y = q.write_samples(n)
        assert same(y, ref.write_samples(n)), n
        parts.append(y)
        q.write_samples(0)                                  # a no-op anywhere in the stream
        assert q.get_buf_index() == ref.p
    assert same(np.concatenate(parts), whole.write_samples(sum(cuts)))
    assert q.source_get_state() == whole.source_get_state()
    check_source(ya, q, ref, src)


def test_gain_and_scheme_change_between_calls_that_end_inside_a_symbol(ya):
    S = ya.ModulationScheme
    q, ref, src = make(ya, 5, 17, S.Qpsk, 22)
    steps = [(203, None, 0.5), (7, S.Qam64, None), (1001, None, -1.25), (4, S.Dpsk4, None), (1337, None, 3.0),
             (2, S.Qpsk, 1.0), (998, None, None), (5, S.Dpsk4, None), (12, None, 0.0)]
    for n, scheme, gain in steps:
        assert same(q.write_samples(n), ref.write_samples(n)), (n, scheme, gain)
        assert q.get_buf_index() == ref.p
        if scheme is not None:
            q.set_scheme(scheme)
            ref.set_modem(ya.Modem(scheme))
            assert q.get_scheme() == scheme and q.is_fused() == (scheme != S.Dpsk4)
        if gain is not None:
            q.set_gain(gain)
            ref.set_gain(gain)
            assert q.get_gain() == np.float32(gain)
    assert same(q.write_samples(77), ref.write_samples(77))
    check_source(ya, q, ref, src)


@pytest.mark.parametrize("scheme", ["Qam16", "Dpsk4"])
def test_modulate_symbols(ya, scheme):
    S = ya.ModulationScheme
    k = 5
    q, ref, src = make(ya, k, 17, S[scheme], 23)
    rng = np.random.default_rng(24)
    M = 1 << ya.Modem(S[scheme]).get_bps()
    sym = rng.integers(0, M, 700).astype(np.uint8)
    s0 = q.source_get_state()
    assert same(q.modulate_symbols(sym), ref.modulate_symbols(sym))
    assert q.source_get_state() == s0                       # the source does not advance
    bad = sym.copy()
    bad[413] = M
    y = np.full(bad.size * k, np.complex64(7 - 7j))
    with pytest.raises(ya.RangeError):
        q.modulate_symbols(bad, y)
    assert np.all(y == np.complex64(7 - 7j)) and q.get_buf_index() == 0
    assert same(q.write_samples(k * 40 + 2), ref.write_samples(k * 40 + 2))     # the state did not move; now off a boundary
    with pytest.raises(ya.ModeError):
        q.modulate_symbols(sym[:3])
    assert same(q.write_samples(k - 2), ref.write_samples(k - 2))
    assert same(q.modulate_symbols(sym[:300]), ref.modulate_symbols(sym[:300]))
    assert same(q.write_samples(1337), ref.write_samples(1337))
    check_source(ya, q, ref, src)


def test_source_bookkeeping_reset_and_clone(ya):
    S = ya.ModulationScheme
    q, ref, src = make(ya, 5, 17, S.Dpsk4, 25)              # the reference's clone test is Dpsk4
    for scheme in (S.Dpsk4, S.Qam16):
        q.set_scheme(scheme)
        ref.set_modem(ya.Modem(scheme))
        assert same(q.write_samples(1337), ref.write_samples(1337))
        check_source(ya, q, ref, src)
        s = q.source_get_state()
        q.reset()
        ref.reset()
        assert q.source_get_state() == s and q.get_buf_index() == 0
        assert same(q.write_samples(1338), ref.write_samples(1338))
        c = q.clone()
        assert (c.get_k(), c.get_m(), c.get_scheme(), c.get_gain(), c.get_buf_index(), c.source_get_state()) == \
               (q.get_k(), q.get_m(), q.get_scheme(), q.get_gain(), q.get_buf_index(), q.source_get_state())
        a, b = q.write_samples(1337), c.write_samples(1337)  # the assertion symstream.rs:332 had to comment out
        assert same(a, b) and same(a, ref.write_samples(1337))
    q.source_set_state(src.get_state())                     # rewind: the stream's symbols repeat
    q.reset()
    again = SymStreamParts(ya, 5, rand_taps(np.random.default_rng(25), "crcf", 2 * 5 * 17 + 1), ya.Modem(S.Qam16), src)
    assert same(q.write_samples(333), again.write_samples(333))


DELAY_SHAPES = [(2, 4), (2, 5), (2, 6), (2, 7), (2, 8), (2, 9), (2, 10), (2, 14), (2, 20), (2, 31), (3, 12), (4, 12),
                (5, 12), (6, 12), (7, 12), (8, 12), (9, 12), (10, 12), (11, 12), (12, 12)]


def test_reference_delay_cases(ya):
    """symstreamcf_delay_00..19 (symstream.rs:132-236): Arkaiser, beta 0.3, Qpsk; the first sample with |y| > 0.9 is
    within 2 + k of k m.  The pair (5, 12) runs one sample per call, as the reference does."""
    S, F = ya.ModulationScheme, ya.FirFilterShape
    for k, m in DELAY_SHAPES:
        q = ya.SymStream(F.Arkaiser, k, m, 0.3, S.Qpsk, ya.MSequence(*golden_generator(23)))
        assert q.is_fused() and q.get_ftype() == F.Arkaiser and q.get_beta() == np.float32(0.3)
        delay = q.get_delay()
        assert delay == k * m
        n = 1000 + delay
        if (k, m) == (5, 12):
            y = np.concatenate([q.write_samples(1) for _ in range(n)])
        else:
            y = q.write_samples(n)
        first = int(np.flatnonzero(np.abs(y) > 0.9)[0])
        assert abs(first - delay) <= 2 + k, (k, m, first)


@pytest.mark.parametrize("k,m,beta", [(2, 12, 0.30), (4, 12, 0.30), (4, 25, 0.20), (7, 11, 0.35)])
def test_reference_psd_cases(ya, k, m, beta):
    """symstreamcf_psd_* (symstream.rs:238-301): gain 1/sqrt(k), 192000 k samples in calls of 1337 into
    Spgram.default(2400); at most -80 dB outside +-0.5 (1 + beta) / k, within +-1 dB inside +-0.5 (1 - beta) / k"""
    S, F = ya.ModulationScheme, ya.FirFilterShape
    q = ya.SymStream(F.Arkaiser, k, m, beta, S.Qpsk, ya.MSequence(*golden_generator(23)))
    q.set_gain(np.float32(1.0) / np.sqrt(np.float32(k)))
    sp = ya.Spgram.default(2400)
    buf = ya.DeviceArray(1337, np.complex64)
    n = 0
    while n < 192000 * k:
        q.write_samples_devptr(buf, 1337)
        sp.write_dev(buf, 1337)
        n += 1337
    psd = sp.get_psd()
    f0, f1 = np.float32(0.5 * (1.0 - beta) / k), np.float32(0.5 * (1.0 + beta) / k)
    regions = [(-0.5, -f1, 0.0, -80.0, False, True), (-f0, f0, -1.0, 1.0, True, True), (f1, 0.5, 0.0, -80.0, False, True)]
    f = np.arange(2400, dtype=np.float32) / np.float32(2400) - np.float32(0.5)
    print(f"k {k} m {m} beta {beta}: passband {psd[(f >= -f0) & (f <= f0)].min():+.3f} .. "
          f"{psd[(f >= -f0) & (f <= f0)].max():+.3f} dB, stopband max {psd[(f <= -f1) | (f >= f1)].max():.2f} dB")
    assert validate_psd_spectrum(psd, 2400, regions)
