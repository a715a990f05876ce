"""SymStreamR on the GPU against the composition that defines it (tests/symstreamr_ref.py): the library's SymStream at
k = 2 into MsResamp("crcf", 0.5 / bw, 60), fed exactly the samples the reference would have pushed.  Every sample
comparison is tobytes() equality; shapes come from plan_symstreamr.  Generators come from tests/golden/sequence.npz.
The reference's own tests (symstreamr.rs:140-326, msresamp.rs:180-228) run at their own tolerances at the end."""
import numpy as np
import pytest

from osc_ref import validate_psd_spectrum
from symstream_ref import golden_generator
from symstreamr_ref import SymStreamRParts

pytestmark = pytest.mark.gpu
BWS = [1.0, 0.77, 0.5, 0.4, 0.25, 0.2, 0.03, 0.01, 0.001]   # 0.01: five stages, the first count whose chain is a launch per stage
STAGES = {1.0: 0, 0.77: 0, 0.5: 0, 0.4: 0, 0.25: 0, 0.2: 1, 0.03: 4, 0.01: 5, 0.001: 8}


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def same(a, b):
    a, b = np.ascontiguousarray(a, np.complex64), np.ascontiguousarray(b, np.complex64)
    return a.size == b.size and a.tobytes() == b.tobytes()


def make(ya, bw, shape="arkaiser", seed=0, scheme=None):
    """(SymStreamR, its composition, the source as it stood at creation)"""
    S, F = ya.ModulationScheme, ya.FirFilterShape
    ftype, m, beta, ms = (F.Arkaiser, 7, 0.3, S.Qpsk) if shape == "arkaiser" else (F.Rrcos, 12, 0.25, S.Qam64)
    ms = ms if scheme is None else scheme
    src = ya.MSequence(*golden_generator(23))
    src.skip(1000 + seed)                                    # created from a source in mid-sequence
    state = src.get_state()
    q = ya.SymStreamR(ftype, bw, m, beta, ms, src)
    assert src.get_state() == state == q.source_get_state()   # copied, not touched
    return q, SymStreamRParts(ya, ftype, bw, m, beta, ms, src), src


def check_source(q, ref, src):
    """the object's source stands where a host MSequence stands after the bits of the symbols the reference pushed"""
    host = src.clone()
    host.skip(ref.bits)
    assert q.source_get_state() == host.get_state() == ref.S.source_get_state()


def ragged(ya, bw, m):
    """the calls of the ragged sequence: arbitrary-stage outputs' worth 1, 2, 3, T-1, T, T+1, three tiles and a ragged
    end, and forty calls of one sample; where there are half-band stages, a call the leftover covers"""
    p = ya.plan_symstreamr(bw, m, 1)
    T, g = p.tile, 1 << p.stages
    calls = [1 * g, 2 * g, 3 * g, (T - 1) * g, T * g, (T + 1) * g, 3 * T * g + 5 * g + (g // 2 + 1)]
    return calls, T, g


@pytest.mark.parametrize("shape,bw", [("arkaiser", bw) for bw in BWS] + [("rrcos", 0.77), ("rrcos", 0.03)])
def test_every_stage_count_on_ragged_calls(ya, shape, bw):
    q, ref, src = make(ya, bw, shape, seed=int(bw * 1000))
    m = q.get_m()
    interp, ns, ra = q.get_params()
    plan = ya.plan_symstreamr(bw, m, 1)
    assert ns == STAGES[bw] == plan.stages and ra == plan.rate_arb and interp == plan.interp
    assert q.is_fused()
    assert interp == (1 if bw < 0.5 else 0)
    calls, T, g = ragged(ya, bw, m)
    for n in calls:
        assert same(q.write_samples(n), ref.write_samples(n)), (bw, n)
        assert q.get_pending() == ref.fifo.size <= 2 * g
        check_source(q, ref, src)
    if ns:                                                   # a call shorter than the leftover: nothing is pushed
        assert 0 < q.get_pending()
        state = q.source_get_state()
        n = min(q.get_pending(), 3)
        assert same(q.write_samples(n), ref.write_samples(n)) and q.source_get_state() == state
    for _ in range(40):
        assert same(q.write_samples(1), ref.write_samples(1)), bw
        check_source(q, ref, src)


@pytest.mark.parametrize("bw", [0.77, 0.4, 0.2, 0.03])
def test_cut_invariance(ya, bw):
    """one call of N samples equals the same N samples of the ragged sequence"""
    calls, T, g = ragged(ya, bw, 7)
    calls += [1] * 40
    q, ref, src = make(ya, bw, seed=5)
    whole = q.write_samples(sum(calls))
    q2, _, _ = make(ya, bw, seed=5)
    parts = np.concatenate([q2.write_samples(n) for n in calls])
    assert same(whole, parts)
    assert q.source_get_state() == q2.source_get_state() and q.get_pending() == q2.get_pending()
    assert same(whole, ref.write_samples(sum(calls)))
    check_source(q, ref, src)


def test_a_workgroup_stages_several_tiles(ya):
    """the smallest call that gives a workgroup more than one tile (one LFSR jump for all of them), with a ragged end"""
    bw, m = 0.4, 7
    T = ya.plan_symstreamr(bw, m, 1).tile
    n = 1
    while ya.plan_symstreamr(bw, m, n * T + 77).wg_tiles < 2:
        n += 1
    n = n * T + 77
    assert ya.plan_symstreamr(bw, m, (n - 77) - T).wg_tiles == 1 and ya.plan_symstreamr(bw, m, 1).max_wg_tiles >= 2
    q, ref, src = make(ya, bw, seed=9)
    assert same(q.write_samples(3), ref.write_samples(3))    # from inside a symbol, phase off zero
    assert same(q.write_samples(n), ref.write_samples(n))
    assert same(q.write_samples(1337), ref.write_samples(1337))
    check_source(q, ref, src)


@pytest.mark.parametrize("bw", [0.4, 0.03])
def test_gain_scheme_reset_and_clone(ya, bw):
    S = ya.ModulationScheme
    q, ref, src = make(ya, bw, seed=3)
    assert same(q.write_samples(1), ref.write_samples(1))
    q.set_gain(0.0)                                          # the delay test's move: reaches later symbols only
    ref.set_gain(0.0)
    assert same(q.write_samples(300), ref.write_samples(300))
    q.set_gain(0.7)
    ref.set_gain(0.7)
    assert q.get_gain() == np.float32(0.7)
    assert same(q.write_samples(501), ref.write_samples(501))
    q.set_scheme(S.Qam16)
    ref.set_scheme(S.Qam16)
    assert q.get_scheme() == S.Qam16 and q.is_fused()
    assert same(q.write_samples(777), ref.write_samples(777))
    check_source(q, ref, src)
    # clone mid-stream, a non-empty leftover included where the shape has one: the assertion symstreamr.rs:356-358 disables
    if bw == 0.03:
        assert q.get_pending() > 0
    c = q.clone()
    assert c.get_pending() == q.get_pending() and c.source_get_state() == q.source_get_state()
    a, b = q.write_samples(1337), c.write_samples(1337)
    assert same(a, b) and same(a, ref.write_samples(1337))
    # reset: the source stays; the block equals a fresh object fed from the same source state
    q.reset()
    assert q.get_pending() == 0
    fresh_src = ya.MSequence(*golden_generator(23))
    fresh_src.set_state(q.source_get_state())
    F = ya.FirFilterShape
    fresh = ya.SymStreamR(F.Arkaiser, bw, 7, 0.3, S.Qam16, fresh_src)
    fresh.set_gain(0.7)
    assert same(q.write_samples(2000), fresh.write_samples(2000))
    assert q.source_get_state() == fresh.source_get_state()


@pytest.mark.parametrize("bw", [0.77, 0.2])
@pytest.mark.parametrize("route", ["Dpsk4", "set_modem"])
def test_fallback_routes(ya, bw, route):
    S = ya.ModulationScheme
    if route == "Dpsk4":
        q, ref, src = make(ya, bw, seed=4, scheme=S.Dpsk4)
    else:
        q, ref, src = make(ya, bw, seed=4)
        md = ya.Modem(S.Dpsk8)                               # a modem the fused path does not take
        q.set_modem(md)
        ref.set_modem(md)
    assert not q.is_fused()
    calls, T, g = ragged(ya, bw, 7)
    for n in calls[:3] + [calls[4] + 1] + [1] * 5 + [1337]:
        assert same(q.write_samples(n), ref.write_samples(n)), (bw, route, n)
        check_source(q, ref, src)
    c = q.clone()
    assert same(q.write_samples(500), c.write_samples(500))


def test_set_modem_table_the_fused_path_takes(ya):
    rng = np.random.default_rng(11)
    table = (rng.standard_normal(32) + 1j * rng.standard_normal(32)).astype(np.complex64)
    md = ya.Modem.from_table(table)
    q, ref, src = make(ya, 0.2, seed=6)
    assert same(q.write_samples(100), ref.write_samples(100))
    q.set_modem(md)
    ref.set_modem(md)
    assert q.is_fused() and q.get_scheme() == ya.ModulationScheme.Arb
    for n in (1337, 1, 2500):
        assert same(q.write_samples(n), ref.write_samples(n))
        check_source(q, ref, src)


def test_getters(ya):
    S, F = ya.ModulationScheme, ya.FirFilterShape
    for bw in BWS:
        q, ref, _ = make(ya, bw)
        rate = np.float32(0.5) / np.float32(bw)
        assert q.get_bw() == np.float32(1.0) / (rate * np.float32(2.0))
        assert q.get_delay() == (np.float32(2 * 7) + ref.R.get_delay()) * rate
        assert (q.get_ftype(), q.get_m(), q.get_beta(), q.get_scheme()) == (F.Arkaiser, 7, np.float32(0.3), S.Qpsk)


# ---- the reference's own tests, at their own tolerances ----------------------------------------------------------------
DELAY_CASES = [(0.5, m) for m in (4, 5, 6, 7, 8, 9, 10, 14, 20, 31)] + \
              [(bw, 12) for bw in (0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.05, 0.025)]


@pytest.mark.parametrize("bw,m", DELAY_CASES)
def test_reference_delay_cases(ya, bw, m):
    """testbench_symstreamrcf_delay (symstreamr.rs:140-260): one sample, gain 0, the rest; the phase slope across the
    pass-band gives the delay within 0.05"""
    S, F = ya.ModulationScheme, ya.FirFilterShape
    q = ya.SymStreamR(F.Arkaiser, bw, m, 0.30, S.Qpsk, ya.MSequence(*golden_generator(23)))
    delay = q.get_delay()
    nfft = 2 * (120 + int(np.float32(delay) / np.sqrt(np.float32(bw))))
    first = q.write_samples(1)
    q.set_gain(0.0)
    x = np.concatenate([first, q.write_samples(nfft - 1)])
    X = np.fft.fft(x.astype(np.complex128))
    mm = int(np.float32(0.4) * np.float32(bw) * np.float32(nfft))
    p = 0j
    for i in range(-mm, mm):
        p += X[(nfft + i) % nfft] * np.conj(X[(nfft + i + 1) % nfft])
    meas = np.angle(p) * nfft / (2 * np.pi)
    print(f"bw {bw} m {m}: expected delay {delay:.6f}, measured {meas:.6f}, err {delay - meas:.6f}")
    assert abs(delay - meas) <= 0.05


@pytest.mark.parametrize("bw,m,beta", [(0.2, 12, 0.30), (0.4, 12, 0.30), (0.4, 25, 0.20), (0.7, 11, 0.35)])
def test_reference_psd_cases(ya, bw, m, beta):
    """testbench_symstreamrcf_psd (symstreamr.rs:262-326): gain sqrt(bw), 192000 / bw samples in calls of 1337 into
    Spgram.default(2400); at most -55 dB outside +-0.5 (1 + beta) bw, within +-2 dB inside +-0.5 (1 - beta) bw"""
    S, F = ya.ModulationScheme, ya.FirFilterShape
    q = ya.SymStreamR(F.Arkaiser, bw, m, beta, S.Qpsk, ya.MSequence(*golden_generator(23)))
    q.set_gain(np.sqrt(np.float32(bw)))
    sp = ya.Spgram.default(2400)
    buf = ya.DeviceArray(1337, np.complex64)
    n, total = 0, int(np.float32(192000.0) / np.float32(bw))
    while n < total:
        q.write_samples_devptr(buf, 1337)
        sp.write_dev(buf, 1337)
        n += 1337
    psd = sp.get_psd()
    f0, f1 = np.float32(0.5 * (1.0 - beta) * bw), np.float32(0.5 * (1.0 + beta) * bw)
    regions = [(-0.5, -f1, 0.0, -55.0, False, True), (-f0, f0, -2.0, 2.0, True, True), (f1, 0.5, 0.0, -55.0, False, True)]
    f = np.arange(2400, dtype=np.float32) / np.float32(2400) - np.float32(0.5)
    print(f"bw {bw} m {m} beta {beta}: passband {psd[(f >= -f0) & (f <= f0)].min():+.3f} .. "
          f"{psd[(f >= -f0) & (f <= f0)].max():+.3f} dB, stopband max {psd[(f <= -f1) | (f >= f1)].max():.2f} dB")
    assert validate_psd_spectrum(psd, 2400, regions)


@pytest.mark.parametrize("r", [0.127115323, 0.373737373, 0.676543210])
def test_reference_msresamp_mask_with_symstreamr_as_the_source(ya, r, as_=60.0):
    """testbench_msresamp_crcf (msresamp.rs:180-228) with the source the reference has: SymStreamR(Kaiser, r bw, 25,
    0.2, Qpsk) at gain sqrt(bw) through MsResamp(r, 60) into Spgram(800, Hann, 400, 200) until 800 000 samples: within
    +-0.5 dB inside +-0.4 bw, below -60 + 0.5 dB beyond +-0.6 bw.  Blocks of 2^18 on the device instead of 256."""
    S, F = ya.ModulationScheme, ya.FirFilterShape
    bw, tol, n_out, nfft, blk = np.float32(0.2), 0.5, 800000, 800, 1 << 18
    r = np.float32(r)
    gen = ya.SymStreamR(F.Kaiser, r * bw, 25, 0.2, S.Qpsk, ya.MSequence(*golden_generator(23)))
    gen.set_gain(np.sqrt(bw))
    rs = ya.MsResamp("crcf", r, as_)
    sp = ya.Spgram(nfft, ya.WindowType.Hann, nfft // 2, nfft // 4)
    b0, b1 = ya.DeviceArray(blk, np.complex64), ya.DeviceArray(blk, np.complex64)
    while sp.get_num_samples_total() < n_out:
        gen.write_samples_devptr(b0, blk)
        nw = rs.execute_dev(b0, blk, b1, blk)
        sp.write_dev(b1, nw)
    psd = np.asarray(sp.get_psd(), np.float32)
    regions = [(-0.5, -0.6 * bw, 0.0, -as_ + tol, False, True), (-0.4 * bw, 0.4 * bw, -tol, tol, True, True),
               (0.6 * bw, 0.5, 0.0, -as_ + tol, False, True)]
    f = np.arange(nfft, dtype=np.float32) / np.float32(nfft) - np.float32(0.5)
    inb, out = np.abs(f) <= np.float32(0.4) * bw, np.abs(f) >= np.float32(0.6) * bw
    print(f"r {r}: passband {psd[inb].min():+.3f} .. {psd[inb].max():+.3f} dB, stopband max {psd[out].max():.2f} dB")
    assert validate_psd_spectrum(psd, nfft, regions)
