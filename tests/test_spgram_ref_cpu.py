"""tests/spgram_ref.py and tests/spgram_shapes.py on the CPU (no device): the f64 reference against the oracle's
per-sample restatement, the sharpness of every case of the shape table, and the plan query.

Sharpness: for every case of the table (row, sample type, mode) the row's sparse stream is built and each mutation is
applied to the f64 reference at each live frame of interest -- the frame displaced by one sample, dropped, counted twice
and, in recursive mode, its weight swapped with its neighbour's (spgram_shapes.SWAP_MIN_ALPHA says where).  Every one
must move the estimate by at least MUTATION_FACTOR * TOL in rel-L2, TOL being the cap test_gpu_spgram_shapes.py puts on
the device's error: an error of that kind in one frame cannot hide under the tolerance."""
import numpy as np
import pytest

import spgram_ref as sr
import spgram_shapes as ss
from gpu_util import rel_l2


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def dense(dt, n, seed):
    rng = np.random.default_rng(seed)
    if dt is np.float32:
        return rng.standard_normal(n).astype(np.float32)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)).astype(np.complex64)


def drive_oracle(oracle, g, dt, x, ops):
    q = oracle.Spgram(g.nfft, g.wtype, g.wlen, g.delay, dtype=dt)
    pos = 0
    for op in ops:
        if op[0] in sr.WRITES:
            q.write(x[pos:pos + op[1]])
            pos += op[1]
        elif op[0] == "set_alpha":
            q.set_alpha(op[1])
        else:
            getattr(q, op[0])()
    return q


# (nfft, wlen, delay, taper), operations
SMALL = [
    ((16, 16, 4, 1), [("write", 100)]),                                          # wlen = nfft, delay < wlen
    ((32, 12, 12, 1), [("write", 5), ("write", 90)]),                            # wlen < nfft, delay = wlen
    ((32, 12, 19, 1), [("write", 7), ("write", 3), ("write", 200)]),             # wlen < delay < nfft; short writes
    ((16, 10, 23, 2), [("write", 22), ("write", 1), ("write", 150)]),            # delay > nfft; a write one short of the timer
    ((8, 1, 3, 7), [("write", 40)]),                                             # wlen = 1 (Triangular)
    ((2, 2, 1, 1), [("write", 33)]),
    ((24, 10, 3, 1), [("write", 50), ("clear",), ("write", 2), ("write", 61)]),  # clear: the buffer survives
    ((24, 10, 3, 1), [("write", 50), ("reset",), ("write", 61)]),                # reset: it does not
    ((24, 10, 3, 1), [("write", 4), ("clear",), ("write", 4), ("clear",), ("write", 30)]),
    ((20, 20, 7, 6), [("set_alpha", 0.25), ("write", 80), ("set_alpha", -1.0), ("write", 70),
                      ("set_alpha", 0.0625), ("write", 90), ("set_alpha", -1.0)]),        # both directions
    ((20, 9, 5, 8), [("set_alpha", 0.1), ("write", 60), ("clear",), ("write", 44), ("set_alpha", -1.0)]),
    ((20, 9, 5, 1), [("set_alpha", 0.1), ("write", 60)]),                        # still averaging: the linear scale is 0
    ((12, 6, 50, 1), [("write", 20)]),                                           # no transform at all
]


@pytest.mark.parametrize("dt", [np.complex64, np.float32], ids=["cf", "f"])
@pytest.mark.parametrize("i", range(len(SMALL)))
def test_reference_vs_oracle(oracle, i, dt):
    """the index arithmetic against oracle.Spgram, which pushes sample by sample: model_f32 restates the oracle's
    rounding, so it gives the oracle's bits; the f64 estimate agrees to f32 rounding (2e-6 in rel-L2: at most 200
    transforms of at most 32 points, each |X|^2 good to a few eps = 6e-8); the counters are the oracle's"""
    geo, ops = SMALL[i]
    g = sr.Geometry(*geo)
    n = sum(op[1] for op in ops if op[0] in sr.WRITES)
    s0 = sr.schedule(g, ops)
    live = range(s0.live0, len(s0.end))
    streams = [dense(dt, n, 100 + i)]
    if len(live):
        streams.append(sr.sparse_stream(dt, g, [live[0], live[len(live) // 2], live[-1]], 200 + i, ops=ops))
    for x in streams:
        q = drive_oracle(oracle, g, dt, x, ops)
        w = sr.taper(oracle, g)
        truth, s = sr.spgram_ref(g, w, x, ops)
        assert (s.num_samples, s.num_samples_total, s.num_transforms, s.num_transforms_total) == \
               (q.num_samples, q.num_samples_total, q.num_transforms, q.num_transforms_total)
        assert len(s.end) - s.live0 == q.num_transforms
        want = q.get_psd_mag()
        assert np.array_equal(sr.model_f32(g, w, x, ops), want)
        assert rel_l2(want, truth) <= 2e-6, rel_l2(want, truth)
        if s.accumulate and s.num_transforms:
            assert np.max(truth) > 1e-6                                          # the estimate is not just the floor


def test_mutations_of_the_small_reference():
    """what a mutation means, on a stream short enough to count by hand: frames of 2 samples every 3, rectangular"""
    g = sr.Geometry(4, 2, 3, 1)
    w = np.ones(2, np.float32)
    x = np.arange(1, 10, dtype=np.float32)                          # frames (2, 3), (5, 6), (8, 9)
    ops = [("write", 9)]
    dc = lambda p: p[2] * 3                                         # bin 0 sits at index nfft / 2; undo the 1 / 3
    base, s = sr.spgram_ref(g, w, x, ops)
    assert list(s.end) == [2, 5, 8] and dc(base) == pytest.approx(5 ** 2 + 11 ** 2 + 17 ** 2)
    assert dc(sr.spgram_ref(g, w, x, ops, ("shift", 1))[0]) == pytest.approx(5 ** 2 + 13 ** 2 + 17 ** 2)
    assert dc(sr.spgram_ref(g, w, x, ops, ("shift", 2))[0]) == pytest.approx(5 ** 2 + 11 ** 2 + 9 ** 2)   # past the end: 0
    assert dc(sr.spgram_ref(g, w, x, ops, ("drop", 0))[0]) == pytest.approx(11 ** 2 + 17 ** 2)
    assert dc(sr.spgram_ref(g, w, x, ops, ("twice", 2))[0]) == pytest.approx(5 ** 2 + 11 ** 2 + 2 * 17 ** 2)
    rec = [("set_alpha", 0.25), ("write", 9), ("set_alpha", -1.0)]
    assert dc(sr.spgram_ref(g, w, x, rec)[0]) == pytest.approx(0.75 ** 2 * 25 + 0.25 * 0.75 * 121 + 0.25 * 289)
    assert dc(sr.spgram_ref(g, w, x, rec, ("swap", 0))[0]) == pytest.approx(0.25 * 0.75 * 25 + 0.75 ** 2 * 121 + 0.25 * 289)
    assert dc(sr.spgram_ref(g, w, x, rec, ("swap", 2))[0]) == pytest.approx(0.75 ** 2 * 25 + 0.25 * 121 + 0.25 * 0.75 * 289)


def mutations(s, j):
    """the mutations that apply to live transform j of a schedule"""
    out = ["shift", "drop", "twice"]
    nlive = len(s.end) - s.live0
    if s.gamma[j] != 1.0 and nlive >= 2 and (s.first[j] or s.alpha[j] >= ss.SWAP_MIN_ALPHA):
        out.append("swap")
    return out


@pytest.mark.parametrize("row", ss.TABLE, ids=[r.name for r in ss.TABLE])
def test_every_case_is_sharp(ya, oracle, row):
    assert ss.TOL * ss.MUTATION_FACTOR <= 3.6e-4
    n = 0
    for dt in ss.dtypes(row):
        for mode in ("ops",) if ss.fixed_modes(row) else ss.MODES:
            c = ss.build_case(ya, row, dt, mode)
            w = sr.taper(oracle, c.g)
            base, s = sr.spgram_ref(c.g, w, c.x, c.ops, sched=c.sched)
            live = [j for j in c.frames if j >= s.live0]
            last_of_calls = [f0 + k - 1 for _, f0, k in s.call_frames if k and f0 + k - 1 >= s.live0]
            assert set(last_of_calls) <= set(live) and s.live0 in live, (c.frames, s.call_frames)
            for j in live:
                for kind in mutations(s, j):
                    eff = rel_l2(sr.spgram_ref(c.g, w, c.x, c.ops, (kind, j), sched=s)[0], base)
                    assert eff >= ss.MUTATION_FACTOR * ss.TOL, (ss.case_id(row, dt, mode), kind, j, eff)
                    n += 1
            if mode == "rec":
                assert "swap" in mutations(s, s.live0) or len(s.end) - s.live0 < 2
                assert s.gamma[-1] ** len(s.end) > 0.1                           # every frame's weight is visible
    assert n >= 3


def test_model_f32_is_the_yardstick(ya, oracle):
    """the f32 model of the pipeline errs by f32 rounding on the table's streams, far below TOL (the recursion of the
    2^20-transform row, 2^20 roundings of psd in a row, is left to the GPU test)"""
    for row in ss.TABLE:
        if row.spec == "cut+37":
            continue
        for mode in ("ops",) if ss.fixed_modes(row) else ss.MODES:
            c = ss.build_case(ya, row, np.complex64, mode)
            w = sr.taper(oracle, c.g)
            e = rel_l2(sr.model_f32(c.g, w, c.x, c.ops), sr.spgram_ref(c.g, w, c.x, c.ops, sched=c.sched)[0])
            assert 0 < e <= ss.TOL / 4, (row.name, mode, e)


# ---- the plan query ----------------------------------------------------------------------------------------------------
def test_plan_fused_flag(ya):
    for nfft in ss.FUSED:
        p = ya.plan_spgram(nfft, 1000)
        assert p.fused == 1 and p.group == 4096 // nfft and p.accum_slab == 0 and p.launch_frames == 1 << 20, (nfft, p)
    for nfft in (2, 64, 100, 255, 257, 768, 4095, 4097, 8192, 1 << 17, 1 << 20):
        p = ya.plan_spgram(nfft, 1000)
        want = min(max((1 << 25) // nfft, 1), 8192)
        assert p.fused == 0 and p.accum_slab == 32 and p.slab == 0 and p.folded == 0 and p.launch_frames == want, (nfft, p)
        assert p.rows == -(-min(1000, want) // 32)
        assert p.workgroups == min(8192, -(-min(1000, want) * nfft // 256))


def test_plan_invariants(ya):
    """slab monotonic in the count and a multiple of the group; rows = workgroups * group; folded exactly when rows > 64;
    the launch holds every transform; beyond launch_frames the first launch is described"""
    counts = sorted(set(list(range(1, 600)) + [1024 * k + d for k in range(1, 40) for d in (-1, 0, 1)] +
                        [(1 << 20) - 1, 1 << 20, (1 << 20) + 37, 1 << 24]))
    for nfft in ss.FUSED:
        prev = 0
        for n in counts:
            p = ya.plan_spgram(nfft, n)
            m = min(n, p.launch_frames)
            assert p.slab >= prev and p.slab % p.group == 0 and 4 <= p.slab <= 32, (nfft, n, p)
            prev = p.slab
            assert p.rows == p.workgroups * p.group and p.workgroups == -(-m // p.slab), (nfft, n, p)
            assert p.folded == (1 if p.rows > 64 else 0), (nfft, n, p)
            assert p.fold_rows == (-(-p.rows // 32) if p.folded else 0), (nfft, n, p)
        assert ya.plan_spgram(nfft, (1 << 20) + 37) == ya.plan_spgram(nfft, 1 << 20)


def test_plan_bad_arguments(ya):
    for bad in (lambda: ya.plan_spgram(1, 10), lambda: ya.plan_spgram((1 << 20) + 1, 10), lambda: ya.plan_spgram(256, 0),
                lambda: ya.plan_spgram(256, 1 << 31)):
        with pytest.raises(ya.ConfigError):
            bad()
    assert ya.lib.yagi_hip_plan_spgram(256, 10, None) == 2                       # YAGI_ERR_CONFIG: null out


def test_table_keys(ya):
    """every row's key is what the query reports for the row's largest call, and the table reaches what it says"""
    names = [r.name for r in ss.TABLE]
    assert len(set(names)) == len(names)
    for row in ss.TABLE:
        c = ss.build_case(ya, row, np.complex64, "ops" if ss.fixed_modes(row) else "acc")
        p = ya.plan_spgram(row.nfft, c.main)
        assert ss.key_of(p, c.main) == row.key, (row.name, c.main, ss.key_of(p, c.main))
        assert len(c.frames) <= 8
    key = {r.name: r.key for r in ss.TABLE}
    for nfft in ss.FUSED:
        B = 4096 // nfft
        assert key[f"{nfft}-rows64"][4] == 64 and key[f"{nfft}-rows64"][5] == 0
        assert key[f"{nfft}-rows65"][4] > 64 and key[f"{nfft}-rows65"][5] > 0
        assert key[f"{nfft}-rows65"][4] - 64 <= B                                 # the very next row count
        f = key[f"{nfft}-fold_ragged"]
        assert f[5] > 4 and f[5] % 4 and f[4] % 32
        assert key[f"{nfft}-slab_above"][2] > key[f"{nfft}-one"][2]
        assert key.get(f"{nfft}-slab_cap", key[f"{nfft}-slab_above"])[2] == 32
    assert key["256-cut+37"][6] == 2 and key["64-cut+33"][3] == 2 and key["131072-cut+5"][3] == 2
    assert key["8192-stride"][1] == 8192
    c = ss.build_case(ya, [r for r in ss.TABLE if r.name == "8192-stride"][0], np.complex64, "acc")
    assert c.main * 8192 > 8192 * 256
