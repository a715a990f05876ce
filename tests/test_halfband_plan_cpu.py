"""The plan queries of the half-band resamplers (yagi_hip_plan_msresamp2 / _resamp2) against tests/halfband_shapes.py,
on the CPU: no device is needed.

  * every row of the table has the key the library reports for its shape;
  * a sweep of the queries meets no key that the table lacks, for any sample type; a key of the universe that no shape
    reaches is listed below with the reason;
  * the planner's invariants hold over the sweep (the fast kernel's tiles lie inside the call's input and outputs);
  * the integer prototypes and samples every GPU row will use keep the whole chain exact in f32.

Sweep: 1 .. 5 stages, every m in 2 .. 1024 in one stage beside small ones and in all stages at once, both sample sizes,
n on both sides of the fast kernel's threshold for each head_tiles and of the tile counts 8192, 16384 and 32768."""
import numpy as np
import pytest

import halfband_shapes as hs

KINDS = ("rrrf", "crcf", "cccf")
SMALL = (2, 3)
N_FAST = [1, 257] + [256 * h + hs.ROOM + d for h in (1, 2, 3, 4) for d in (0, 1)]
N_TPW = [t * 256 + d for t in (8191, 16383, 32767) for d in (0, 17)]

# Keys of the universe that no shape reaches, with the reason.
UNREACHABLE = {}
for _h in (1, 2, 3, 4):
    UNREACHABLE[hs.F(1, "R2", _h)] = "one stage runs four outputs per lane"
    UNREACHABLE[hs.F(3, "R2", _h)] = "three stages run four outputs per lane at the full rate"
    for _w in ("R4/RHO0", "R4/RHO0/Q1", "R4/RHO2", "R4/RHO2/Q1"):
        UNREACHABLE[hs.F(2, _w, _h)] = "two stages run two outputs per lane at the full rate"
    if _h > 1:
        # a tile's halo is U = 2 (2 m1 - 1) + 2 m0 - 1 input pairs with 2 F + U <= 512 and F >= 64: U <= 384, so the first
        # output whose halo lies inside the block is at most 192; at three stages 4 F + U <= 1024: U <= 768, again 192
        UNREACHABLE[hs.F(2, "R2", _h)] = "a geometry with F >= 64 has a halo of at most 192 outputs"
        for _w in ("R4/RHO0", "R4/RHO0/Q1", "R4/RHO2", "R4/RHO2/Q1"):
            UNREACHABLE[hs.F(3, _w, _h)] = "a geometry with F >= 64 has a halo of at most 192 outputs"
        for _w in ("R4/RHO0/Q1", "R4/RHO2/Q1"):
            UNREACHABLE[hs.F(1, _w, _h)] = "Q = 1 is m = 2, 3: a halo of 3 or 5 outputs"
# Keys the sweep meets for a sample size that the table leaves to the other one.
NO_ROW = {(8, hs.G8): "32768 tiles of four stages are 2^27 complex samples, a gigabyte; the rrrf row runs the same kernel"}
# Rows the issue names or that mark a threshold.
NAMED = [
    ("decim", ((3, 5, 10), 236800)), ("decim", ((3, 5, 10), 236801)), ("decim", ((3, 5, 10), 237031)),
    ("decim", ((2,), 236801)), ("decim", ((128,), 236801)), ("decim", ((129,), 237057)), ("decim", ((480,), 237569)),
    ("decim", ((481,), 237569)), ("decim", ((64, 64), 236801)), ("decim", ((65, 65), 236801)),
    ("decim", ((55, 55, 55), 236801)), ("decim", ((56, 56, 56), 236801)),
    ("decim", (hs.T4, 8190 * 256 + 17)), ("decim", (hs.T4, 8191 * 256 + 17)), ("decim", (hs.T4, 16383 * 256 + 17)),
    ("decim", (hs.T4, 32767 * 256 + 17)), ("decim", ((2, 2, 3, 3, 4), 1 << 15)),
    ("resamp2", (64, (1 << 19) - 2)), ("resamp2", (64, 1 << 19)), ("resamp2", (65, 1 << 19)),
]
# uniform m, last that fits the fused chain's 64 KiB (decimator, interpolator); None: every m fits
LDS_BOUND = {(4, 8): (5, 21), (4, 4): (84, 355), (3, 8): (105, 271), (3, 4): (291, 753), (2, 8): (416, 665), (2, 4): (928, None)}


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def universe():
    keys = [("decim", "general", t) for t in (1, 2, 4, 8)]
    keys += [hs.F(S, w, h) for S in (1, 2, 3) for w in ("R2", "R4/RHO0", "R4/RHO0/Q1", "R4/RHO2", "R4/RHO2/Q1") for h in (1, 2, 3, 4)]
    keys += [("decim", "chain"), ("interp", "chain"), ("interp", "fused"), ("decim", "chain", 5), ("interp", "chain", 5)]
    keys += [("resamp2", "kernel"), ("resamp2", "chain")]
    return keys


def sweep_shapes():
    """(family, ms in processing order, n list)"""
    for ns in range(1, 6):
        for m in (range(2, 1025) if ns <= 4 else (2, 3, 64, 1024)):       # five stages never share a launch
            lines = {(m,) * ns}
            for pos in range(ns):
                for small in SMALL:
                    lines.add(tuple(m if k == pos else small for k in range(ns)))
            for ms in sorted(lines):
                yield "decim", ms, N_FAST if ns <= 3 else (1, 257, N_FAST[-1])      # the fast kernel has at most three stages
                yield "interp", ms, (1, 257)
    for ms in ((2,), (3, 5), (2, 3, 3), hs.T4, (5,) * 4, (84,) * 4, (2, 2, 3, 3, 4)):
        yield "decim", ms, N_TPW


def check_invariants(p, family, ms, n, elem):
    S = len(ms)
    assert p.lds <= 64 << 10 and p.tpw in (1, 2, 4, 8)
    if family == "interp":
        assert p.tiles == (n + 255) // 256
        return
    halo = 0                                                                    # stage-0 pairs before a tile's own 256 << (S - 1)
    for m in reversed(ms):
        halo = 2 * halo + 2 * m - 1
    assert p.long_halo == int(halo > 256)
    assert p.tiles == p.head_tiles + max(0, n - p.tail_first + 255) // 256 and p.tpw == next(
        t for t in (1, 2, 4, 8) if t == 8 or p.tiles // (2 * t) < 4096)
    if p.F:
        R0 = 4 if S == 1 else 1 << (S - 1)
        assert 64 <= p.F and p.n[S - 1] == p.F and p.cnt0 <= 256 * R0 and p.cnt0 == p.n[0] + 2 * ms[0] - 1
        for k in range(S):
            R = (4 if S == 1 else 1) << (S - 1 - k)
            rho = 2 * ms[k] % R if R == 4 else 0
            assert p.walk[k] == {1: 1, 2: 2, 4: 3 + rho // 2}[R] and R * p.walk_q[k] + rho == 2 * ms[k]
            assert (p.n[k] + R - 1) // R <= 256                                  # a lane per R outputs
    if p.fast_tiles:
        assert S <= 3 and p.F and p.fast_tpw == (1 if S == 1 else 2) and p.fast_lds <= 64 << 10
        assert 256 * p.head_tiles + p.F * p.fast_tiles == p.tail_first <= n - 1
        assert n - p.tail_first <= p.F                                          # the tail: 1 .. F outputs
        assert (256 * p.head_tiles << (S - 1)) - p.U >= 0                        # the first fast tile's halo lies inside the block
        last = ((256 * p.head_tiles + (p.fast_tiles - 1) * p.F) << (S - 1)) - p.U
        assert last + p.cnt0 <= n << (S - 1)                                    # and so does the last one's input
        assert n - 1 - 256 * p.head_tiles >= hs.ROOM
    else:
        assert p.head_tiles == (n + 255) // 256 and p.tail_first == 256 * p.head_tiles
        if p.F:                                                                 # a geometry, but the block is too short
            P2 = 1 << (S - 1)
            head = ((p.U + P2 - 1) // P2 + 255) // 256
            assert n - 1 - 256 * head < hs.ROOM


@pytest.fixture(scope="module")
def sweep(ya):
    """smallest[(elem, key)] = the shortest call with that key; the invariants are checked on the way"""
    smallest = {}
    for elem in (4, 8):
        for family, ms, ns_ in sweep_shapes():
            for n in ns_:
                p = hs.plan_ms(ya, elem, family, ms, n)
                key = hs.ms_key(p, family == "interp", len(ms))
                if p.fused:
                    check_invariants(p, family, ms, n, elem)
                smallest[(elem, key)] = min(n, smallest.get((elem, key), 1 << 62))
        for m in range(2, 1025):
            for nx in (2, (1 << 19) - 2, 1 << 19, (1 << 19) + 2, 1 << 22):
                p = ya.plan_resamp2(elem, hs.DECIM_MODE, m, nx)
                assert p.chain == int(nx >= 1 << 19 and m <= 64)
                key = ("resamp2", "chain" if p.chain else "kernel")
                one = ya.plan_msresamp2(elem, False, [m], nx // 2)
                assert p.lds == (one.lds if p.chain else 2 * (1024 + 2 * m) * elem)
                assert p.tiles == (one.tiles if p.chain else (nx // 2 + 1023) // 1024)
                smallest[(elem, key)] = min(nx, smallest.get((elem, key), 1 << 62))
    return smallest


def test_queries_need_no_device_and_reject_bad_arguments(ya):
    p = ya.plan_msresamp2(8, False, [10, 5, 3], 236801)           # object order: the full-rate stage is m = 3
    assert (p.fused, p.F, p.n, p.cnt0, p.U, p.head_tiles, p.fast_tiles, p.tail_first, p.tiles, p.tpw, p.fast_tpw) == (
        1, 231, (1018, 500, 231), 1023, 99, 1, 1024, 236800, 2, 1, 2)
    assert p.walk == (ya.PLAN_WALK_R4_RHO2, ya.PLAN_WALK_R2, ya.PLAN_WALK_R1, 0) and p.walk_q == (1, 5, 20, 0)
    assert ya.plan_msresamp2(8, False, [3, 5, 10], 236801).walk[0] == ya.PLAN_WALK_R4_RHO0       # the order matters
    q = ya.plan_msresamp2(8, True, [21] * 4, 1000)
    assert (q.fused, q.tiles, q.lds) == (1, 4, 65488) and ya.plan_msresamp2(8, True, [22] * 4, 1000).fused == 0
    assert ya.plan_msresamp2(4, False, [2] * 5, 100) == ya.MsResamp2Plan(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, (0, 0, 0), 0, 0, (0,) * 4, (0,) * 4, 0)
    assert ya.plan_resamp2(8, 3, 64, 1 << 19) == ya.Resamp2Plan(1, 5, 6128)
    assert ya.plan_resamp2(4, 4, 7, 1000) == ya.Resamp2Plan(0, 1, 2 * (1024 + 14) * 4)           # other forms: resamp2_kernel
    for bad in (lambda: ya.plan_msresamp2(3, False, [2], 10), lambda: ya.plan_msresamp2(4, False, [], 10),
                lambda: ya.plan_msresamp2(4, False, [2] * 17, 10), lambda: ya.plan_msresamp2(4, False, [1], 10),
                lambda: ya.plan_msresamp2(4, True, [2, 1025], 10), lambda: ya.plan_msresamp2(4, False, [2], 0),
                lambda: ya.plan_resamp2(16, 3, 4, 8), lambda: ya.plan_resamp2(4, 5, 4, 8), lambda: ya.plan_resamp2(4, 3, 1, 8),
                lambda: ya.plan_resamp2(4, 3, 4, 7), lambda: ya.plan_resamp2(4, 3, 4, 0)):
        with pytest.raises(ya.ConfigError):
            bad()
    assert ya.lib.yagi_hip_plan_msresamp2(4, 0, 1, None, 10, None) == 2       # YAGI_ERR_CONFIG: null pointers
    assert ya.lib.yagi_hip_plan_resamp2(4, 3, 4, 8, None) == 2


@pytest.mark.parametrize("row,kind", hs.cases(), ids=[hs.case_id(r, k) for r, k in hs.cases()])
def test_row_has_the_key_the_library_reports(ya, row, kind):
    key, p = hs.query(ya, row, kind)
    assert key == row.key, (row.shape, kind, p)


def test_rows_state_what_the_planner_gives(ya):
    """the figures the table's comments rest on"""
    def plan(ms, n, elem=8):
        return hs.plan_ms(ya, elem, "decim", ms, n)
    p = plan((3, 5, 10), 236800)
    assert (p.fast_tiles, p.tiles, p.F, p.U) == (0, 925, 231, 99)
    p = plan((3, 5, 10), 236801)
    assert (p.fast_tiles, 236801 - p.tail_first, p.head_tiles) == (1024, 1, 1)
    p = plan((3, 5, 10), 237031)
    assert (p.fast_tiles, 237031 - p.tail_first) == (1024, 231)
    assert plan((3, 5, 10), 237032).fast_tiles == 1025
    assert [plan((2,), n).fast_tiles for n in (236801, 236801 + 1021)] == [231, 232] and plan((2,), 236801).F == 1021
    assert [plan(ms, 236801).fast_tiles for ms in ((2, 3), (3, 2), (2, 2, 3), (3, 3, 2), (3, 2, 2))] == [949, 946, 953, 949, 946]
    assert [(plan((m,), 300000).head_tiles, plan((m,), 300000).F) for m in (128, 129, 256, 257, 384, 385, 480)] == [
        (1, 769), (2, 767), (2, 513), (3, 511), (3, 257), (4, 255), (4, 65)]
    assert plan((481,), 300000).F == 0 and plan((64, 64), 300000).F == 65 and plan((65, 65), 300000).F == 0
    assert plan((55,) * 3, 300000).F == 65 and plan((56,) * 3, 300000).F == 0
    assert plan(hs.T4, 1000).lds == 63968 and plan(hs.T4, 1000, 4).lds == 31984
    assert [plan(ms, 1000).long_halo for ms in ((128,), (129,), (43, 43), (44, 44), (18,) * 3, (19,) * 3, (10, 5, 3))] == [0, 1, 0, 1, 0, 1, 0]
    assert [(plan(hs.T4, t * 256 - 239).tiles, plan(hs.T4, t * 256 - 239).tpw) for t in (8191, 8192, 16383, 16384, 32767, 32768)] == [
        (8191, 1), (8192, 2), (16383, 2), (16384, 4), (32767, 4), (32768, 8)]
    for (ns, elem), (dlast, ilast) in LDS_BOUND.items():
        assert plan((dlast,) * ns, 600, elem).fused == 1 and plan((dlast + 1,) * ns, 600, elem).fused == 0
        if ilast is None:
            assert hs.plan_ms(ya, elem, "interp", (1024,) * ns, 300).fused == 1
        else:
            assert hs.plan_ms(ya, elem, "interp", (ilast,) * ns, 300).fused == 1
            assert hs.plan_ms(ya, elem, "interp", (ilast + 1,) * ns, 300).fused == 0


def test_table_covers_every_key_of_the_sweep(ya, sweep):
    have = {(kind, row.key) for row, kind in hs.cases()}
    missing = [f"{kind} {key}: no row (the sweep's shortest call: {n})" for (elem, key), n in sorted(sweep.items(), key=str)
               for kind in KINDS if hs.ELEM[kind] == elem and (kind, key) not in have and (elem, key) not in NO_ROW]
    assert not missing, "\n".join(missing)
    assert all(k in sweep for k in NO_ROW)
    # every key of the universe is met by the sweep or listed as unreachable -- and only one of the two
    met = {key for (_, key) in sweep}
    for key in universe():
        assert (key in met) != (key in UNREACHABLE), (key, key in met)
    assert met <= set(universe()), met - set(universe())
    for row in hs.TABLE:
        assert row.key not in UNREACHABLE and row.key in met, row
    absent = [n for n in NAMED if not any(r.family == n[0] and r.shape == n[1] for r in hs.TABLE)]
    assert not absent, absent


def test_table_has_both_sides_of_every_threshold(ya):
    rows = {}
    for r, k in hs.cases():
        rows[(r.family, k, r.shape)] = r.key
    missing = []
    for kind in KINDS:
        elem = hs.ELEM[kind]
        for (ns, e), bounds in LDS_BOUND.items():
            if e != elem:
                continue
            for family, last in zip(("decim", "interp"), bounds):
                n = 600 if family == "decim" else 300
                if last is None:
                    continue
                a, b = rows.get((family, kind, ((last,) * ns, n))), rows.get((family, kind, ((last + 1,) * ns, n)))
                if a is None or b is None or a[1] == "chain" or b[1] != "chain":
                    missing.append(f"{kind} {family} LDS bound at {ns} stages: m {last} | {last + 1}")
        pairs = [(((3, 5, 10), 256 + hs.ROOM), ((3, 5, 10), 257 + hs.ROOM)), ((hs.T4, 8190 * 256 + 17), (hs.T4, 8191 * 256 + 17)),
                 (((128,), 257 + hs.ROOM), ((129,), 513 + hs.ROOM)), (((480,), 1025 + hs.ROOM), ((481,), 1025 + hs.ROOM)),
                 (((64, 64), 257 + hs.ROOM), ((65, 65), 257 + hs.ROOM)), (((55,) * 3, 257 + hs.ROOM), ((56,) * 3, 257 + hs.ROOM))]
        for a, b in pairs:
            ka, kb = rows.get(("decim", kind, a)), rows.get(("decim", kind, b))
            if ka is None or kb is None or ka == kb:
                missing.append(f"{kind} decim {a} | {b}: {ka} | {kb}")
        for a, b in (((64, (1 << 19) - 2), (64, 1 << 19)), ((65, 1 << 19), (64, 1 << 19))):
            if (rows.get(("resamp2", kind, a)), rows.get(("resamp2", kind, b))) != (("resamp2", "kernel"), ("resamp2", "chain")):
                missing.append(f"{kind} resamp2 {a} | {b}")
    assert not missing, "\n".join(missing)


@pytest.mark.parametrize("row", hs.TABLE, ids=[hs.case_id(r, "any") for r in hs.TABLE])
def test_row_is_exact_in_f32(row):
    """max|x| prod_k (1 + sum|h1_k|) <= 2^24 for the prototypes the GPU row uses, whose first and last branch taps are
    non-zero; the prototypes are a function of the row alone"""
    hfs = hs.prototypes(row)
    ms = hs.row_stages(row)
    assert [len(hf) for hf in hfs] == [4 * m + 1 for m in ms]
    assert hs.exactness_bound(hfs) <= 1 << 24
    for hf in hfs:
        assert hf[1] != 0 and hf[-2] != 0 and np.array_equal(hf, np.round(hf)) and np.max(np.abs(hf)) <= 3
    assert all(np.array_equal(a, b) for a, b in zip(hfs, hs.prototypes(row)))
    x = hs.int_stream(np.random.default_rng(1), "cccf", 4096)
    assert max(np.max(np.abs(x.real)), np.max(np.abs(x.imag))) <= hs.MAX_SAMPLE
