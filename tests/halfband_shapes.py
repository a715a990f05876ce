"""The launch plans of the half-band resamplers and the shapes that reach them (a helper, not a conftest).

What a block call of MsResamp2 and of Resamp2's decimator launches is decided on the host by the planners of
yagi_amd/csrc/resamp2_kernels.hip (msresamp2_decim_plan, msresamp2_interp_plan, resamp2_takes_chain), and the library
answers for a shape through yagi_amd.plan_msresamp2 / plan_resamp2 -- the planners the launches themselves call.  TABLE
holds, per plan key, shapes that reach it and one shape on each side of every threshold;
tests/test_halfband_plan_cpu.py checks every row's key against the query and that the table covers every key a sweep
of the queries meets, tests/test_gpu_halfband_plans.py runs every row bit for bit against the oracle's sequential loop.

Keys
  ("decim", "general", tpw)               msresamp2_decim_kernel alone, tpw = 1, 2, 4, 8 consecutive tiles per workgroup
  ("decim", "fast", S, walk0, head)       msresamp2_decim_fast_kernel<S> between `head` general tiles and a general tail;
                                          walk0 = the tap walk of the full-rate stage: "R4/RHO0" (m even), "R4/RHO2" (m odd),
                                          each with "/Q1" where the walk has no full group (m = 2, 3), or "R2" (S = 2).  At
                                          S = 3 the later stages always walk R2 and R1.
  ("decim" | "interp", "chain")           at most four stages whose streams do not fit 64 KiB: one Resamp2 call per stage
  ("decim" | "interp", "chain", ns)       more than four stages: the same
  ("interp", "fused")                     msresamp2_interp_kernel
  ("resamp2", "kernel" | "chain")         Resamp2 DECIM: resamp2_kernel, or the one-stage case of the chain kernels
Shapes
  decim / interp: (ms, n) with ms in PROCESSING order (the first entry is the stage the samples enter first: the full-rate
  stage of a decimator, i.e. stage len(ms) - 1 of the object) and n execute() calls (decim: outputs, interp: inputs);
  resamp2: (m, nx).  A GPU case runs three calls that continue one stream: the shape, then 1 output, then 5."""
import collections

import numpy as np

from gpu_util import int_samples

Row = collections.namedtuple("Row", "family kinds key shape why")

REAL, CPLX, ALL = ("rrrf",), ("crcf", "cccf"), ("rrrf", "crcf", "cccf")
ELEM = {"rrrf": 4, "crcf": 8, "cccf": 8}                      # bytes per sample
WALK = {1: "R1", 2: "R2", 3: "R4/RHO0", 4: "R4/RHO2"}
DECIM_MODE = 3                                                # Resamp2.DECIM
ROOM = 1024 * 231                                             # the fast kernel runs from this many outputs past the head on
MAX_SAMPLE = 8                                                # gpu_util.int_samples: components in -8..8

G1, G2, G4, G8 = (("decim", "general", t) for t in (1, 2, 4, 8))


def F(S, walk0, head=1):
    return ("decim", "fast", S, walk0, head)


T4 = (2, 3, 3, 4)                                             # four stages: no fast path; 63 968 bytes for complex samples

TABLE = [
    # ---- the general kernel and its tiles per workgroup ----------------------------------------------------------------
    Row("decim", ALL, G1, ((2,), 1), "shortest call"),
    Row("decim", ALL, G1, ((3, 5, 10), 300), "two tiles, the second ragged"),
    Row("decim", ALL, G1, (T4, 8190 * 256 + 17), "8191 | 8192 tiles: last with tpw 1"),
    Row("decim", ALL, G2, (T4, 8191 * 256 + 17), "8191 | 8192 tiles: first with tpw 2"),
    Row("decim", ALL, G4, (T4, 16383 * 256 + 17), "16383 | 16384 tiles: first with tpw 4"),
    Row("decim", REAL, G8, (T4, 32767 * 256 + 17), "32768 tiles, 2^27 floats in"),
    # ---- the threshold of the fast kernel ------------------------------------------------------------------------------
    Row("decim", ALL, G1, ((3, 5, 10), 256 + ROOM), "room 236543 | 236544: last without fast tiles (925 general tiles)"),
    Row("decim", ALL, F(3, "R4/RHO2/Q1"), ((3, 5, 10), 257 + ROOM), "first with fast tiles (1024), a tail of one output"),
    Row("decim", ALL, F(3, "R4/RHO2/Q1"), ((3, 5, 10), 256 + ROOM + 231), "the longest tail: F outputs"),
    Row("decim", ALL, G1, ((129,), 512 + ROOM), "head of two tiles: last without fast tiles"),
    # ---- one stage: four outputs per lane, head_tiles 1 .. 4 -----------------------------------------------------------
    Row("decim", ALL, F(1, "R4/RHO0/Q1"), ((2,), 257 + ROOM), "m 2: 231 fast tiles (odd)"),
    Row("decim", ALL, F(1, "R4/RHO0/Q1"), ((2,), 257 + ROOM + 1021), "232 fast tiles (even)"),
    Row("decim", ALL, F(1, "R4/RHO2/Q1"), ((3,), 257 + ROOM), "m 3"),
    Row("decim", ALL, F(1, "R4/RHO0"), ((4,), 257 + ROOM), "m 4: one full group"),
    Row("decim", ALL, F(1, "R4/RHO2"), ((5,), 257 + ROOM), "m 5: one full group"),
    Row("decim", ALL, F(1, "R4/RHO0"), ((64,), 257 + ROOM), "large even m"),
    Row("decim", ALL, F(1, "R4/RHO2"), ((63,), 257 + ROOM), "large odd m"),
    Row("decim", ALL, F(1, "R4/RHO0"), ((128,), 257 + ROOM), "head_tiles 1 | 2: last m with 1"),
    Row("decim", ALL, F(1, "R4/RHO2", 2), ((129,), 513 + ROOM), "head_tiles 1 | 2: first m with 2"),
    Row("decim", ALL, F(1, "R4/RHO0", 2), ((130,), 513 + ROOM), "shortest call"),
    Row("decim", ALL, F(1, "R4/RHO2", 3), ((257,), 769 + ROOM), "head_tiles 2 | 3: first m with 3"),
    Row("decim", ALL, F(1, "R4/RHO0", 3), ((258,), 769 + ROOM), "shortest call"),
    Row("decim", ALL, F(1, "R4/RHO2", 4), ((385,), 1025 + ROOM), "head_tiles 3 | 4: first m with 4"),
    Row("decim", ALL, F(1, "R4/RHO0", 4), ((386,), 1025 + ROOM), "shortest call"),
    Row("decim", ALL, F(1, "R4/RHO0", 4), ((480,), 1025 + ROOM), "the last m with a geometry (F = 65)"),
    Row("decim", ALL, G1, ((481,), 1025 + ROOM), "the first m without a geometry: general kernel only"),
    # ---- two stages: two outputs per lane at the full rate ---------------------------------------------------------------
    Row("decim", ALL, F(2, "R2"), ((2, 3), 257 + ROOM), "stage-0 m 2, 949 fast tiles (odd: a half-filled last workgroup)"),
    Row("decim", ALL, F(2, "R2"), ((3, 2), 257 + ROOM), "stage-0 m 3, 946 fast tiles (even)"),
    Row("decim", ALL, F(2, "R2"), ((64, 64), 257 + ROOM), "the last uniform m with a geometry (F = 65)"),
    Row("decim", ALL, G1, ((65, 65), 257 + ROOM), "the first uniform m without a geometry"),
    # ---- three stages: 4 / 2 / 1 outputs per lane --------------------------------------------------------------------------
    Row("decim", ALL, F(3, "R4/RHO0/Q1"), ((2, 2, 3), 257 + ROOM), "stage-0 m 2, stage-1 m 2, 953 fast tiles (odd)"),
    Row("decim", ALL, F(3, "R4/RHO2/Q1"), ((3, 3, 2), 257 + ROOM), "stage-0 m 3, stage-1 m 3, 949 fast tiles (odd)"),
    Row("decim", ALL, F(3, "R4/RHO2/Q1"), ((3, 2, 2), 257 + ROOM), "946 fast tiles (even)"),
    Row("decim", ALL, F(3, "R4/RHO0"), ((4, 5, 10), 257 + ROOM), "stage-0 m 4"),
    Row("decim", ALL, F(3, "R4/RHO2"), ((5, 3, 2), 257 + ROOM), "stage-0 m 5"),
    Row("decim", ALL, F(3, "R4/RHO0"), ((40, 3, 2), 257 + ROOM), "large even stage-0 m"),
    Row("decim", ALL, F(3, "R4/RHO2"), ((41, 3, 2), 257 + ROOM), "large odd stage-0 m"),
    Row("decim", ALL, F(3, "R4/RHO2"), ((55, 55, 55), 257 + ROOM), "the last uniform m with a geometry (F = 65)"),
    Row("decim", ALL, G1, ((56, 56, 56), 257 + ROOM), "the first uniform m without a geometry"),
    # ---- the 64 KiB bound of the fused decimator (uniform m: last that fits | first past) ----------------------------------
    Row("decim", CPLX, G1, ((5,) * 4, 600), "LDS bound, 4 stages: last"),
    Row("decim", CPLX, ("decim", "chain"), ((6,) * 4, 600), "LDS bound, 4 stages: first past"),
    Row("decim", REAL, G1, ((84,) * 4, 600), "LDS bound, 4 stages: last"),
    Row("decim", REAL, ("decim", "chain"), ((85,) * 4, 600), "LDS bound, 4 stages: first past"),
    Row("decim", CPLX, G1, ((105,) * 3, 600), "LDS bound, 3 stages: last"),
    Row("decim", CPLX, ("decim", "chain"), ((106,) * 3, 600), "LDS bound, 3 stages: first past"),
    Row("decim", REAL, G1, ((291,) * 3, 600), "LDS bound, 3 stages: last"),
    Row("decim", REAL, ("decim", "chain"), ((292,) * 3, 600), "LDS bound, 3 stages: first past"),
    Row("decim", CPLX, G1, ((416,) * 2, 600), "LDS bound, 2 stages: last"),
    Row("decim", CPLX, ("decim", "chain"), ((417,) * 2, 600), "LDS bound, 2 stages: first past"),
    Row("decim", REAL, G1, ((928,) * 2, 600), "LDS bound, 2 stages: last"),
    Row("decim", REAL, ("decim", "chain"), ((929,) * 2, 600), "LDS bound, 2 stages: first past"),
    Row("decim", CPLX, ("decim", "chain"), ((2, 3, 900), 600), "one long stage"),
    # ---- the interpolator ----------------------------------------------------------------------------------------------------
    Row("interp", ALL, ("interp", "fused"), ((2,), 1), "shortest call"),
    Row("interp", ALL, ("interp", "fused"), ((10, 5, 3), 300), "two tiles, the second ragged"),
    Row("interp", ALL, ("interp", "fused"), ((4, 3, 3, 2), 513), "three tiles, one input in the last"),
    Row("interp", CPLX, ("interp", "fused"), ((21,) * 4, 300), "LDS bound, 4 stages: last"),
    Row("interp", CPLX, ("interp", "chain"), ((22,) * 4, 300), "LDS bound, 4 stages: first past"),
    Row("interp", REAL, ("interp", "fused"), ((355,) * 4, 300), "LDS bound, 4 stages: last"),
    Row("interp", REAL, ("interp", "chain"), ((356,) * 4, 300), "LDS bound, 4 stages: first past"),
    Row("interp", CPLX, ("interp", "fused"), ((271,) * 3, 300), "LDS bound, 3 stages: last"),
    Row("interp", CPLX, ("interp", "chain"), ((272,) * 3, 300), "LDS bound, 3 stages: first past"),
    Row("interp", REAL, ("interp", "fused"), ((753,) * 3, 300), "LDS bound, 3 stages: last"),
    Row("interp", REAL, ("interp", "chain"), ((754,) * 3, 300), "LDS bound, 3 stages: first past"),
    Row("interp", CPLX, ("interp", "fused"), ((665,) * 2, 300), "LDS bound, 2 stages: last"),
    Row("interp", CPLX, ("interp", "chain"), ((666,) * 2, 300), "LDS bound, 2 stages: first past"),
    Row("interp", REAL, ("interp", "fused"), ((1024,) * 2, 300), "2 stages of real samples fit at every m"),
    Row("interp", CPLX, ("interp", "chain"), ((2, 3, 900), 300), "one long stage, the last"),
    Row("interp", CPLX, ("interp", "fused"), ((1024, 3, 2), 300), "one long stage, the first: fits at every m"),
    # ---- more than four stages: one Resamp2 call per stage -------------------------------------------------------------------
    Row("decim", ALL, ("decim", "chain", 5), ((2, 2, 3, 3, 4), 1 << 15), "the first two stages' calls are >= 2^19 samples, the third's is not"),
    Row("interp", ALL, ("interp", "chain", 5), ((4, 3, 3, 2, 2), 300), "shortest call"),
    # ---- Resamp2's decimator ---------------------------------------------------------------------------------------------------
    Row("resamp2", ALL, ("resamp2", "kernel"), (2, 2), "shortest call"),
    Row("resamp2", ALL, ("resamp2", "kernel"), (64, (1 << 19) - 2), "nx 2^19 - 2 | 2^19: last on resamp2_kernel"),
    Row("resamp2", ALL, ("resamp2", "chain"), (64, 1 << 19), "nx 2^19 - 2 | 2^19, m 64 | 65: the chain kernels"),
    Row("resamp2", ALL, ("resamp2", "kernel"), (65, 1 << 19), "m 64 | 65: first on resamp2_kernel"),
    Row("resamp2", ALL, ("resamp2", "chain"), (2, 1 << 19), "shortest call"),
]


def walk_name(walk, q):
    return WALK[walk] + ("/Q1" if walk in (3, 4) and q == 1 else "")


def ms_key(p, interp, ns):
    """key of a MsResamp2Plan"""
    side = "interp" if interp else "decim"
    if not p.fused:
        return (side, "chain") if ns <= 4 else (side, "chain", ns)
    if interp:
        return ("interp", "fused")
    if p.fast_tiles:
        return ("decim", "fast", ns, walk_name(p.walk[0], p.walk_q[0]), p.head_tiles)
    return ("decim", "general", p.tpw)


def object_order(family, ms):
    """the stage lengths as the object holds them (get_stage_lengths): a decimator runs its last stage first"""
    return list(ms)[::-1] if family == "decim" else list(ms)


def plan_ms(ya, elem, family, ms, n):
    return ya.plan_msresamp2(elem, family == "interp", object_order(family, ms), n)


def query(ya, row, kind):
    """(key, plan) of `row` for sample type `kind` from the library"""
    elem = ELEM[kind]
    if row.family == "resamp2":
        m, nx = row.shape
        p = ya.plan_resamp2(elem, DECIM_MODE, m, nx)
        return ("resamp2", "chain" if p.chain else "kernel"), p
    ms, n = row.shape
    p = plan_ms(ya, elem, row.family, ms, n)
    return ms_key(p, row.family == "interp", len(ms)), p


def cases(family=None):
    return [(row, kind) for row in TABLE if not family or row.family == family for kind in row.kinds]


def case_id(row, kind):
    shape = row.shape if row.family == "resamp2" else ("_".join(str(m) for m in row.shape[0]), row.shape[1])
    return f"{kind}-{'-'.join(str(k) for k in row.key)}-{'x'.join(str(s) for s in shape)}".replace("/", "")


def row_stages(row):
    """semi-lengths in processing order"""
    return [row.shape[0]] if row.family == "resamp2" else list(row.shape[0])


# ---- integer prototypes under which the whole chain is exact in f32 ----------------------------------------------------
# h1[i] = 2 hf[4m - 1 - 2i] (for_halfband at f0 = 0): the branch uses the 2m odd entries of the prototype.  A stage's
# output is bounded by (1 + sum|h1|) max|input| (delay branch + filter branch; the decimator's zeta is a power of two), so
# with G = prod_k (1 + sum|h1_k|) every partial sum of every stage is an integer (times zeta) below MAX_SAMPLE G.
LEVELS = (("dense", 3), ("dense", 1), ("sparse", 3), ("sparse", 1), ("ends", 1))
EXACT = 1 << 24


def stage_prototype(seed, m, level):
    """hf[4m+1] of integers: dense in -amp..amp, or few non-zero taps -- always the first and the last tap of the
    branch, the ones a halo that slips by one entry loses or gains"""
    rng = np.random.default_rng(seed)
    mode, amp = LEVELS[level]
    hf = rng.integers(-3, 4, 4 * m + 1).astype(np.float32)           # the even entries are never read
    v = np.zeros(2 * m, np.int64)
    if mode == "dense":
        v = rng.integers(-amp, amp + 1, 2 * m)
    elif mode == "sparse":
        idx = rng.choice(np.arange(1, 2 * m - 1), size=min(4, 2 * m - 2), replace=False)
        v[idx] = rng.integers(1, amp + 1, idx.size) * rng.choice([-1, 1], idx.size)
    for end in (0, -1):
        if v[end] == 0:
            v[end] = int(rng.integers(1, amp + 1)) * int(rng.choice([-1, 1]))
    hf[1:4 * m:2] = v
    return hf


def stage_gain(hf):
    return 1 + int(np.sum(np.abs(2.0 * hf[1::2].astype(np.float64))))


def exactness_bound(hfs):
    g = MAX_SAMPLE
    for hf in hfs:
        g *= stage_gain(hf)
    return g


def prototypes(row):
    """integer prototypes of the row's stages in processing order with MAX_SAMPLE prod (1 + sum|h1|) <= 2^24: dense taps
    in -3..3 where m is small, thinned stage by stage (the one with the largest gain first) until the bound holds"""
    ms = row_stages(row)
    seed = 1000 * TABLE.index(row)
    level = [0 if m <= 10 else 2 for m in ms]
    while True:
        hfs = [stage_prototype(seed + 10 * k + lv, m, lv) for k, (m, lv) in enumerate(zip(ms, level))]
        if exactness_bound(hfs) <= EXACT:
            return hfs
        order = sorted(range(len(ms)), key=lambda k: -stage_gain(hfs[k]))
        k = next(k for k in order if level[k] + 1 < len(LEVELS))       # StopIteration: no choice of taps is exact
        level[k] += 1


def int_stream(rng, kind, n):
    """gpu_util.int_samples in pieces (a 2^27-sample row would hold a gigabyte of int64 at once)"""
    out = np.empty(n, np.float32 if kind == "rrrf" else np.complex64)
    for o in range(0, n, 1 << 22):
        c = min(1 << 22, n - o)
        out[o:o + c] = int_samples(rng, kind, c)
    return out


def call_sizes(row):
    """n of the three calls (outputs of a decimator, inputs of an interpolator, input samples of Resamp2)"""
    if row.family == "resamp2":
        return [row.shape[1], 2, 10]
    return [row.shape[1], 1, 5]


def oracle_chain(oracle, kind, family, ms, hfs, x):
    """the stages as the oracle's sequential objects, one after the other in processing order; a decimator's zeta
    multiplies its last stage's output (the object's stage 0), as MsResamp2Obj::init folds it"""
    if family == "resamp2":
        return oracle.Resamp2(kind, hfs[0], ms[0]).execute_block("decim", x)
    stages = [oracle.Resamp2(kind, hf, m) for m, hf in zip(ms, hfs)]
    if family == "decim":
        stages[-1].set_scale(1.0 / (1 << len(ms)))
    cur = x
    for s in stages:
        cur = s.execute_block(family, cur)
    return cur
