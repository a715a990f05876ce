"""The launch plans of the FIR family and the shapes that reach them (a helper, not a conftest).

What a block call of FirFilter (kernel 1), FirDecimationFilter, Ddc, FirPfbFilter.execute_all, FirInterpolationFilter,
Duc, Rresamp and Resamp launches is decided on the host by four planners (yagi_amd/csrc/fir_bodies.hpp: fir_block_plan,
firpfb_all_plan, rresamp_plan, resamp_plan), and the library answers for a shape through yagi_amd.plan_* -- the planner
the launch itself calls.  TABLE holds, per plan key and sample type, the smallest shape that reaches the key and one
shape on each side of every threshold that separates two plans; tests/test_fir_plan_cpu.py checks every row's key
against the query and that the table covers every key a sweep of the queries meets, tests/test_gpu_fir_plans.py runs
every row on the GPU.  The rows hold for the default YAGI_HIP_DECIM_WINDOW_MIN_STEPS.

Keys
  ("consec",)                      fir_consec_kernel: M = 1, calls of >= 512 outputs
  ("decim", nt, r, staging)        fir_decim_consec_kernel<nt, r>; staging of a tile wholly inside the call's input:
                                   "pow2" (M a power of two, nt / M a multiple of r), "desc" (any other M) or "elem"
  ("staged", tile)                 fir_block_kernel<K, true> with `tile` outputs per workgroup
  ("unstaged",)                    fir_block_kernel<K, false>
  ("pfb", "few" | "taps_lds" | "taps_global" | "none")
  ("rresamp", "full" | "halved" | "none")      blocks per tile 1024 / max(P, Q) | fewer | one block does not fit
  ("resamp", "full" | "fit_limited" | "none")  1024 outputs per tile | fewer | one output's span does not fit
Shapes
  fir (M, L, ny) | pfb (nf, Ls) | rresamp (P, Q, Ls), Ls = 2 m | resamp (rate, Ls), Ls = 2 m"""
import collections

from resamp_util import rust_step          # Resamp's 8.24 step for a rate: round(2^24 / rate) in f32

Row =collections.namedtuple("Row", "family kinds key shape why")

REAL, CPLX, ALL = ("rrrf",), ("crcf", "cccf"), ("rrrf", "crcf", "cccf")
ELEM = {"rrrf": (4, 4), "crcf": (8, 4), "cccf": (8, 8)}          # bytes per sample, per tap
STAGING = {0: "elem", 1: "desc", 2: "pow2"}
PFB = {0: "few", 1: "taps_lds", 2: "taps_global", 3: "none"}

TABLE = [
    # ---- launch_fir_block ------------------------------------------------------------------------------------------
    Row("fir", ALL, ("staged", 1024), (1, 1, 511), "ny 511 | 512"),
    Row("fir", ALL, ("consec",), (1, 1, 512), "smallest; ny 511 | 512"),
    Row("fir", CPLX, ("consec",), (1, 3405, 512), "LDS bound of consec: last"),
    Row("fir", CPLX, ("staged", 1024), (1, 3406, 512), "LDS bound of consec: first past"),
    Row("fir", CPLX, ("staged", 1024), (1, 5120, 512), "LDS bound of staged 1024: last"),
    Row("fir", CPLX, ("staged", 512), (1, 5121, 512), "LDS bound of staged 1024: first past"),
    Row("fir", CPLX, ("staged", 512), (1, 5632, 512), "LDS bound of staged 512: last"),
    Row("fir", CPLX, ("staged", 256), (1, 5633, 512), "LDS bound of staged 512: first past"),
    Row("fir", CPLX, ("staged", 256), (1, 5888, 512), "LDS bound of staged 256: last"),
    Row("fir", CPLX, ("staged", 128), (1, 5889, 512), "LDS bound of staged 256: first past"),
    Row("fir", CPLX, ("staged", 64), (1, 6080, 512), "LDS bound of staged 64: last"),
    Row("fir", CPLX, ("unstaged",), (1, 6081, 512), "LDS bound of staged 64: first past"),
    Row("fir", REAL, ("consec",), (1, 8866, 512), "LDS bound of consec: last"),
    Row("fir", REAL, ("staged", 1024), (1, 8867, 512), "LDS bound of consec: first past"),
    Row("fir", REAL, ("staged", 1024), (1, 11264, 512), "LDS bound of staged 1024: last"),
    Row("fir", REAL, ("staged", 512), (1, 11265, 512), "LDS bound of staged 1024: first past"),
    Row("fir", REAL, ("staged", 256), (1, 12032, 512), "LDS bound of staged 256: last"),
    Row("fir", REAL, ("staged", 128), (1, 12033, 512), "LDS bound of staged 256: first past"),
    Row("fir", REAL, ("staged", 128), (1, 12160, 512), "LDS bound of staged 128: last"),
    Row("fir", REAL, ("staged", 64), (1, 12161, 512), "LDS bound of staged 128: first past"),
    Row("fir", REAL, ("staged", 64), (1, 12224, 512), "LDS bound of staged 64: last"),
    Row("fir", REAL, ("unstaged",), (1, 12225, 512), "LDS bound of staged 64: first past"),
    Row("fir", ALL, ("staged", 1024), (2, 1, 512), "smallest"),
    Row("fir", ALL, ("staged", 1024), (2, 15, 512), "7 | 8 taps per phase: last"),
    Row("fir", ALL, ("staged", 1024), (2, 16, 511), "ny 511 | 512"),
    Row("fir", ALL, ("decim", 256, 4, "pow2"), (2, 16, 512), "smallest; 7 | 8 taps per phase: first past; ny 511 | 512"),
    Row("fir", ALL, ("decim", 256, 4, "pow2"), (2, 63, 512), "31 | 32 taps per phase: last"),
    Row("fir", ALL, ("decim", 256, 8, "pow2"), (2, 64, 512), "smallest; 31 | 32 taps per phase: first past"),
    Row("fir", CPLX, ("decim", 256, 8, "pow2"), (2, 1344, 512), "LDS bound of decim 256 8: last"),
    Row("fir", CPLX, ("decim", 256, 4, "pow2"), (2, 1345, 512), "LDS bound of decim 256 8: first past"),
    Row("fir", ALL, ("decim", 256, 4, "desc"), (3, 24, 512), "smallest"),
    Row("fir", REAL, ("decim", 256, 8, "desc"), (3, 96, 512), "smallest"),
    Row("fir", REAL, ("decim", 256, 4, "pow2"), (4, 32, 512), "real samples: M 4 | 5 at 8 taps per phase"),
    Row("fir", CPLX, ("decim", 256, 4, "pow2"), (4, 784, 512), "LDS bound of decim 256 4: last"),
    Row("fir", CPLX, ("decim", 128, 4, "pow2"), (4, 785, 512), "LDS bound of decim 256 4: first past"),
    Row("fir", REAL, ("decim", 64, 8, "pow2"), (4, 7761, 512), "smallest"),
    Row("fir", REAL, ("staged", 1024), (5, 40, 512), "real samples: M 4 | 5 at 8 taps per phase"),
    Row("fir", CPLX, ("decim", 128, 4, "desc"), (5, 40, 512), "smallest"),
    Row("fir", REAL, ("staged", 1024), (5, 159, 512), "31 | 32 taps per phase: last"),
    Row("fir", REAL, ("decim", 256, 8, "desc"), (5, 160, 512), "31 | 32 taps per phase: first past"),
    Row("fir", REAL, ("decim", 256, 8, "desc"), (5, 600, 512), "LDS bound of decim 256 8: last"),
    Row("fir", REAL, ("decim", 256, 4, "desc"), (5, 601, 512), "LDS bound of decim 256 8: first past"),
    Row("fir", CPLX, ("staged", 512), (6, 1, 512), "smallest"),
    Row("fir", CPLX, ("decim", 128, 4, "pow2"), (8, 64, 512), "smallest"),
    Row("fir", CPLX, ("decim", 64, 8, "pow2"), (8, 769, 512), "smallest"),
    Row("fir", CPLX, ("decim", 128, 4, "desc"), (9, 252, 512), "LDS bound of decim 128 4: last"),
    Row("fir", CPLX, ("staged", 512), (9, 253, 512), "LDS bound of decim 128 4: first past"),
    Row("fir", CPLX, ("staged", 512), (9, 287, 512), "31 | 32 taps per phase: last"),
    Row("fir", CPLX, ("decim", 64, 8, "desc"), (9, 288, 512), "smallest; 31 | 32 taps per phase: first past"),
    Row("fir", REAL, ("decim", 256, 4, "desc"), (9, 540, 512), "LDS bound of decim 256 4: last"),
    Row("fir", REAL, ("decim", 128, 4, "desc"), (9, 541, 512), "LDS bound of decim 256 4: first past"),
    Row("fir", CPLX, ("decim", 64, 8, "desc"), (9, 720, 512), "LDS bound of decim 64 8: last"),
    Row("fir", CPLX, ("decim", 64, 4, "desc"), (9, 721, 512), "LDS bound of decim 64 8: first past"),
    Row("fir", REAL, ("decim", 128, 4, "desc"), (10, 320, 512), "smallest"),
    Row("fir", CPLX, ("decim", 64, 4, "desc"), (10, 320, 512), "smallest"),
    Row("fir", REAL, ("staged", 512), (12, 1, 512), "smallest"),
    Row("fir", CPLX, ("staged", 256), (12, 1, 512), "smallest"),
    Row("fir", REAL, ("decim", 128, 4, "pow2"), (16, 512, 512), "smallest"),
    Row("fir", CPLX, ("decim", 64, 4, "pow2"), (16, 512, 512), "smallest"),
    Row("fir", CPLX, ("decim", 64, 4, "pow2"), (16, 704, 512), "LDS bound of decim 64 4: last"),
    Row("fir", CPLX, ("staged", 256), (16, 705, 512), "LDS bound of decim 64 4: first past"),
    Row("fir", REAL, ("decim", 64, 4, "pow2"), (16, 2561, 512), "smallest"),
    Row("fir", REAL, ("decim", 128, 4, "desc"), (17, 1020, 512), "LDS bound of decim 128 4: last"),
    Row("fir", REAL, ("decim", 64, 8, "desc"), (17, 1021, 512), "LDS bound of decim 128 4: first past"),
    Row("fir", REAL, ("decim", 64, 8, "desc"), (18, 576, 512), "smallest"),
    Row("fir", REAL, ("decim", 64, 8, "desc"), (19, 912, 512), "LDS bound of decim 64 8: last"),
    Row("fir", REAL, ("decim", 64, 4, "desc"), (19, 913, 512), "LDS bound of decim 64 8: first past"),
    Row("fir", REAL, ("decim", 64, 4, "desc"), (20, 640, 512), "smallest"),
    Row("fir", REAL, ("staged", 512), (23, 506, 512), "LDS bound of staged 512: last"),
    Row("fir", REAL, ("staged", 256), (23, 507, 512), "LDS bound of staged 512: first past"),
    Row("fir", REAL, ("staged", 256), (24, 1, 512), "smallest"),
    Row("fir", CPLX, ("staged", 128), (24, 1, 512), "smallest"),
    Row("fir", REAL, ("decim", 64, 4, "desc"), (33, 1188, 512), "LDS bound of decim 64 4: last"),
    Row("fir", REAL, ("staged", 256), (33, 1189, 512), "LDS bound of decim 64 4: first past"),
    Row("fir", CPLX, ("staged", 128), (47, 94, 512), "LDS bound of staged 128: last"),
    Row("fir", CPLX, ("staged", 64), (47, 95, 512), "LDS bound of staged 128: first past"),
    Row("fir", REAL, ("staged", 128), (48, 1, 512), "smallest"),
    Row("fir", CPLX, ("staged", 64), (48, 1, 512), "smallest"),
    Row("fir", REAL, ("staged", 64), (64, 4097, 512), "64 phases of 65 taps: no window kernel fits"),
    Row("fir", REAL, ("staged", 64), (96, 1, 512), "smallest"),
    Row("fir", CPLX, ("unstaged",), (96, 1, 512), "smallest"),
    Row("fir", REAL, ("unstaged",), (256, 1, 512), "smallest"),
    # ---- launch_firpfb_all -----------------------------------------------------------------------------------------
    Row("pfb", ALL, ("pfb", "few"), (2, 1), "smallest"),
    Row("pfb", ALL, ("pfb", "few"), (16, 4), "nf 16 | 17"),
    Row("pfb", ALL, ("pfb", "taps_lds"), (17, 4), "nf 16 | 17"),
    Row("pfb", ALL, ("pfb", "taps_lds"), (17, 1), "smallest"),
    Row("pfb", ALL, ("pfb", "taps_lds"), (32, 8), "interpolation factor 32"),
    Row("pfb", ALL, ("pfb", "taps_lds"), (100, 3), "interpolation factor above 64"),
    Row("pfb", REAL, ("pfb", "taps_lds"), (17, 679), "LDS bound of the taps: last"),
    Row("pfb", REAL, ("pfb", "taps_global"), (17, 680), "smallest; LDS bound of the taps: first past"),
    Row("pfb", REAL, ("pfb", "taps_lds"), (100, 121), "LDS bound of the taps: last"),
    Row("pfb", REAL, ("pfb", "taps_global"), (100, 122), "LDS bound of the taps: first past"),
    Row("pfb", REAL, ("pfb", "few"), (2, 12033), "LDS bound of the 256-sample span: last"),
    Row("pfb", REAL, ("pfb", "taps_global"), (2, 12034), "LDS bound of the 256-sample span: first past"),
    Row("pfb", REAL, ("pfb", "taps_global"), (2, 12225), "LDS bound of the 64-sample span: last"),
    Row("pfb", REAL, ("pfb", "none"), (2, 12226), "LDS bound of the 64-sample span: first past"),
    Row("pfb", ("crcf",), ("pfb", "taps_lds"), (17, 640), "LDS bound of the taps: last"),
    Row("pfb", ("crcf",), ("pfb", "taps_global"), (17, 641), "LDS bound of the taps: first past"),
    Row("pfb", ("crcf",), ("pfb", "taps_lds"), (100, 119), "LDS bound of the taps: last"),
    Row("pfb", ("crcf",), ("pfb", "taps_global"), (100, 120), "LDS bound of the taps: first past"),
    Row("pfb", ("cccf",), ("pfb", "taps_lds"), (17, 337), "LDS bound of the taps: last"),
    Row("pfb", ("cccf",), ("pfb", "taps_global"), (17, 338), "smallest; LDS bound of the taps: first past"),
    Row("pfb", ("cccf",), ("pfb", "taps_lds"), (100, 60), "LDS bound of the taps: last"),
    Row("pfb", ("cccf",), ("pfb", "taps_global"), (100, 61), "LDS bound of the taps: first past"),
    Row("pfb", CPLX, ("pfb", "few"), (2, 5889), "LDS bound of the 256-sample span: last"),
    Row("pfb", CPLX, ("pfb", "taps_global"), (2, 5890), "LDS bound of the 256-sample span: first past"),
    Row("pfb", CPLX, ("pfb", "taps_global"), (2, 6081), "LDS bound of the 64-sample span: last"),
    Row("pfb", CPLX, ("pfb", "none"), (2, 6082), "smallest; LDS bound of the 64-sample span: first past"),
    # ---- launch_rresamp (Ls = 2 m is even) ---------------------------------------------------------------------------
    Row("rresamp", ALL, ("rresamp", "full"), (1, 1, 2), "smallest"),
    Row("rresamp", ALL, ("rresamp", "full"), (7000, 1, 4), "P above the 1024 outputs of a tile: one block per workgroup"),
    Row("rresamp", REAL, ("rresamp", "full"), (1, 1, 11264), "LDS bound of 1024 blocks: last"),
    Row("rresamp", REAL, ("rresamp", "halved"), (1, 1, 11266), "LDS bound of 1024 blocks: first past"),
    Row("rresamp", REAL, ("rresamp", "full"), (3, 5, 11268), "LDS bound of 204 blocks: last"),
    Row("rresamp", REAL, ("rresamp", "halved"), (3, 5, 11270), "LDS bound of 204 blocks: first past"),
    Row("rresamp", REAL, ("rresamp", "full"), (5, 3, 11676), "LDS bound of 204 blocks: last"),
    Row("rresamp", REAL, ("rresamp", "halved"), (5, 3, 11678), "LDS bound of 204 blocks: first past"),
    Row("rresamp", REAL, ("rresamp", "halved"), (3, 5, 12284), "LDS bound of one block, halved down to it: last"),
    Row("rresamp", REAL, ("rresamp", "none"), (3, 5, 12286), "LDS bound of one block: first past"),
    Row("rresamp", REAL, ("rresamp", "full"), (1, 7000, 5288), "LDS bound of one block, Q 7000: last"),
    Row("rresamp", REAL, ("rresamp", "none"), (1, 7000, 5290), "LDS bound of one block, Q 7000: first past"),
    Row("rresamp", CPLX, ("rresamp", "full"), (1, 1, 5120), "LDS bound of 1024 blocks: last"),
    Row("rresamp", CPLX, ("rresamp", "halved"), (1, 1, 5122), "smallest; LDS bound of 1024 blocks: first past"),
    Row("rresamp", CPLX, ("rresamp", "full"), (3, 5, 5124), "LDS bound of 204 blocks: last"),
    Row("rresamp", CPLX, ("rresamp", "halved"), (3, 5, 5126), "LDS bound of 204 blocks: first past"),
    Row("rresamp", CPLX, ("rresamp", "full"), (5, 3, 5532), "LDS bound of 204 blocks: last"),
    Row("rresamp", CPLX, ("rresamp", "halved"), (5, 3, 5534), "LDS bound of 204 blocks: first past"),
    Row("rresamp", CPLX, ("rresamp", "halved"), (3, 5, 6140), "LDS bound of one block, halved down to it: last"),
    Row("rresamp", CPLX, ("rresamp", "none"), (3, 5, 6142), "LDS bound of one block: first past"),
    Row("rresamp", CPLX, ("rresamp", "full"), (1, 1024, 5120), "LDS bound of one block, Q 1024: last"),
    Row("rresamp", CPLX, ("rresamp", "none"), (1, 1024, 5122), "LDS bound of one block, Q 1024: first past"),
    Row("rresamp", CPLX, ("rresamp", "none"), (1, 7000, 2), "smallest: 7000 complex inputs of one block do not fit"),
    # ---- launch_resamp (Ls = 2 m is even; the object refuses a "none" shape when it is created) --------------------------
    Row("resamp", ALL, ("resamp", "full"), (1.0, 2), "smallest"),
    Row("resamp", ALL, ("resamp", "full"), (250.0, 2), "highest rate"),
    Row("resamp", ALL, ("resamp", "fit_limited"), (0.004, 2), "smallest: lowest rate, 250 inputs per output"),
    Row("resamp", ALL, ("resamp", "fit_limited"), (0.05, 14), "20 inputs per output"),
    Row("resamp", REAL, ("resamp", "full"), (1.0, 11264), "LDS bound of 1024 outputs: last"),
    Row("resamp", REAL, ("resamp", "fit_limited"), (1.0, 11266), "LDS bound of 1024 outputs: first past"),
    Row("resamp", REAL, ("resamp", "full"), (3.7, 12010), "LDS bound of 1024 outputs: last"),
    Row("resamp", REAL, ("resamp", "fit_limited"), (3.7, 12012), "LDS bound of 1024 outputs: first past"),
    Row("resamp", REAL, ("resamp", "fit_limited"), (1.0, 12286), "LDS bound of one output: last"),
    Row("resamp", REAL, ("resamp", "none"), (1.0, 12288), "LDS bound of one output: first past"),
    Row("resamp", CPLX, ("resamp", "full"), (1.0, 5120), "LDS bound of 1024 outputs: last"),
    Row("resamp", CPLX, ("resamp", "fit_limited"), (1.0, 5122), "LDS bound of 1024 outputs: first past"),
    Row("resamp", CPLX, ("resamp", "full"), (3.7, 5866), "LDS bound of 1024 outputs: last"),
    Row("resamp", CPLX, ("resamp", "fit_limited"), (3.7, 5868), "LDS bound of 1024 outputs: first past"),
    Row("resamp", CPLX, ("resamp", "fit_limited"), (1.0, 6142), "LDS bound of one output: last"),
    Row("resamp", CPLX, ("resamp", "none"), (1.0, 6144), "smallest; LDS bound of one output: first past"),
]


def plan_of(ya, rec):
    """a record of a plan_*_range array as a Plan"""
    return ya.Plan(*(int(rec[f]) for f in ya.Plan._fields))


def fir_key(p):
    """key of a Plan of plan_fir_block"""
    if p.kind == 0:
        return ("consec",)
    if p.kind == 1:
        return ("decim", p.nt, p.r, STAGING[p.staging])
    if p.kind == 2:
        return ("staged", p.tile)
    return ("unstaged",)


def rresamp_class(tile, P, Q):
    if tile == 0:
        return "none"
    return "full" if tile == max(1, 1024 // max(P, Q)) else "halved"


def resamp_class(tile):
    return "none" if tile == 0 else "full" if tile == 1024 else "fit_limited"


def query(ya, row, kind):
    """(key, Plan) of `row` for sample type `kind` from the library; Plan.tile = 0 where the shape does not fit"""
    elem, celem = ELEM[kind]
    if row.family == "fir":
        M, L, ny = row.shape
        p = ya.plan_fir_block(elem, L, M, ny)
        return fir_key(p), p
    if row.family == "pfb":
        nf, Ls = row.shape
        p = ya.plan_firpfb_all(elem, celem, nf, Ls)
        return ("pfb", PFB[p.kind]), p
    if row.family == "rresamp":
        P, Q, Ls = row.shape
        p = plan_of(ya, ya.plan_rresamp_range(elem, P, Q, Ls, 1)[0])
        return ("rresamp", rresamp_class(p.tile, P, Q)), p
    rate, Ls = row.shape
    p = plan_of(ya, ya.plan_resamp_range(elem, Ls, 1, rust_step(rate))[0])
    return ("resamp", resamp_class(p.tile)), p


def cases(family=None, runnable_fir=True):
    """(row, kind) pairs; with runnable_fir the fir rows at ny = 511 are left out (the 512 rows' streams hold such a call)"""
    out = []
    for row in TABLE:
        if family and row.family != family:
            continue
        if runnable_fir and row.family == "fir" and row.shape[2] < 512:
            continue
        out += [(row, kind) for kind in row.kinds]
    return out


def case_id(row, kind):
    return f"{kind}-{'-'.join(str(k) for k in row.key)}-{'x'.join(str(s) for s in row.shape)}"
