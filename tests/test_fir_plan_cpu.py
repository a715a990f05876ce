"""The plan queries of the C ABI (yagi_hip_plan_*) against tests/fir_shapes.py, on the CPU: no device is needed.

  * every row of the table has the key the library reports for its shape;
  * a sweep of the queries collects every key that occurs; the table holds, for every key and sample type, a row as
    small as the smallest shape of the sweep, and a row on each side of every threshold at which the plan changes
    along the tap count -- a missing row fails with the key's name;
  * a key of the planners' enums that the sweep never meets is listed below with the reason.

Sweep: fir_block_plan and firpfb_all_plan over elem 4 and 8, M / nf in 1..64 and 96, 100, 128, 256, 300, 512, 1024, 2048,
L / Ls in 1..8192 (ny 511 and 512); rresamp over P, Q in 1..64, 1024, 7000 and resamp over rates 0.004..250, Ls up to
8192.  The thresholds are followed up to 13000 taps, past the last LDS bound of real samples."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fir_shapes as fs
from conftest import ROOT

pytestmark = pytest.mark.skipif("YAGI_HIP_DECIM_WINDOW_MIN_STEPS" in os.environ,
                                reason="tests/fir_shapes.py describes the default YAGI_HIP_DECIM_WINDOW_MIN_STEPS")

SWEEP_M = list(range(1, 65)) + [96, 100, 128, 256, 300, 512, 1024, 2048]
SWEEP_PQ = list(range(1, 65)) + [1024, 7000]
SWEEP_RATES = sorted(set([0.004, 0.05, 0.5, 1.0, 3.7, 250.0] + [float(r) for r in np.geomspace(0.004, 250.0, 49)]))
L_SWEEP, L_FOLLOW = 8192, 13000
KINDS = ("rrrf", "crcf", "cccf")
NT_R = [(256, 8), (256, 4), (128, 4), (64, 8), (64, 4)]

# Keys of the enums that no shape reaches, per sample type, with the reason.
UNREACHABLE = {}
for _kind in KINDS:
    for _nt, _r in NT_R:
        # the body falls back to entry-by-entry staging of an interior tile only when the tile's entries, (nt r + taps
        # per phase - 1) M samples, pass 4 GiB; a shape whose M rows fit 48 KiB of LDS is five orders of magnitude below
        UNREACHABLE[(_kind, ("decim", _nt, _r, "elem"))] = "interior tiles of a shape that fits the LDS are far below 4 GiB"
for _kind in ("crcf", "cccf"):
    # <256, 8> needs M rows of at least (2048 + 8 + 32) 9/8 complex samples: M <= 2 in 48 KiB, and 2 is a power of two
    UNREACHABLE[(_kind, ("decim", 256, 8, "desc"))] = "fits complex samples only at M = 2, which stages by the power-of-two path"
# Keys met only above the sweep's 8192 taps (the table holds rows for them all the same).
BEYOND_SWEEP = {
    ("rrrf", ("pfb", "none")): "64 + Ls - 1 real samples pass 48 KiB from Ls = 12226",
    ("rrrf", ("rresamp", "halved")): "1024 real inputs + Ls - 1 pass 48 KiB from Ls = 11266",
    ("rrrf", ("resamp", "none")): "Ls + 1 real samples pass 48 KiB from Ls = 12288",
}
# Rows the issue names or that mark a threshold in M, nf or ny instead of the tap count.
NAMED = [
    ("fir", (1, 1, 511)), ("fir", (1, 1, 512)), ("fir", (2, 16, 511)), ("fir", (2, 16, 512)),      # ny 511 | 512
    ("fir", (4, 32, 512)), ("fir", (5, 40, 512)),                       # real samples: short phases only up to M = 4
    ("fir", (64, 4097, 512)),
    ("pfb", (16, 4)), ("pfb", (17, 4)), ("pfb", (32, 8)), ("pfb", (100, 3)),                       # nf 16 | 17, 32, > 64
    ("rresamp", (7000, 1, 4)), ("resamp", (250.0, 2)), ("resamp", (0.05, 14)),
]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def universe(kind):
    keys = [("consec",), ("unstaged",)] + [("staged", t) for t in (1024, 512, 256, 128, 64)]
    keys += [("decim", nt, r, s) for nt, r in NT_R for s in ("elem", "desc", "pow2")]
    keys += [("pfb", k) for k in fs.PFB.values()]
    keys += [("rresamp", k) for k in ("full", "halved", "none")] + [("resamp", k) for k in ("full", "fit_limited", "none")]
    return keys


def fir_codes(p):
    return ((p["kind"].astype(np.int64) << 40) | (p["nt"].astype(np.int64) << 28) | (p["r"].astype(np.int64) << 24) |
            (p["staging"].astype(np.int64) << 20) | p["tile"])


def fir_threshold(M, L, a, b):
    """the name of the threshold between key a at L taps and key b at L + 1"""
    if a[0] == "staged" and b[0] == "decim":
        return f"{(L + 1) // M - 1} | {(L + 1) // M} taps per phase"
    if a[0] == "decim" and b[0] == "decim" and a[1:3] == (256, 4) and b[1:3] == (256, 8):
        return "31 | 32 taps per phase, 4- to 8-sample window"
    return "LDS bound of " + " ".join(str(v) for v in (a[:3] if a[0] == "decim" else a))


@pytest.fixture(scope="module")
def sweep(ya):
    """smallest[(kind, key)] = the size of the smallest shape with that key (fir M L, pfb nf Ls, rresamp and resamp Ls);
    thresholds[(family, kind)] = the names of the thresholds met along the tap count"""
    smallest, thresholds = {}, {}

    def note(kind, key, size):
        if size < smallest.get((kind, key), 1 << 62):
            smallest[(kind, key)] = size

    for kind in KINDS:
        elem, celem = fs.ELEM[kind]
        th = thresholds.setdefault(("fir", kind), set())
        for M in SWEEP_M:
            for ny in (511, 512):
                p = ya.plan_fir_block_range(elem, 1, L_FOLLOW, M, ny)
                starts = np.concatenate([[0], np.flatnonzero(np.diff(fir_codes(p))) + 1])
                keys = [fs.fir_key(fs.plan_of(ya, p[i])) for i in starts]
                for i, k in zip(starts, keys):
                    if i + 1 <= L_SWEEP:
                        note(kind, k, M * int(i + 1))
                if ny == 512:
                    th.update(fir_threshold(M, int(i), a, b) for i, a, b in zip(starts[1:], keys[:-1], keys[1:]))
        for nf in SWEEP_M[1:]:                      # an interpolator has at least two branches
            p = ya.plan_firpfb_all_range(elem, celem, nf, 1, L_SWEEP)
            u, idx = np.unique(p["kind"], return_index=True)
            for k, i in zip(u, idx):
                note(kind, ("pfb", fs.PFB[int(k)]), nf * int(i + 1))
        for P in SWEEP_PQ:
            for Q in SWEEP_PQ:
                t = ya.plan_rresamp_range(elem, P, Q, 1, L_SWEEP)["tile"][1::2]          # Ls = 2 m
                full = max(1, 1024 // max(P, Q))
                cls = np.where(t == 0, 2, np.where(t == full, 0, 1))
                u, idx = np.unique(cls, return_index=True)
                for k, i in zip(u, idx):
                    note(kind, ("rresamp", ("full", "halved", "none")[int(k)]), 2 * int(i + 1))
        for rate in SWEEP_RATES:
            t = ya.plan_resamp_range(elem, 1, L_SWEEP, fs.rust_step(rate))["tile"][1::2]
            cls = np.where(t == 0, 2, np.where(t == 1024, 0, 1))
            u, idx = np.unique(cls, return_index=True)
            for k, i in zip(u, idx):
                note(kind, ("resamp", ("full", "fit_limited", "none")[int(k)]), 2 * int(i + 1))
    return smallest, thresholds


def row_size(row):
    s = row.shape
    return {"fir": lambda: s[0] * s[1], "pfb": lambda: s[0] * s[1], "rresamp": lambda: s[2], "resamp": lambda: s[1]}[row.family]()


def test_queries_need_no_device_and_reject_bad_arguments(ya):
    p = ya.plan_fir_block(8, 2049, 8, 4096)
    assert (p.kind, p.nt, p.r, p.tile, p.staging) == (ya.PLAN_FIR_DECIM, 64, 4, 256, ya.PLAN_STAGE_POW2) and 0 < p.lds <= 48 << 10
    assert ya.plan_firpfb_all(8, 4, 32, 400).kind == ya.PLAN_PFB_TAPS_GLOBAL
    assert ya.plan_rresamp(4, 3, 5, 30).tile == 204 and ya.plan_resamp(4, 14, 1 << 24).tile == 1024
    for bad in (lambda: ya.plan_fir_block(3, 8, 2, 512), lambda: ya.plan_fir_block(4, 0, 2, 512),
                lambda: ya.plan_fir_block(4, 8, 0, 512), lambda: ya.plan_fir_block(4, 8, 2, 0),
                lambda: ya.plan_firpfb_all(4, 8, 4, 4), lambda: ya.plan_firpfb_all(8, 4, 0, 4),
                lambda: ya.plan_rresamp(4, 0, 1, 4), lambda: ya.plan_resamp(4, 4, 0), lambda: ya.plan_resamp(16, 4, 1)):
        with pytest.raises(ya.ConfigError):
            bad()
    assert ya.lib.yagi_hip_plan_fir_block(4, 8, 2, 512, None) == 2          # YAGI_ERR_CONFIG: null out
    one = np.zeros(1, ya.PLAN_DTYPE)
    assert ya.lib.yagi_hip_plan_fir_block_range(4, 2, 2 ** 64 - 1, 2, 512, one.ctypes.data) == 2      # L0 + count wraps
    assert ya.lib.yagi_hip_plan_resamp_range(4, 2, 2 ** 64 - 1, 1, one.ctypes.data) == 2


def test_range_queries_equal_the_single_ones(ya):
    rng = np.random.default_rng(11)
    for _ in range(200):
        elem = int(rng.choice([4, 8]))
        M, L, ny = int(rng.integers(1, 80)), int(rng.integers(1, 9000)), int(rng.choice([100, 511, 512, 5000]))
        r = ya.plan_fir_block_range(elem, L, 3, M, ny)
        assert [fs.plan_of(ya, v) for v in r] == [ya.plan_fir_block(elem, L + i, M, ny) for i in range(3)]
        celem = int(rng.choice([4, elem]))
        r = ya.plan_firpfb_all_range(elem, celem, M, L, 2)
        assert [fs.plan_of(ya, v) for v in r] == [ya.plan_firpfb_all(elem, celem, M, L + i) for i in range(2)]


@pytest.mark.parametrize("row,kind", fs.cases(runnable_fir=False), ids=[fs.case_id(r, k) for r, k in fs.cases(runnable_fir=False)])
def test_row_has_the_key_the_library_reports(ya, row, kind):
    key, p = fs.query(ya, row, kind)
    assert key == row.key, (row.shape, kind, p)
    elem = fs.ELEM[kind][0]
    assert p.lds <= 48 << 10
    if row.family == "rresamp":                    # the single query fails exactly where the block call does
        if key[1] == "none":
            with pytest.raises(ya.ConfigError, match="do not fit"):
                ya.plan_rresamp(elem, *row.shape)
        else:
            assert ya.plan_rresamp(elem, *row.shape) == p
    if row.family == "resamp":
        if key[1] == "none":
            with pytest.raises(ya.ConfigError, match="does not fit"):
                ya.plan_resamp(elem, row.shape[1], fs.rust_step(row.shape[0]))
        else:
            assert ya.plan_resamp(elem, row.shape[1], fs.rust_step(row.shape[0])) == p


def test_table_covers_every_key_of_the_sweep(ya, sweep):
    smallest, _ = sweep
    have = {}
    for row, kind in fs.cases(runnable_fir=False):
        have[(kind, row.key)] = min(have.get((kind, row.key), 1 << 62), row_size(row))
    missing = [f"{kind} {key}: no row" for (kind, key) in smallest if (kind, key) not in have]
    missing += [f"{kind} {key}: smallest row has size {have[(kind, key)]}, the sweep found {size}"
                for (kind, key), size in smallest.items() if (kind, key) in have and have[(kind, key)] > size]
    missing += [f"{kind} {key}: met only above {L_SWEEP} taps, no row" for (kind, key) in BEYOND_SWEEP if (kind, key) not in have]
    assert not missing, "\n".join(sorted(missing))
    # every key of the enums is met by the sweep, lies beyond it, or is listed as unreachable -- and only one of these
    for kind in KINDS:
        for key in universe(kind):
            where = [(kind, key) in smallest, (kind, key) in BEYOND_SWEEP, (kind, key) in UNREACHABLE]
            assert sum(where) == 1, (kind, key, where)
    for row, kind in fs.cases(runnable_fir=False):
        assert (kind, row.key) not in UNREACHABLE


def test_table_has_both_sides_of_every_threshold(ya, sweep):
    _, thresholds = sweep
    rows = {(r.family, k, r.shape): r.key for r, k in fs.cases(runnable_fir=False)}
    missing = []
    for kind in KINDS:
        have = set()
        for (fam, k, shape), key in rows.items():
            if fam == "fir" and k == kind and shape[2] == 512:
                M, L, _ = shape
                nxt = rows.get(("fir", kind, (M, L + 1, 512)))
                if nxt is not None and nxt != key:
                    have.add(fir_threshold(M, L, key, nxt))
        missing += [f"fir {kind}: {t}" for t in thresholds[("fir", kind)] - have]
    # the bank and resampler planners: every change of class met along Ls for an nf / (P, Q) / rate the table uses lies
    # between two rows of the table on one of these lines (Ls = 2 m is even for the resamplers)
    for kind in KINDS:
        elem, celem = fs.ELEM[kind]
        lines, need, have = {}, {}, set()
        for (fam, k, shape) in rows:
            if k == kind and fam != "fir":
                lines.setdefault((fam, shape[:-1]), set()).add(shape[-1])
        for (fam, head), taps in lines.items():
            if fam == "pfb":
                cls = [fs.PFB[int(v)] for v in ya.plan_firpfb_all_range(elem, celem, head[0], 1, L_FOLLOW)["kind"]]
                step = 1
            elif fam == "rresamp":
                t = ya.plan_rresamp_range(elem, head[0], head[1], 1, L_FOLLOW)["tile"]
                cls, step = [fs.rresamp_class(int(v), *head) for v in t], 2
            else:
                t = ya.plan_resamp_range(elem, 1, L_FOLLOW, fs.rust_step(head[0]))["tile"]
                cls, step = [fs.resamp_class(int(v)) for v in t], 2
            for Ls in range(step, L_FOLLOW - step + 1, step):
                a, b = cls[Ls - 1], cls[Ls + step - 1]
                if a != b:
                    need.setdefault((fam, a, b), f"{fam} {kind}: {a} | {b}, e.g. {head} at {Ls} | {Ls + step} taps")
                    if Ls in taps and Ls + step in taps:
                        have.add((fam, a, b))
        missing += [msg for k, msg in need.items() if k not in have]
    assert not missing, "\n".join(sorted(missing))
    absent = [n for n in NAMED if not any(r.family == n[0] and r.shape == n[1] for r in fs.TABLE)]
    assert not absent, absent


def test_override_variable_reaches_the_query():
    """the query reads YAGI_HIP_DECIM_WINDOW_MIN_STEPS through the planner, as the launch does"""
    code = ("import yagi_amd as ya; p = ya.plan_fir_block(8, 64, 2, 512); q = ya.plan_fir_block(8, 4, 2, 512); "
            "print(p.kind, q.kind)")
    out = {}
    for v in ("0", "100000"):
        env = dict(os.environ, YAGI_HIP_DECIM_WINDOW_MIN_STEPS=v, YAGI_NO_TORCH_PRELOAD="1")
        out[v] = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT, env=env, text=True).split()
    assert out["0"] == ["1", "1"] and out["100000"] == ["2", "2"], out
