"""The launch shapes of Spgram and the calls that reach them (a helper, not a conftest).

What a write of n transforms launches is host arithmetic in yagi_amd/csrc/spgram_kernels.hip (spgram_launch_frames,
spgram_fused_slab, spgram_fused_rows, spgram_frames_grid), and yagi_amd.plan_spgram answers with those very functions.
A row of TABLE names a geometry and either a rule that derives the transform count of its main call from the plan query
(so the count follows the launch code if its thresholds move) or an explicit list of operations; `key` is what the
query must report for the largest call of the row.

Keys
  ("fused", group, slab, workgroups, rows, fold_rows, launches)   fold_rows = 0: the partial rows are summed unfolded
  ("unfused", workgroups, rows, launches)                         workgroups of the frame builder, rows = 32-frame slabs
  both describe the first launch of the call; launches = ceil(transforms / launch_frames)

Rules (B = group, S = the smallest slab of the nfft, L = launch_frames, A = accum_slab)
  one, group-1, group, group+1      1, B - 1, B, B + 1 transforms: dead slots in the frame group
  slab3+1                           3 S + 1: ragged last workgroup
  rows64 / rows65                   the last count with rows <= 64 (summed unfolded) / the first with rows > 64 (folded)
  fold_ragged                       the first folded count with more than 4 fold_rows, their number no multiple of 4 (the
                                    sum kernel adds four at a time), whose last fold chunk is ragged (rows no multiple
                                    of 32)
  slab_above / slab_cap             the first count whose slab exceeds S / reaches the slab of a full launch (32)
  cut+k                             L + k transforms in one call: the launch cut of run_frames
  acc-1, acc, acc+1, 2acc+1         A - 1, A, A + 1, 2 A + 1: the Horner slabs of the unfused accumulation
  stride                            the first count whose frames exceed 256 elements per workgroup of the capped grid
                                    (the frame builder's grid-stride loop) plus 43
A rule row is two calls: delay - 1 samples (shorter than the timer, no transform, carried in the window) and one
write_dev that runs exactly the rule's count and ends one sample past its last transform (delay > 1).

Every case runs in accumulate mode ("acc") and in recursive mode ("rec": set_alpha before the first write with
alpha = min(0.3, 1.5 / transforms), so gamma^transforms stays above 0.1 and every frame's weight is visible; set_alpha(-1)
after the last write exposes the estimate, whose linear scale is 0 while averaging)."""
import collections
import functools

import numpy as np

import spgram_ref as sr

Row = collections.namedtuple("Row", "name nfft wlen delay win spec key real why")
HAMMING, FLATTOP, TRIANGULAR, RCOSTAPER = 1, 6, 7, 8           # yagi_amd.WindowType
FUSED = (256, 512, 1024, 2048, 4096)
MODES = ("acc", "rec")
# A swap of two adjacent weights moves the estimate by about alpha times the frames' share of it: below what f32 resolves
# once alpha is small, and alpha is bounded by gamma^transforms > 0.1.  So the swap is checked wherever alpha >= 0.1
# (up to 15 transforms), and at the first frame of every recursive case, whose weight differs from its neighbour's by
# the factor 1 / alpha whatever alpha is.
SWAP_MIN_ALPHA = 0.1
# The cap on the device's error (per bin relative to the largest bin, and in rel-L2).  At most a tenth of the smallest
# effect any mutation of test_spgram_ref_cpu.py has on any case of the table: 3.6e-4 (512-alpha-switch, frame 198
# displaced by one sample); the f32 model of the pipeline errs by 2e-8 .. 6e-7 on these cases (and by 1.4e-4 on the
# recursive 2^20-transform row, where it rounds psd 2^20 times in a row).
TOL = 2e-5
MUTATION_FACTOR = 10


def key_of(p, n):
    launches = -(-n // p.launch_frames)
    if p.fused:
        return ("fused", p.group, p.slab, p.workgroups, p.rows, p.fold_rows, launches)
    return ("unfused", p.workgroups, p.rows, launches)


@functools.lru_cache(maxsize=None)
def _first(ya, nfft, what):
    p1 = ya.plan_spgram(nfft, 1)
    full = ya.plan_spgram(nfft, p1.launch_frames)
    pred = {"folded": lambda p, n: p.folded,
            "fold_ragged": lambda p, n: p.folded and p.fold_rows > 4 and p.fold_rows % 4 and p.rows % 32,
            "slab_above": lambda p, n: p.slab > p1.slab,
            "slab_cap": lambda p, n: p.slab == full.slab,
            "stride": lambda p, n: n * nfft > p.workgroups * 256}[what]
    for n in range(1, p1.launch_frames + 1):
        if pred(ya.plan_spgram(nfft, n), n):
            return n
    raise AssertionError((nfft, what))


def count(ya, nfft, rule):
    """transforms of the main call of a rule row, from the plan query"""
    p1 = ya.plan_spgram(nfft, 1)
    B, S, L, A = p1.group, p1.slab, p1.launch_frames, p1.accum_slab
    if rule.startswith("cut+"):
        return L + int(rule[4:])
    return {"one": lambda: 1, "group-1": lambda: B - 1, "group": lambda: B, "group+1": lambda: B + 1,
            "slab3+1": lambda: 3 * S + 1, "rows64": lambda: _first(ya, nfft, "folded") - 1,
            "rows65": lambda: _first(ya, nfft, "folded"), "fold_ragged": lambda: _first(ya, nfft, "fold_ragged"),
            "slab_above": lambda: _first(ya, nfft, "slab_above"), "slab_cap": lambda: _first(ya, nfft, "slab_cap"),
            "acc-1": lambda: A - 1, "acc": lambda: A, "acc+1": lambda: A + 1, "2acc+1": lambda: 2 * A + 1,
            "stride": lambda: _first(ya, nfft, "stride") + 43}[rule]()


def seams(ya, nfft, rule, n):
    """the frames (numbered in the main call) on both sides of every seam the rule is about"""
    p = ya.plan_spgram(nfft, n)
    B, L, A = p.group, p.launch_frames, p.accum_slab
    out = []
    pair = lambda f: out.extend([f - 1, f]) if 0 < f < n else None
    if rule == "slab3+1":
        pair(3 * p.slab)
    elif rule in ("rows64", "rows65", "fold_ragged"):
        pair(32 // B * p.slab)                                   # partial rows 31 | 32: the first fold chunk's end
        if rule == "fold_ragged":
            pair((p.rows - 1) // 32 * 32 // B * p.slab)          # the ragged last fold chunk's first row
    elif rule in ("slab_above", "slab_cap"):
        pair(p.slab)
        pair((p.workgroups - 1) * p.slab)
    elif rule.startswith("cut+"):
        pair(L)
        pair(L + (A if A else p.slab))
    elif rule in ("acc+1", "2acc+1"):
        pair(A)
        pair(2 * A)
    elif rule == "stride":
        pair(p.workgroups * 256 // nfft)
        pair(p.workgroups * 256 // nfft + 1)
    return out


def rule_ops(g, n):
    pre = g.delay - 1
    main = (g.delay - pre) + (n - 1) * g.delay + (1 if g.delay > 1 else 0)
    return ([("write", pre)] if pre else []) + [("write_dev", main)]


def geometry_ops(ya, g):
    """a write shorter than the timer, a call of B + 2 transforms and a call long enough that frames lie wholly in x with
    all their nfft slots, 2 B + 3 transforms past that, ending off a transform where delay allows"""
    B = ya.plan_spgram(g.nfft, 1).group
    pre = min(g.delay - 1, 5)
    k1, k2 = B + 2, -(-(g.wlen + g.nfft) // g.delay) + 2 * B + 3
    c1 = (g.delay - pre) + (k1 - 1) * g.delay + (g.delay > 2)
    c2 = k2 * g.delay
    return ([("write", pre)] if pre else []) + [("write_dev", c1), ("write_dev", c2)]


def G(name, nfft, wlen, delay, why, win=HAMMING, spec="geometry"):
    return Row(name, nfft, wlen, delay, win, spec, GEOMETRY_KEYS.get(name), True, why)


def _rule_rows():
    rows = []
    keys = RULE_KEYS
    for nfft in FUSED:
        B = 4096 // nfft
        rules = ["one"] + (["group-1"] if B > 2 else []) + (["group", "group+1"] if B > 1 else ["group+1"])
        rules += ["slab3+1", "rows64", "rows65", "fold_ragged", "slab_above", "slab_cap"]
        for r in rules:
            if r == "slab_cap" and keys[(nfft, r)] == keys[(nfft, "slab_above")]:
                continue                                          # nfft 256: the first slab above the minimum is the cap
            real = r in ("rows64", "rows65", "fold_ragged", "slab3+1")
            rows.append(Row(f"{nfft}-{r}", nfft, 20, 9, HAMMING, r, keys[(nfft, r)], real, "fused: " + r))
    rows.append(Row("256-cut+37", 256, 8, 3, HAMMING, "cut+37", keys[(256, "cut+37")], False,
                    "fused: the 2^20-transform launch cut in one write_dev (about 512 MiB of scratch)"))
    for nfft in (2, 64, 100, 8192):
        for r in ("acc-1", "acc", "acc+1", "2acc+1"):
            rows.append(Row(f"{nfft}-{r}", nfft, min(nfft, 20), 9 if nfft > 2 else 1, HAMMING, r, keys[(nfft, r)], False,
                            "unfused: " + r))
    rows.append(Row("8192-stride", 8192, 16, 3, HAMMING, "stride", keys[(8192, "stride")], False,
                    "unfused: more than 8192 * 256 frame elements in one batch, the frame builder strides"))
    rows.append(Row("64-cut+33", 64, 8, 3, HAMMING, "cut+33", keys[(64, "cut+33")], False,
                    "unfused: the chunk cut of 8192 transforms at a small nfft"))
    rows.append(Row("131072-cut+5", 1 << 17, 16, 3, HAMMING, "cut+5", keys[(1 << 17, "cut+5")], False,
                    "unfused: the chunk cut of 2^25 / nfft transforms, four-step transforms"))
    return rows


# what plan_spgram reports for the main call of every rule row (test_spgram_ref_cpu.py checks each against the query)
RULE_KEYS = {
    (256, "one"): ("fused", 16, 16, 1, 16, 0, 1),
    (256, "group-1"): ("fused", 16, 16, 1, 16, 0, 1),
    (256, "group"): ("fused", 16, 16, 1, 16, 0, 1),
    (256, "group+1"): ("fused", 16, 16, 2, 32, 0, 1),
    (256, "slab3+1"): ("fused", 16, 16, 4, 64, 0, 1),
    (256, "rows64"): ("fused", 16, 16, 4, 64, 0, 1),
    (256, "rows65"): ("fused", 16, 16, 5, 80, 3, 1),
    (256, "fold_ragged"): ("fused", 16, 16, 9, 144, 5, 1),
    (256, "slab_above"): ("fused", 16, 32, 544, 8704, 272, 1),
    (256, "slab_cap"): ("fused", 16, 32, 544, 8704, 272, 1),
    (512, "one"): ("fused", 8, 8, 1, 8, 0, 1),
    (512, "group-1"): ("fused", 8, 8, 1, 8, 0, 1),
    (512, "group"): ("fused", 8, 8, 1, 8, 0, 1),
    (512, "group+1"): ("fused", 8, 8, 2, 16, 0, 1),
    (512, "slab3+1"): ("fused", 8, 8, 4, 32, 0, 1),
    (512, "rows64"): ("fused", 8, 8, 8, 64, 0, 1),
    (512, "rows65"): ("fused", 8, 8, 9, 72, 3, 1),
    (512, "fold_ragged"): ("fused", 8, 8, 17, 136, 5, 1),
    (512, "slab_above"): ("fused", 8, 16, 576, 4608, 144, 1),
    (512, "slab_cap"): ("fused", 8, 32, 800, 6400, 200, 1),
    (1024, "one"): ("fused", 4, 4, 1, 4, 0, 1),
    (1024, "group-1"): ("fused", 4, 4, 1, 4, 0, 1),
    (1024, "group"): ("fused", 4, 4, 1, 4, 0, 1),
    (1024, "group+1"): ("fused", 4, 4, 2, 8, 0, 1),
    (1024, "slab3+1"): ("fused", 4, 4, 4, 16, 0, 1),
    (1024, "rows64"): ("fused", 4, 4, 16, 64, 0, 1),
    (1024, "rows65"): ("fused", 4, 4, 17, 68, 3, 1),
    (1024, "fold_ragged"): ("fused", 4, 4, 33, 132, 5, 1),
    (1024, "slab_above"): ("fused", 4, 8, 640, 2560, 80, 1),
    (1024, "slab_cap"): ("fused", 4, 32, 928, 3712, 116, 1),
    (2048, "one"): ("fused", 2, 4, 1, 2, 0, 1),
    (2048, "group-1"): ("fused", 2, 4, 1, 2, 0, 1),
    (2048, "group"): ("fused", 2, 4, 1, 2, 0, 1),
    (2048, "group+1"): ("fused", 2, 4, 1, 2, 0, 1),
    (2048, "slab3+1"): ("fused", 2, 4, 4, 8, 0, 1),
    (2048, "rows64"): ("fused", 2, 4, 32, 64, 0, 1),
    (2048, "rows65"): ("fused", 2, 4, 33, 66, 3, 1),
    (2048, "fold_ragged"): ("fused", 2, 4, 65, 130, 5, 1),
    (2048, "slab_above"): ("fused", 2, 6, 854, 1708, 54, 1),
    (2048, "slab_cap"): ("fused", 2, 32, 992, 1984, 62, 1),
    (4096, "one"): ("fused", 1, 4, 1, 1, 0, 1),
    (4096, "group"): ("fused", 1, 4, 1, 1, 0, 1),
    (4096, "group+1"): ("fused", 1, 4, 1, 1, 0, 1),
    (4096, "slab3+1"): ("fused", 1, 4, 4, 4, 0, 1),
    (4096, "rows64"): ("fused", 1, 4, 64, 64, 0, 1),
    (4096, "rows65"): ("fused", 1, 4, 65, 65, 3, 1),
    (4096, "fold_ragged"): ("fused", 1, 4, 129, 129, 5, 1),
    (4096, "slab_above"): ("fused", 1, 5, 1024, 1024, 32, 1),
    (4096, "slab_cap"): ("fused", 1, 32, 1024, 1024, 32, 1),
    (256, "cut+37"): ("fused", 16, 32, 32768, 524288, 16384, 2),
    (2, "acc-1"): ("unfused", 1, 1, 1),
    (2, "acc"): ("unfused", 1, 1, 1),
    (2, "acc+1"): ("unfused", 1, 2, 1),
    (2, "2acc+1"): ("unfused", 1, 3, 1),
    (64, "acc-1"): ("unfused", 8, 1, 1),
    (64, "acc"): ("unfused", 8, 1, 1),
    (64, "acc+1"): ("unfused", 9, 2, 1),
    (64, "2acc+1"): ("unfused", 17, 3, 1),
    (100, "acc-1"): ("unfused", 13, 1, 1),
    (100, "acc"): ("unfused", 13, 1, 1),
    (100, "acc+1"): ("unfused", 13, 2, 1),
    (100, "2acc+1"): ("unfused", 26, 3, 1),
    (8192, "acc-1"): ("unfused", 992, 1, 1),
    (8192, "acc"): ("unfused", 1024, 1, 1),
    (8192, "acc+1"): ("unfused", 1056, 2, 1),
    (8192, "2acc+1"): ("unfused", 2080, 3, 1),
    (8192, "stride"): ("unfused", 8192, 10, 1),
    (64, "cut+33"): ("unfused", 2048, 256, 2),
    (131072, "cut+5"): ("unfused", 8192, 8, 2),
}

# the same for the largest call of every geometry row
GEOMETRY_KEYS = {
    "512-wlen=nfft": ("fused", 8, 8, 3, 24, 0, 1),
    "512-delay1": ("fused", 8, 8, 68, 544, 17, 1),
    "512-delay=wlen": ("fused", 8, 8, 3, 24, 0, 1),
    "512-wlen1": ("fused", 8, 8, 24, 192, 6, 1),
    "512-wlen<delay<nfft": ("fused", 8, 8, 3, 24, 0, 1),
    "512-delay>nfft": ("fused", 8, 8, 3, 24, 0, 1),
    "512-flattop": ("fused", 8, 8, 3, 24, 0, 1),
    "512-rcostaper": ("fused", 8, 8, 3, 24, 0, 1),
    "512-short-calls": ("fused", 8, 8, 2, 16, 0, 1),
    "512-reach-two-calls": ("fused", 8, 8, 5, 40, 0, 1),
    "512-clear": ("fused", 8, 8, 19, 152, 5, 1),
    "512-alpha-switch": ("fused", 8, 8, 19, 152, 5, 1),
    "512-push": ("fused", 8, 8, 19, 152, 5, 1),
    "512-reset": ("fused", 8, 8, 4, 32, 0, 1),
    "100-wlen=nfft": ("unfused", 4, 1, 1),
    "100-delay1": ("unfused", 46, 4, 1),
    "100-delay=wlen": ("unfused", 4, 1, 1),
    "100-wlen1": ("unfused", 16, 2, 1),
    "100-wlen<delay<nfft": ("unfused", 4, 1, 1),
    "100-delay>nfft": ("unfused", 3, 1, 1),
    "100-flattop": ("unfused", 4, 1, 1),
    "100-rcostaper": ("unfused", 4, 1, 1),
    "100-short-calls": ("unfused", 5, 1, 1),
    "100-reach-two-calls": ("unfused", 4, 1, 1),
    "100-clear": ("unfused", 17, 2, 1),
    "100-alpha-switch": ("unfused", 17, 2, 1),
    "100-push": ("unfused", 11, 1, 1),
    "100-reset": ("unfused", 3, 1, 1),
}

GEOMETRY = [row for nfft in (512, 100) for row in (
    G(f"{nfft}-wlen=nfft", nfft, nfft, nfft // 2 + 1, "wlen = nfft"),
    G(f"{nfft}-delay1", nfft, 12, 1, "delay = 1"),
    G(f"{nfft}-delay=wlen", nfft, nfft // 3, nfft // 3, "wlen < nfft, delay = wlen"),
    G(f"{nfft}-wlen1", nfft, 1, 3, "wlen = 1 (Triangular: Hamming is not defined at one tap)", TRIANGULAR),
    G(f"{nfft}-wlen<delay<nfft", nfft, nfft // 5, nfft // 2 + 1, "wlen < delay < nfft"),
    G(f"{nfft}-delay>nfft", nfft, nfft - 3, nfft + 77, "delay > nfft"),
    G(f"{nfft}-flattop", nfft, nfft // 2, nfft // 2 - 7,
      "FlatTop taper (its edge taps are near zero: delay near wlen keeps frame 0 visible)", FLATTOP),
    G(f"{nfft}-rcostaper", nfft, nfft - 1, nfft - 10, "RcosTaper taper (edge taps zero, as FlatTop)", RCOSTAPER),
    G(f"{nfft}-short-calls", nfft, nfft // 4, nfft // 11, "calls of fewer than nfft samples: every frame takes the rolled path",
      spec=(("write_dev", nfft - 1), ("write_dev", nfft // 2 + 3), ("write_dev", nfft - 2))),
    G(f"{nfft}-reach-two-calls", nfft, nfft // 4 + 5, 40,
      "two writes shorter than the timer, then a call whose first frames reach across both",
      spec=(("write", 15), ("write", 20), ("write_dev", 3 * nfft + 9))),
    G(f"{nfft}-clear", nfft, 60, 7, "clear between two writes, then a first frame again",
      spec=(("write", 200), ("write_dev", 300), ("clear",), ("write_dev", 2 * nfft + 11))),
    G(f"{nfft}-alpha-switch", nfft, 60, 7, "set_alpha switched between writes in both directions",
      spec=(("set_alpha", 0.05), ("write_dev", 300), ("set_alpha", -1.0), ("write_dev", 2 * nfft + 5),
            ("set_alpha", 0.03), ("write_dev", 250), ("set_alpha", -1.0))),
    G(f"{nfft}-push", nfft, 60, 7, "push of a few samples, then write_dev: the queue is flushed first",
      spec=(("write", 100), ("push", 5), ("write_dev", 2 * nfft + 1), ("push", 3))),
    G(f"{nfft}-reset", nfft, 60, 41, "reset: the window is zeroed, the timer and the counters restart",
      spec=(("write_dev", 300), ("reset",), ("write_dev", 2 * nfft + 13))))]

TABLE = _rule_rows() + GEOMETRY


def geometry(row):
    return sr.Geometry(row.nfft, row.wlen, row.delay, row.win)


def dtypes(row):
    return (np.complex64, np.float32) if row.real else (np.complex64,)


def fixed_modes(row):
    """rows whose operations set alpha themselves run once"""
    return isinstance(row.spec, tuple) and any(op[0] == "set_alpha" for op in row.spec)


def cases():
    return [(row, dt, mode) for row in TABLE for dt in dtypes(row)
            for mode in (("ops",) if fixed_modes(row) else MODES)]


def case_id(row, dt, mode):
    return f"{row.name}-{'cf' if dt is np.complex64 else 'f'}-{mode}"


Case = collections.namedtuple("Case", "g ops frames x alpha main sched")


def build_case(ya, row, dt, mode):
    """the operations of a case, its frames of interest and its sparse stream; main = transforms of the largest call"""
    g = geometry(row)
    if isinstance(row.spec, tuple):
        ops, sm = list(row.spec), []
    elif row.spec == "geometry":
        ops, sm = geometry_ops(ya, g), []
    else:
        n = count(ya, row.nfft, row.spec)
        ops, sm = rule_ops(g, n), seams(ya, row.nfft, row.spec, n)
    s = sr.schedule(g, ops)
    alpha = None
    if mode == "rec":
        alpha = float(np.float32(min(0.3, 1.5 / max(1, len(s.end)))))
        ops = [("set_alpha", alpha)] + ops + [("set_alpha", -1.0)]
        s = sr.schedule(g, ops)
    B = ya.plan_spgram(row.nfft, 1).group
    i_main, f_main, k_main = max(s.call_frames, key=lambda c: c[2])
    wr = [c for c in s.call_frames if c[2]]
    last_call = wr[-1]
    x0 = sum(int(op[1]) for op in ops[:last_call[0]] if op[0] in sr.WRITES)      # first sample of the last call
    inside = [j for j in range(last_call[1], last_call[1] + last_call[2]) if s.end[j] - (g.wlen - 1) >= x0][:1]
    # in order of precedence: the last frame of every call, the first frame since the last clear, frame 0, the seams, the
    # last full group, the first frame in x
    want = [c[1] + c[2] - 1 for c in wr] + [s.live0, 0] + [f_main + f for f in sm]
    want += [last_call[1] + last_call[2] // B * B - 1] if last_call[2] >= B else []
    want += inside
    frames = []
    for j in want:
        if j not in frames and len(frames) < 8:
            frames.append(int(j))
    seed = 9000 + 7 * row.nfft + 13 * g.wlen + g.delay + len(row.name)
    frames = sorted(frames)
    # a first transform after a clear carries 1 where the others carry alpha: its burst is scaled down until its weight
    # is the median of the frames of interest, or it would be all the estimate shows
    wt = np.ones(len(frames))
    live = [i for i, j in enumerate(frames) if j >= s.live0]
    wt[live] = sr.weights(s)[[frames[i] - s.live0 for i in live]]
    gains = np.sqrt(np.minimum(1.0, np.median(wt[live]) / wt))
    x = sr.sparse_stream(dt, g, frames, seed, ops=ops, gains=gains)
    return Case(g, ops, frames, x, alpha, k_main, s)
