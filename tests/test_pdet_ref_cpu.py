"""tests/pdet_ref.py against itself and against the library's host forms, no GPU needed: the vectorised bank and detection
equal the composition of oracle.Window and oracle.dotprod with a per-sample state machine byte for byte on every shape
and both stream families; the library's own host form (preamble_detect_host) gives the same events on every shape and
cut; preamble_templates is within 1 f32 ulp of a numpy-f64 evaluation and conj(p) at dphi = 0; and the streams provably
reach what they are meant to reach (asserted on the reference, T = the tile): in noise exactly the four preambles at
L = 64, 257 and 1024, at start + L - 1 with the expected hypotheses, ratios 0.86 to 0.93 and noise below 0.16; the four
preambles among hundreds of noise runs per tile at L = 5 and 8 and among the several per tile that Gaussian noise gives
at L = 16; on the plateaus runs with tied peaks that cross one seam, span three tiles, end on a tile's last sample,
start on its first and stay pending over a call seam."""
import numpy as np
import pytest

import pdet_ref as pr

T = pr.T
CASES = [(n, f) for f in pr.FAMILIES for n in pr.NAMES]


def lib_templates(p, dphi):
    import yagi_amd as ya
    return ya.preamble_templates(p, dphi)


def events_of(results):
    return np.concatenate([r[0] for r in results])


@pytest.mark.parametrize("name,family", CASES)
def test_fast_and_slow_forms_agree(oracle, name, family):
    p, dphi, x, make, runs, cuts = pr.case(name, family, lib_templates)
    V = make().co.V
    fast, slow = pr.Correlator(V), pr.SlowCorrelator(oracle, V)
    lens = cuts["T+1"]
    sums = [[c.correlate_block(part) for part in pr.cut(x, lens)] for c in (fast, slow)]
    assert all(pr.same_sums(a, b) for a, b in zip(*sums))
    for label in ("one", "pending"):
        # the slow form end to end: the state machine on Window + dotprod's own sums (the long shapes take them for the
        # whole stream once, above, and run the state machine on the fast sums that were just proven equal)
        short = p.size * dphi.size <= 1024 and (p.size <= 64 or label == "pending")
        own = pr.SlowCorrelator(oracle, V) if short else None
        got = pr.run_calls(make(cls=pr.SlowPreambleDetector, correlator=own), x, cuts[label])
        assert pr.same(got, pr.want(name, family, label, lib_templates)), (name, family, label)


@pytest.mark.parametrize("name,family", CASES)
def test_the_cut_does_not_matter(name, family):
    p, dphi, x, make, runs, cuts = pr.case(name, family, lib_templates)
    for label in pr.LABELS:
        det = make()
        got = pr.run_calls(det, x, cuts[label])
        assert not any(r[1] for r in got)
        whole = np.concatenate([events_of(got), det.flush()])
        assert whole.tobytes() == runs.tobytes(), (name, family, label)
        assert det.position == x.size and det.pending is None


@pytest.mark.parametrize("name,family", CASES)
def test_the_librarys_host_form_equals_the_reference(name, family):
    import yagi_amd as ya
    p, dphi, x, make, runs, cuts = pr.case(name, family, lib_templates)
    ends = sorted({x.size} | {lens[0] for lens in cuts.values()})   # a stream from reset() up to every first cut
    for n in ends:
        det = make()
        want, over = det.detect_block(x[:n])
        ev, o, pend = ya.preamble_detect_host(x[:n], p, dphi, pr.THRESHOLD)
        assert ev.dtype == pr.EVENT and ev.tobytes() == want.tobytes() and o == over, (name, family, n)
        assert (pend is None) == (det.pending is None)
        if pend is not None:
            assert pend.tobytes() == det.pending.tobytes()
    det = make(min_length=2)
    want, _ = det.detect_block(x)
    ev, _, _ = ya.preamble_detect_host(x, p, dphi, pr.THRESHOLD, 0.0, 2)
    assert ev.tobytes() == want.tobytes()


def test_the_librarys_host_form_applies_the_capacity_rule_and_the_floor():
    import yagi_amd as ya
    one = np.ones(1, np.complex64)
    for n in (8 * T + 16, 8 * T + 18, 8 * T + 20):
        over = (n + 1) // 2 > (n + T - 1) // T + pr.SEGMAX
        ev, o, _ = ya.preamble_detect_host(pr.alternating(n), one, [0.0], 0.5)
        assert o == over and ev.size == (0 if over else (n + 1) // 2)
    ev, o, pend = ya.preamble_detect_host(pr.alternating(100), one, [0.0], 0.5, 2.0)
    assert ev.size == 0 and not o and pend is None


def _ulp_apart(a, b):
    """distance in f32 units in the last place of a, b a float64 array"""
    a64 = a.astype(np.float64)
    return np.abs(a64 - b) / np.spacing(np.maximum(np.abs(a), np.float32(2.0 ** -126))).astype(np.float64)


@pytest.mark.parametrize("name", pr.NAMES)
def test_templates_are_the_f64_evaluation_rounded_once(name):
    import yagi_amd as ya
    p, dphi, *_ = pr.case(name, "noise", lib_templates)
    rng = np.random.default_rng(p.size)
    p = (p * rng.uniform(0.5, 2.0, p.size)).astype(np.complex64)   # parts that are not 0 or +-1
    V = ya.preamble_templates(p, dphi)
    assert V.dtype == np.complex64 and V.shape == (dphi.size, p.size)
    want = pr.templates_f64(p, dphi)
    # one rounding of a value that numpy's f64 gives to within an f64 ulp or two: 1 ulp of f32 bounds it
    assert _ulp_apart(V.real, want.real).max() <= 1.0 and _ulp_apart(V.imag, want.imag).max() <= 1.0
    zero = ya.preamble_templates(p, np.zeros(3, np.float32))
    assert all(np.array_equal(row, np.conj(p)) for row in zero)
    assert np.array_equal(ya.preamble_templates(p, dphi[::-1].copy()), V[::-1])   # the caller's order


@pytest.mark.parametrize("name", ["L64", "L257", "L1024"])
def test_noise_streams_hold_exactly_the_four_preambles(name):
    p, dphi, x, make, runs, _ = pr.case(name, "noise", lib_templates)
    L, K = p.size, dphi.size
    starts = pr.preamble_starts(L)
    assert runs.size == 4 and (runs["length"] == 1).all()
    assert runs["peak"].tolist() == [s + L - 1 for s in starts]
    assert runs["hypothesis"].tolist() == [0, K // 2, K - 1, 1]
    assert ((runs["ratio"] >= 0.86) & (runs["ratio"] <= 0.93)).all()
    ends = [s + L - 1 for s in starts]
    assert ends[0] // T == starts[0] // T and ends[0] % T != T - 1           # inside a tile
    assert all(ends[i] // T == starts[i] // T + 1 for i in (1, 2))           # these end across a tile seam
    assert ends[3] == x.size - 8                                             # 7 samples follow it
    rxy, en = make().co.correlate_block(x)
    away = np.ones(x.size, bool)
    for s in starts:
        away[s:s + 2 * L] = False
    with np.errstate(all="ignore"):
        m = (rxy.real * rxy.real + rxy.imag * rxy.imag).max(axis=0)
        noise = (m / (en * pr.preamble_energy(p)))[away & (en > 0)]
    assert noise.max() <= 0.16                                               # the threshold's 0.36 is far off


def test_noise_streams_at_small_lengths_crowd_their_tiles():
    """What noise alone does at threshold 0.6 follows from L, not from the noise level (r is a ratio): for Gaussian noise
    r of one hypothesis is Beta(1, L - 1), so P(r > 0.36) = 0.64^(L-1).  At L = 5 and 8 that is 0.17 and 0.044 per
    hypothesis: hundreds of runs per tile, among which the four preambles still stand as runs of their own.  At L = 16,
    K = 3 it is 1 - (1 - 0.64^15)^3 = 0.0037 per sample, 7.6 expected per tile of 2048 and about 25 in the stream: every
    tile holds several one-sample noise runs beside the detections, and no noise level gives more."""
    per_tile, noise_runs = {}, {}
    for name in ("L1", "L5", "L8", "L16"):
        p, dphi, x, _, runs, _ = pr.case(name, "noise", lib_templates)
        L, K = p.size, dphi.size
        per_tile[name] = np.bincount((runs["start"] // T).astype(int), minlength=4)
        peaks = [s + L - 1 for s in pr.preamble_starts(L)]
        found = runs[np.isin(runs["peak"], peaks)]
        rest = runs[~np.isin(runs["peak"], peaks)]
        noise_runs[name] = np.bincount((rest["start"] // T).astype(int), minlength=4)
        if name != "L1":
            # the four detections are runs of one sample among the noise runs of their tiles
            assert found["peak"].tolist() == peaks and (found["length"] == 1).all() and (found["ratio"] > 0.8).all()
            assert (found["peak"] // T).tolist() == [0, 1, 2, 3]
        if name in ("L5", "L16"):                                # at L = 8 the 32 hypotheses are too close to tell
            assert found["hypothesis"].tolist() == [0, K // 2, K - 1, 1]
        if name == "L16":
            assert (rest["length"] == 1).all()
    assert per_tile["L1"][:3].min() > 250                                    # runs of six between the zeros
    assert noise_runs["L5"][:3].min() > 300 and noise_runs["L8"][:3].min() > 150   # crowded tiles, a detection in each
    assert noise_runs["L16"].min() >= 5 and 20 <= noise_runs["L16"].sum() <= 36    # 7.6 a tile expected, 25 in all
    assert len({int(h) for h in pr.case("L8", "noise", lib_templates)[4]["hypothesis"]}) > 8


def test_plateau_streams_reach_every_path():
    reached = set()
    for name in pr.NAMES:
        p, dphi, x, make, runs, cuts = pr.case(name, "plateau", lib_templates)
        L = p.size
        assert dphi[0] == 0 and runs.size == 2 and (runs["hypothesis"] == 0).all()
        for r in runs:
            s, e = int(r["start"]), int(r["start"] + r["length"])
            if (e - 1) // T == s // T + 1:
                reached.add("across one seam")
            if (e - 1) // T >= s // T + 2:
                reached.add("three tiles")
            if e == x.size:
                reached.add("pending at the stream's end")
        first = runs[0]
        if L < 1024:
            # r climbs as (j + 1) / L to exactly 1 and stays: the peak is the first sample with a full window
            assert first["ratio"] == 1.0 and first["peak"] == pr.plateau_spans(L)[0][0] + L - 1
            assert first["length"] > 1000
            rxy, en = make().co.correlate_block(x)
            with np.errstate(all="ignore"):
                r = (rxy[0].real ** 2 + rxy[0].imag ** 2) / (en * pr.preamble_energy(p))
            assert (r[int(first["peak"]):int(first["peak"]) + 1000] == 1.0).all()   # tied: the earliest is reported
        s, e = cuts["start"][0], cuts["pending"][0]
        second = pr.want(name, "plateau", "start", lib_templates)[1]
        assert pr.want(name, "plateau", "start", lib_templates)[0][2] is None
        if second[0].size and second[0]["start"][0] == s:
            reached.add("starts on a tile's first sample")
        at = cuts["end"][0]
        if (e - at) % T == 0 and e - at > 0:
            reached.add("ends on a tile's last sample")
        pend = pr.want(name, "plateau", "pending", lib_templates)
        if pend[0][2] is not None and pend[0][2]["start"] == s and pend[0][2]["length"] == e - s \
                and pend[1][0].size and pend[1][0]["start"][0] == s and pend[1][0]["length"][0] == e - s:
            reached.add("pending over a call seam")
    assert reached == {"across one seam", "three tiles", "pending at the stream's end", "starts on a tile's first sample",
                       "ends on a tile's last sample", "pending over a call seam"}, reached


def test_ties_between_hypotheses_keep_the_lowest_and_nan_gives_no_hit():
    p = np.exp(1j * np.pi / 2 * np.arange(8) ** 2 / 3).astype(np.complex64)
    dphi = np.array([0.1, 0.05, 0.05, 0.1, 0.05], np.float32)
    V = lib_templates(p, dphi)
    assert V[1].tobytes() == V[2].tobytes() == V[4].tobytes()
    x = np.zeros(64, np.complex64)
    x[10:18] = p * np.exp(1j * 0.05 * np.arange(8)).astype(np.complex64)
    x[30:38] = p * np.exp(1j * 0.1 * np.arange(8)).astype(np.complex64)
    for cls in (pr.PreambleDetector, pr.SlowPreambleDetector):
        ev, _ = cls(p, V, 0.9).detect_block(x)
        assert ev["peak"].tolist() == [17, 37] and ev["hypothesis"].tolist() == [1, 0]
        xn = x.copy()
        xn[14] = np.nan
        ev, _ = cls(p, V, 0.9).detect_block(xn)
        assert ev["peak"].tolist() == [37]
