"""PreambleDetector on the GPU against tests/pdet_ref.py, byte for byte: events, overflow, pending and position after
every call, on the streams and cuts that tests/test_pdet_ref_cpu.py proves to reach every path of pdet_kernels.hip (T = the
tile): detections inside a tile and across seams, alone (L >= 64), beside a few one-sample noise runs per tile (L = 16)
and inside crowded tiles (L <= 8), plateaus with tied peaks over three tiles, runs ending
on a tile's last sample, starting on its first, pending over a call seam, calls shorter than the carried history.  Then
the chunking property, the bank's raw output against the reference's sums, the fused path against the reference's
detection on the GPU's own correlate_block, getters / flush / clone / reset, a short events buffer, the capacity
boundary, a NaN and an Inf inside a run, an energy floor, duplicate hypotheses, and the argument checks.  The reference
is given the library's own templates, so no libm decides a comparison."""
import numpy as np
import pytest

import nonfinite_util as nfu
import pdet_ref as pr

pytestmark = pytest.mark.gpu
T = pr.TILE
CASES = [(n, f) for f in pr.FAMILIES for n in pr.NAMES]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.PDET_TILE == T
    return yagi_amd


def gpu(ya, name, family, **kw):
    p, dphi, *_ = pr.case(name, family, ya.preamble_templates)
    return ya.PreambleDetector(p, dphi, kw.get("threshold", pr.THRESHOLD), kw.get("energy_floor", 0.0),
                               kw.get("min_length", 1))


@pytest.mark.parametrize("label", pr.LABELS)
@pytest.mark.parametrize("name,family", CASES)
def test_every_call_equals_the_reference_and_the_cut_does_not_matter(ya, name, family, label):
    _, _, x, _, runs, cuts = pr.case(name, family, ya.preamble_templates)
    q = gpu(ya, name, family)
    got = pr.run_calls(q, x, cuts[label])
    assert all(r[0].dtype == pr.EVENT for r in got)
    assert pr.same(got, pr.want(name, family, label, ya.preamble_templates)), (name, family, label)
    whole = np.concatenate([r[0] for r in got] + [q.flush()])
    assert whole.tobytes() == runs.tobytes()                        # the chunking property: the one-call list
    assert q.pending is None and q.position == x.size


@pytest.mark.parametrize("name,family", CASES)
def test_correlate_block_equals_the_references_sums(ya, name, family):
    _, _, x, make, _, cuts = pr.case(name, family, ya.preamble_templates)
    q, ref = gpu(ya, name, family), make().co.clone()
    ref.reset()
    for lens in (cuts["T+1"], cuts["small"][:3]):                   # the second: calls shorter than the history
        for part in pr.cut(x[:sum(lens)], lens):
            got, want = q.correlate_block(part), ref.correlate_block(part)
            assert got[0].dtype == np.complex64 and got[1].dtype == np.float32
            assert pr.same_sums(got, want), (name, family, part.size)
        assert q.position == sum(lens) and q.pending is None
        q.reset()
        ref.reset()


@pytest.mark.parametrize("name,family", CASES)
def test_fused_path_equals_the_detection_on_the_gpus_own_sums(ya, name, family):
    _, _, x, make, _, cuts = pr.case(name, family, ya.preamble_templates)
    composed = make(correlator=gpu(ya, name, family))               # the reference's detection on correlate_block's output
    want = pr.run_calls(composed, x, cuts["T+1"])
    assert pr.same(pr.run_calls(gpu(ya, name, family), x, cuts["T+1"]), want)


def test_getters_flush_clone_and_reset(ya):
    name, family = "L16", "plateau"
    p, dphi, x, make, runs, cuts = pr.case(name, family, ya.preamble_templates)
    q, r = gpu(ya, name, family, min_length=8), make(min_length=8)
    assert (q.length, q.hypotheses, q.min_length) == (16, 3, 8)
    assert q.threshold == np.float32(pr.THRESHOLD) and q.energy_floor == np.float32(0.0)
    assert q.preamble_energy == pr.preamble_energy(p) and q.dphi.tobytes() == dphi.tobytes()
    V = q.get_templates()
    assert V.tobytes() == ya.preamble_templates(p, dphi).tobytes() == r.co.V.tobytes()
    assert q.pending is None and q.position == 0 and q.flush().size == 0
    s = cuts["start"][0]
    mid = s + 40                                                    # inside the longest run
    for o in (q, r):
        o.detect_block(x[:mid])
    assert r.pending is not None and r.pending["start"] == s
    assert q.pending.tobytes() == r.pending.tobytes()
    q2, r2 = q.clone(), r.clone()                                   # mid-run: history, pending run and counter
    assert q2.pending.tobytes() == r.pending.tobytes() and q2.position == mid
    assert q2.get_templates().tobytes() == V.tobytes() and q2.min_length == 8
    for o, w in ((q, r), (q2, r2)):
        got, want = o.detect_block(x[mid:]), w.detect_block(x[mid:])
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
        assert o.position == x.size
    q3, r3 = gpu(ya, name, family), make()
    for o in (q3, r3):
        o.detect_block(x[:mid])
    got, want = q3.flush(), r3.flush()                              # the pending run closes, the counter stays
    assert got.size == 1 and got.tobytes() == want.tobytes() and got["length"][0] == 40
    assert q3.pending is None and q3.position == mid and q3.flush().size == 0
    a, b = q3.detect_block(x[mid:]), r3.detect_block(x[mid:])       # the rest of the run is a run of its own
    assert a[0].tobytes() == b[0].tobytes() and a[0]["start"][0] == mid
    short = gpu(ya, name, family, min_length=41)                    # a flushed run shorter than min_length is no event
    short.detect_block(x[:mid])
    assert short.pending is not None and short.flush().size == 0 and short.pending is None
    q.reset()
    assert q.position == 0 and q.pending is None
    r.reset()
    assert pr.same(pr.run_calls(q, x, cuts["one"]), pr.run_calls(r, x, cuts["one"]))


def test_a_short_events_buffer_truncates_and_reports_the_total(ya):
    _, _, x, make, _, _ = pr.case("L5", "noise", ya.preamble_templates)
    want, _ = make().detect_block(x)
    assert want.size > 300
    for cap in (0, 1, 7, want.size, want.size + 5):
        ev, over, count = gpu(ya, "L5", "noise").detect_block(x, cap=cap)
        assert count == want.size and not over
        assert ev.tobytes() == want[:cap].tobytes()


ONE = np.ones(1, np.complex64)


def lone(ya):
    """L = 1, K = 1, p = [1]: r = 1 wherever there is energy"""
    V = ya.preamble_templates(ONE, [0.0])
    return ya.PreambleDetector(ONE, [0.0], 0.5), pr.PreambleDetector(ONE, V, 0.5)


# on 1, 0, 1, 0, ... n samples hold ceil(n / 2) segments in ceil(n / T) tiles
def _boundary(delta):
    n = next(n for n in range(2 * pr.SEGMAX, 4 * pr.SEGMAX + 4 * T, 2)
             if (n + 1) // 2 - ((n + T - 1) // T + pr.SEGMAX) == delta)
    return n


@pytest.mark.parametrize("label,delta,over", [("below", -1, False), ("at", 0, False), ("above", 1, True)])
def test_capacity_boundary(ya, label, delta, over):
    n = _boundary(delta)
    x = pr.alternating(n + 4)
    q, r = lone(ya)
    want = pr.run_calls(r, x, (n, 4))
    assert want[0][1] == over and want[0][0].size == (0 if over else (n + 1) // 2)
    assert want[1][0].size == 2 and not want[1][1]
    assert pr.same(pr.run_calls(q, x, (n, 4)), want)


def test_overflow_drops_the_pending_run_and_the_stream_goes_on(ya):
    n = _boundary(1) + 1                                            # ends on a 1: a run is pending there
    x = pr.alternating(n)
    x[0] = 0
    x = np.concatenate([np.ones(3, np.complex64), x, np.ones(2, np.complex64), np.array([1, 0], np.complex64)])
    lens = (3, n + 2, 2)
    q, r = lone(ya)
    want = pr.run_calls(r, x, lens)
    assert want[0][2] is not None and want[1][1] and want[1][2] is None and want[2][0]["start"][0] == n + 5
    assert pr.same(pr.run_calls(q, x, lens), want)


@pytest.mark.parametrize("value", ["nan", "+inf"])
@pytest.mark.parametrize("name", ["L16", "L257"])
def test_a_non_finite_sample_inside_a_run(ya, name, value):
    p, _, x, make, runs, cuts = pr.case(name, "plateau", ya.preamble_templates)
    s, e = int(runs[0]["start"]), int(runs[0]["start"] + runs[0]["length"])
    at = s + 700                                                    # in the first tile, the run goes on for two more
    xp = nfu.poison(x, at, value, "re")
    lens = (T + 1, x.size - T - 1)
    want = pr.run_calls(make(), xp, lens)
    flat = np.concatenate([w[0] for w in want])
    assert not ((flat["start"] <= at) & (flat["start"] + flat["length"] > at)).any()   # no run holds the sample
    assert ((flat["start"] == s) & (flat["length"] == at - s)).any()             # the run ends in front of it
    assert (flat["start"] == at + p.size).any()                                 # and starts again behind its window
    assert pr.same(pr.run_calls(gpu(ya, name, "plateau"), xp, lens), want)


def test_an_energy_floor_silences_everything(ya):
    p, dphi, x, make, runs, _ = pr.case("L64", "noise", ya.preamble_templates)
    for floor in (100.0, 1e9):
        want = pr.run_calls(make(energy_floor=floor), x, (T + 1, x.size - T - 1))
        got = pr.run_calls(gpu(ya, "L64", "noise", energy_floor=floor), x, (T + 1, x.size - T - 1))
        assert pr.same(got, want)
    assert sum(w[0].size for w in want) == 0
    floor = float(runs["energy"].min()) - 0.5                      # just below the weakest detection: all four stay
    want = pr.run_calls(make(energy_floor=floor), x, (x.size,))
    assert want[0][0].size == 4
    assert pr.same(pr.run_calls(gpu(ya, "L64", "noise", energy_floor=floor), x, (x.size,)), want)


def test_duplicate_hypotheses_report_the_lower_index(ya):
    p, _, x, _, runs, _ = pr.case("L64", "noise", ya.preamble_templates)
    dphi = np.array([0.1, -0.1, 0.0, -0.1, 0.1, 0.0], np.float32)
    q = ya.PreambleDetector(p, dphi, pr.THRESHOLD)
    V = q.get_templates()
    assert V[0].tobytes() == V[4].tobytes() and V[1].tobytes() == V[3].tobytes()
    ref = pr.PreambleDetector(p, V, pr.THRESHOLD)
    want = pr.run_calls(ref, x, (T - 1, x.size - T + 1))
    flat = np.concatenate([w[0] for w in want])
    assert flat["peak"].tolist()[:3] == runs["peak"].tolist()[:3] and flat["hypothesis"].tolist()[:3] == [1, 2, 0]
    assert pr.same(pr.run_calls(q, x, (T - 1, x.size - T + 1)), want)


def test_bad_arguments_are_config_errors_and_an_empty_call_is_a_no_op(ya):
    p = np.exp(1j * np.pi / 2 * np.arange(8)).astype(np.complex64)
    nan, inf = float("nan"), float("inf")
    for args in [(p[:0], [0.0], 0.5), (np.ones(ya.PDET_LMAX + 1, np.complex64), [0.0], 0.5), (p, [], 0.5),
                 (p, np.zeros(ya.PDET_KMAX + 1, np.float32), 0.5), (p, [nan], 0.5), (p, [inf], 0.5),
                 (np.zeros(8, np.complex64), [0.0], 0.5), (p, [0.0], 0.0), (p, [0.0], -1.0), (p, [0.0], nan),
                 (p, [0.0], inf), (p, [0.0], 0.5, -1.0), (p, [0.0], 0.5, inf), (p, [0.0], 0.5, 0.0, 0)]:
        with pytest.raises(ya.ConfigError):
            ya.PreambleDetector(*args)
    with pytest.raises(ya.ConfigError):
        ya.PreambleDetector(p, [0.0], 0.5, kind="rrrf")
    ya.PreambleDetector(np.ones(ya.PDET_LMAX, np.complex64), np.zeros(ya.PDET_KMAX, np.float32), 0.5, 0.0, 2 ** 40)
    q = ya.PreambleDetector(p, [0.0, 0.1], 0.5)
    ev, over = q.detect_block(np.zeros(0, np.complex64))            # an empty call is a no-op
    assert ev.size == 0 and not over and q.position == 0
    rxy, en = q.correlate_block(np.zeros(0, np.complex64))
    assert rxy.shape == (2, 0) and en.size == 0 and q.position == 0
