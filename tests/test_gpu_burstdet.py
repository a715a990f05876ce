"""BurstDetector on the GPU against tests/burstdet_ref.py, byte for byte: events, overflow, pending and position after every
call, on the streams and cuts that tests/test_burstdet_ref_cpu.py proves to reach every path of burstdet_kernels.hip (T =
the tile): runs inside a tile, across seams, over three tiles, ending on a tile's last sample, starting on its first,
pending over a call seam, a tile with hundreds of runs, calls shorter than the carried history.  Then the chunking
property, flush / clone / reset, the fused path against the composition on the GPU's own Autocorr, a short events
buffer, the capacity boundary, a NaN and an Inf inside a burst, one isolated run per tile with empty tiles between (the
stitch kernel's path for scattered runs), and the argument checks."""
import numpy as np
import pytest

import burstdet_ref as bdr
import nonfinite_util as nfu

pytestmark = pytest.mark.gpu
T = bdr.TILE
KINDS = ("cccf", "rrrf")
NAMES = [s[0] for s in bdr.SHAPES]
LABELS = ("one", "1", "T-1", "T", "T+1", "small", "start", "end", "pending")


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def gpu(ya, kind, name, **kw):
    _, W, d, _, thr, minlen, _ = next(s for s in bdr.SHAPES if s[0] == name)
    return ya.BurstDetector(kind, W, d, thr, 0.0, kw.get("min_length", minlen))


@pytest.mark.parametrize("label", LABELS)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_call_equals_the_reference_and_the_cut_does_not_matter(ya, kind, name, label):
    x, _, runs, cuts = bdr.case(kind, name)
    q = gpu(ya, kind, name)
    got = bdr.run_calls(q, x, cuts[label])
    assert all(r[0].dtype == bdr.EVENT for r in got)
    assert bdr.same(got, bdr.want(kind, name, label)), (kind, name, label)
    whole = np.concatenate([r[0] for r in got] + [q.flush()])
    assert whole.tobytes() == runs.tobytes()                        # the chunking property: the one-call list
    assert q.pending is None and q.position == x.size


@pytest.mark.parametrize("kind", KINDS)
def test_getters_flush_clone_and_reset(ya, kind):
    x, make, runs, cuts = bdr.case(kind, "W16")
    q, r = gpu(ya, kind, "W16"), make()
    assert (q.window_size, q.delay, q.min_length) == (16, 16, 8)
    assert q.threshold == np.float32(0.5) and q.energy_floor == np.float32(0.0)
    assert q.pending is None and q.position == 0 and q.flush().size == 0
    s, _ = cuts["start"]
    mid = s + 40                                                    # inside the longest run
    for o in (q, r):
        o.detect_block(x[:mid])
    assert r.pending is not None and r.pending["start"] == s
    assert q.pending.tobytes() == r.pending.tobytes()
    q2, r2 = q.clone(), r.clone()                                   # mid-run: history, pending run and counter
    assert q2.pending.tobytes() == r.pending.tobytes() and q2.position == mid
    for o, w in ((q, r), (q2, r2)):
        got, want = o.detect_block(x[mid:]), w.detect_block(x[mid:])
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
        assert o.position == x.size
    q3, r3 = gpu(ya, kind, "W16"), make()
    for o in (q3, r3):
        o.detect_block(x[:mid])
    got, want = q3.flush(), r3.flush()                              # the pending run closes, the counter stays
    assert got.size == 1 and got.tobytes() == want.tobytes() and got["length"][0] == 40
    assert q3.pending is None and q3.position == mid and q3.flush().size == 0
    a, b = q3.detect_block(x[mid:]), r3.detect_block(x[mid:])       # the rest of the run is a run of its own
    assert a[0].tobytes() == b[0].tobytes() and a[0]["start"][0] == mid
    short = gpu(ya, kind, "W16", min_length=41)                     # a flushed run shorter than min_length is no event
    short.detect_block(x[:mid])
    assert short.pending is not None and short.flush().size == 0 and short.pending is None
    q.reset()
    assert q.position == 0 and q.pending is None
    got = bdr.run_calls(q, x, cuts["one"])
    assert bdr.same(got, bdr.want(kind, "W16", "one"))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_fused_path_equals_the_composition_on_the_gpu(ya, kind, name):
    x, make, _, cuts = bdr.case(kind, name)
    _, W, d, *_ = next(s for s in bdr.SHAPES if s[0] == name)
    composed = make(autocorr=ya.Autocorr(kind, W, d))               # the reference's detection on Autocorr's own output
    want = bdr.run_calls(composed, x, cuts["T+1"])
    assert bdr.same(bdr.run_calls(gpu(ya, kind, name), x, cuts["T+1"]), want)


def test_a_short_events_buffer_truncates_and_reports_the_total(ya):
    x, make, _, _ = bdr.case("cccf", "W1")
    want, _ = make().detect_block(x)
    assert want.size > 300
    for cap in (0, 1, 7, want.size, want.size + 5):
        ev, over, count = gpu(ya, "cccf", "W1").detect_block(x, cap=cap)
        assert count == want.size and not over
        assert ev.tobytes() == want[:cap].tobytes()


# W = 1, d = 0 on 1, 0, 1, 0, ...: ceil(n / 2) segments in ceil(n / T) tiles (tests/test_burstdet_ref_cpu.py)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("label,n,over", [("below", 8 * T + 16, False), ("at", 8 * T + 18, False),
                                          ("above", 8 * T + 20, True)])
def test_capacity_boundary(ya, kind, label, n, over):
    x = bdr.alternating(kind, n + 4)
    want = bdr.run_calls(bdr.BurstDetector(kind, 1, 0, 0.5), x, (n, 4))
    assert want[0][1] == over and want[0][0].size == (0 if over else (n + 1) // 2)
    got = bdr.run_calls(ya.BurstDetector(kind, 1, 0, 0.5), x, (n, 4))
    assert bdr.same(got, want)


def test_overflow_drops_the_pending_run_and_the_stream_goes_on(ya):
    n = 8 * T + 21
    x = bdr.alternating("cccf", n)
    x[0] = 0
    x = np.concatenate([np.ones(3, np.complex64), x, np.ones(2, np.complex64), np.array([1, 0], np.complex64)])
    lens = (3, n + 2, 2)
    want = bdr.run_calls(bdr.BurstDetector("cccf", 1, 0, 0.5), x, lens)
    assert want[0][2] is not None and want[1][1] and want[1][2] is None and want[2][0]["start"][0] == n + 5
    assert bdr.same(bdr.run_calls(ya.BurstDetector("cccf", 1, 0, 0.5), x, lens), want)


@pytest.mark.parametrize("value", ["nan", "+inf"])
def test_a_non_finite_sample_inside_a_burst(ya, value):
    x, make, runs, cuts = bdr.case("cccf", "W16")
    s, _ = cuts["start"]
    e = next(int(r["start"] + r["length"]) for r in runs if r["start"] == s)
    at = (s + e) // 2
    xp = nfu.poison(x, at, value, "re")
    lens = (T + 1, x.size - T - 1)
    want = bdr.run_calls(make(), xp, lens)
    flat = np.concatenate([w[0] for w in want])
    before = runs[runs["start"] + runs["length"] <= at]
    assert before.size and flat[:before.size].tobytes() == before.tobytes()     # what closed before it is unchanged
    assert not ((flat["start"] <= at) & (flat["start"] + flat["length"] > at)).any()   # no run holds the sample
    assert ((flat["start"] == s) & (flat["length"] == at - s)).any()             # the burst's run ends in front of it
    assert bdr.same(bdr.run_calls(gpu(ya, "cccf", "W16"), xp, lens), want)


@pytest.mark.parametrize("kind", KINDS)
def test_one_short_run_per_tile_with_empty_tiles_between(ya, kind):
    """silence with a burst inside every other tile, one of them shorter than min_length: every tile that has a
    segment has exactly one, and it touches neither edge of its tile (the stitch kernel reports such tiles together)"""
    n, W = 9 * T + 100, 16
    x = np.zeros(n, bdr.acr.DTYPES[kind])
    for k in range(0, 9, 2):
        length = 60 if k == 4 else 200 + 10 * k
        x[k * T + 300 + k:k * T + 300 + k + length] = bdr.bursts(kind, W, W, length, [(0, length)], seed=k)[:length]
    ref = bdr.BurstDetector(kind, W, W, 0.5, 0.0, 1)
    every, _ = ref.detect_block(x)
    tiles = every["start"] // T
    assert every.size == 5 and len(set(tiles.tolist())) == 5 and ref.pending is None
    assert ((every["start"] % T != 0) & ((every["start"] + every["length"]) // T == tiles)).all()
    assert (every["length"] < 100).sum() == 1
    for minlen, cap in ((1, None), (100, None), (1, 3)):
        want = bdr.BurstDetector(kind, W, W, 0.5, 0.0, minlen).detect_block(x)[0]
        assert want.size == (5 if minlen == 1 else 4)
        q = ya.BurstDetector(kind, W, W, 0.5, 0.0, minlen)
        q.detect_block(np.ones(W + 40, bdr.acr.DTYPES[kind]) if cap is None else np.zeros(3, bdr.acr.DTYPES[kind]))
        r = bdr.BurstDetector(kind, W, W, 0.5, 0.0, minlen)       # a pending run in front (ones correlate), or none
        r.detect_block(np.ones(W + 40, bdr.acr.DTYPES[kind]) if cap is None else np.zeros(3, bdr.acr.DTYPES[kind]))
        assert (r.pending is not None) == (cap is None)
        want, _ = r.detect_block(x)
        got = q.detect_block(x) if cap is None else q.detect_block(x, cap=cap)
        assert got[0].tobytes() == want[:cap].tobytes() and not got[1]
        assert cap is None or got[2] == want.size
        assert q.pending is None and q.position == r.position


def test_threshold_one_never_fires_on_the_energy_itself(ya):
    for kind in KINDS:
        x, *_ = bdr.case(kind, "W1")
        q = ya.BurstDetector(kind, 1, 0, 1.0)
        ev, over = q.detect_block(x)
        assert ev.size == 0 and not over and q.pending is None and q.position == x.size


def test_energy_floor(ya):
    x, *_ = bdr.case("cccf", "W64")
    for floor in (100.0, 1e9):
        want = bdr.run_calls(bdr.BurstDetector("cccf", 64, 5, 0.7, floor), x, (T + 1, T))
        assert bdr.same(bdr.run_calls(ya.BurstDetector("cccf", 64, 5, 0.7, floor), x, (T + 1, T)), want)
    assert sum(w[0].size for w in want) == 0


def test_bad_arguments_are_config_errors(ya):
    for kind in KINDS:
        for args in [(0, 1, 0.5), (ya.AUTOCORR_WMAX + 1, 1, 0.5), (8, ya.AUTOCORR_DMAX + 1, 0.5), (8, 8, 0.0),
                     (8, 8, -1.0), (8, 8, float("nan")), (8, 8, float("inf")), (8, 8, 0.5, -1.0),
                     (8, 8, 0.5, float("inf")), (8, 8, 0.5, 0.0, 0)]:
            with pytest.raises(ya.ConfigError):
                ya.BurstDetector(kind, *args)
        ya.BurstDetector(kind, ya.AUTOCORR_WMAX, ya.AUTOCORR_DMAX, 0.5, 0.0, 2 ** 40)
    with pytest.raises(ya.ConfigError):
        ya.BurstDetector("crcf", 8, 8, 0.5)
    q = ya.BurstDetector("cccf", 8, 8, 0.5)
    ev, over = q.detect_block(np.zeros(0, np.complex64))            # an empty call is a no-op
    assert ev.size == 0 and not over and q.position == 0
