"""tests/burstdet_ref.py against itself: the vectorised form and the per-sample state machine agree byte for byte on every
stream and cut the GPU tests use, the streams provably reach every path of the device form (asserted on the reference:
a run inside a tile, across a tile seam, ending on a tile's last sample, starting on a tile's first, pending at a call's
end and closed by the next call's first sample, across three tiles or more, a tile with more than 300 runs, runs shorter
than min_length beside longer ones, threshold 1 at W = 1, d = 0), the capacity rule has its boundary where the
definition puts it, and the library's own host form (burst_detect_host, no GPU needed) gives the same events."""
import numpy as np
import pytest

import burstdet_ref as bdr

T = bdr.TILE
KINDS = ("cccf", "rrrf")
NAMES = [s[0] for s in bdr.SHAPES]
LABELS = ("one", "1", "T-1", "T", "T+1", "small", "start", "end", "pending")


def events_of(results):
    return np.concatenate([r[0] for r in results])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_fast_and_slow_forms_agree_and_the_cut_does_not_matter(kind, name):
    x, make, runs, cuts = bdr.case(kind, name)
    whole = None
    for label in LABELS:
        if name == "W1024" and label == "small" and kind == "rrrf":
            continue                                               # the slow form's cost; cccf covers the cut
        fast = bdr.want(kind, name, label)
        slow_det = make(cls=bdr.SlowBurstDetector)
        slow = bdr.run_calls(slow_det, x, cuts[label])
        assert bdr.same(fast, slow), (kind, name, label)
        assert not any(r[1] for r in fast)
        det = make()
        got = np.concatenate([events_of(bdr.run_calls(det, x, cuts[label])), det.flush()])
        assert got.tobytes() == np.concatenate([events_of(slow), slow_det.flush()]).tobytes()
        whole = got if whole is None else whole
        assert got.tobytes() == whole.tobytes() == runs.tobytes(), (kind, name, label)
        assert det.position == x.size and det.pending is None


def _segments(kind, name, lens):
    """per call, the (start, end) of every segment relative to the call's first sample, from a min_length = 1 detector"""
    x, make, _, _ = bdr.case(kind, name)
    det, out = make(min_length=1), []
    for part in bdr.cut(x, lens):
        pos0 = det.position
        before = det.pending
        ev, _ = det.detect_block(part)
        spans = [(int(e["start"]) - pos0, int(e["start"] + e["length"]) - pos0) for e in ev]
        if det.pending is not None:
            spans.append((int(det.pending["start"]) - pos0, part.size))
        out.append((spans, before))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_the_streams_reach_every_path(kind):
    reached = set()
    for name in NAMES:
        x, make, runs, cuts = bdr.case(kind, name)
        for s, e in _segments(kind, name, cuts["one"])[0][0]:
            if s // T == (e - 1) // T and s % T and e % T:
                reached.add("inside a tile")
            if (e - 1) // T == s // T + 1:
                reached.add("across a seam")
            if (e - 1) // T >= s // T + 2:
                reached.add("three tiles or more")
        per_tile = np.bincount([s // T for s, _ in _segments(kind, name, cuts["one"])[0][0]])
        if per_tile.max() > (300 if kind == "cccf" else 290):      # rrrf's stream has a zero every 7th sample only
            reached.add("a crowded tile")
        second = _segments(kind, name, cuts["start"])[1]
        if second[1] is None and any(s == 0 for s, _ in second[0]):
            reached.add("starts on a tile's first sample")
        second = _segments(kind, name, cuts["end"])[1]
        if any(e % T == 0 and e < sum(cuts["end"][1:]) for _, e in second[0]):
            reached.add("ends on a tile's last sample")
        pend = bdr.want(kind, name, "pending")
        first_pending = pend[0][2]
        if first_pending is not None and len(pend[1][0]):
            closed = pend[1][0][0]
            if closed["start"] == first_pending["start"] and closed["length"] == first_pending["length"] \
                    and closed["start"] + closed["length"] == pend[0][3]:
                reached.add("closed by the next call's first sample")
        all_runs = make(min_length=1)
        every = np.concatenate([all_runs.detect_block(x)[0], all_runs.flush()])
        if make().min_length > 1 and 0 < runs.size < every.size and (every["length"] < make().min_length).any():
            reached.add("short runs beside long ones")
    assert reached == {"inside a tile", "across a seam", "three tiles or more", "a crowded tile",
                       "starts on a tile's first sample", "ends on a tile's last sample",
                       "closed by the next call's first sample", "short runs beside long ones"}, reached


@pytest.mark.parametrize("kind", KINDS)
def test_threshold_one_never_fires_on_the_energy_itself(kind):
    x, _, runs, _ = bdr.case(kind, "W1")
    assert runs.size > 200
    det = bdr.BurstDetector(kind, 1, 0, 1.0)
    ev, over = det.detect_block(x)
    assert ev.size == 0 and not over and det.pending is None and det.flush().size == 0


# W = 1, d = 0 on 1, 0, 1, 0, ...: T / 2 segments a tile.  n samples hold ceil(n / 2) segments and ceil(n / T) tiles.
CAPACITY = [("below", 8 * T + 16, False), ("at", 8 * T + 18, False), ("above", 8 * T + 20, True)]


@pytest.mark.parametrize("label,n,over", CAPACITY)
def test_capacity_boundary(label, n, over):
    tiles, segments = (n + T - 1) // T, (n + 1) // 2
    assert (segments > tiles + bdr.SEGMAX) == over
    assert segments - (tiles + bdr.SEGMAX) == {"below": -1, "at": 0, "above": 1}[label]
    for kind in KINDS:
        x = bdr.alternating(kind, n + 4)
        res = []
        for cls in (bdr.BurstDetector, bdr.SlowBurstDetector):
            det = cls(kind, 1, 0, 0.5)
            res.append(bdr.run_calls(det, x, (n, 4)))
        assert bdr.same(*res)
        (ev, o, pend, pos), (ev2, o2, _, _) = res[0]
        assert o == over and not o2 and pos == n and pend is None   # sample n - 1 is a 0
        assert ev.size == (0 if over else segments)
        assert ev2.size == 2 and ev2["start"][0] == n              # the stream goes on after an overflow
    det = bdr.BurstDetector("cccf", 1, 0, 0.5)
    ev, o = det.detect_block(bdr.alternating("cccf", 8 * T))
    assert ev.size == 8192 and not o


def test_overflow_drops_the_pending_run():
    n = 8 * T + 21                                                  # ends on a 1: a run is pending there
    for cls in (bdr.BurstDetector, bdr.SlowBurstDetector):
        det = cls("cccf", 1, 0, 0.5)
        det.detect_block(np.ones(3, np.complex64))
        assert det.pending is not None and det.pending["length"] == 3
        x = bdr.alternating("cccf", n)
        x[0] = 0
        ev, over = det.detect_block(np.concatenate([x, np.ones(2, np.complex64)]))
        assert over and ev.size == 0 and det.pending is None
        ev, over = det.detect_block(np.array([1, 0], np.complex64))
        assert not over and ev.size == 1 and (ev["start"][0], ev["length"][0]) == (n + 5, 1)


@pytest.mark.parametrize("name", ["W16", "W64", "W1"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_librarys_host_form_equals_the_reference(kind, name):
    import yagi_amd as ya
    x, make, runs, _ = bdr.case(kind, name)
    det = make()
    _, W, d, _, thr, minlen, _ = next(s for s in bdr.SHAPES if s[0] == name)
    n = x.size - 3                                                  # a run of W1 is then pending at the end
    want, over = det.detect_block(x[:n])
    ev, o, pend = ya.burst_detect_host(kind, x[:n], W, d, thr, 0.0, minlen)
    assert ev.dtype == bdr.EVENT and ev.tobytes() == want.tobytes() and o == over
    assert (pend is None) == (det.pending is None)
    if pend is not None:
        assert pend.tobytes() == det.pending.tobytes()


def test_the_librarys_host_form_applies_the_capacity_rule():
    import yagi_amd as ya
    for _, n, over in CAPACITY:
        ev, o, _ = ya.burst_detect_host("rrrf", bdr.alternating("rrrf", n), 1, 0, 0.5)
        assert o == over and ev.size == (0 if over else (n + 1) // 2)
    with pytest.raises(ya.ConfigError):
        ya.burst_detect_host("cccf", np.zeros(4, np.complex64), 1, 0, float("nan"))
