"""Autocorr on the GPU against tests/autocorr_ref.py, bit for bit (rxx and energy), at the smallest shapes that reach
each path of autocorr_kernels.hip (T = the tile): a one-sample window and call, calls shorter than the carried history,
coinciding / overlapping / adjacent spans, the largest LDS stage, a delayed span one tile back, and at the longest delay a
delayed span wholly in the history, then across the history seam, then in the caller's buffer.  Then the stream semantics
(per-sample calls after a block, clone, reset), the argument checks and the exact non-finite footprint."""
import numpy as np
import pytest

import autocorr_ref as acr
import nonfinite_util as nfu

pytestmark = pytest.mark.gpu
T, WMAX, DMAX = acr.TILE, acr.WMAX, acr.DMAX

#        W     d      call lengths
ROWS = [(1,    0,     (1, T + 1)),
        (4,    3,     (2, 3, T - 1)),
        (33,   0,     (T + 1,)),
        (64,   64,    (3 * T + 17,)),
        (64,   5,     (T, T + 1)),
        (WMAX, 1,     (T - 1, 2 * T + 1)),
        (7,    T + 9, (3 * T,)),
        (16,   DMAX,  (100, DMAX + 2 * T))]
CASES = [("cccf",) + r for r in ROWS] + [("rrrf",) + r for r in ROWS if r[0] in (4, WMAX) or r[:2] == (64, 5)]
IDS = [f"{k}-W{W}-d{d}" for k, W, d, _ in CASES]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


_REF = {}


def reference(kind, W, d, lens):
    """(x, [(rxx, energy) per call]) of the stream cut into calls of `lens`; computed once and handed out read-only"""
    key = (kind, W, d, tuple(lens))
    if key not in _REF:
        x = acr.stream(np.random.default_rng(W * 131 + d * 7 + len(kind) + sum(lens)), kind, sum(lens))
        r = acr.Autocorr(kind, W, d)
        outs, at = [], 0
        for n in lens:
            outs.append(r.execute_block(x[at:at + n], energy=True))
            at += n
        for a in [x] + [v for pair in outs for v in pair]:
            a.setflags(write=False)
        _REF[key] = (x, outs)
    return _REF[key]


def parts(x, lens):
    at = 0
    for n in lens:
        yield x[at:at + n]
        at += n


@pytest.mark.parametrize("kind,W,d,lens", CASES, ids=IDS)
def test_block_calls_equal_the_reference_with_and_without_energy(ya, kind, W, d, lens):
    x, want = reference(kind, W, d, lens)
    q, p = ya.Autocorr(kind, W, d), ya.Autocorr(kind, W, d)
    assert (q.window_size, q.delay) == (W, d)
    for i, part in enumerate(parts(x, lens)):
        rxx, en = q.execute_block(part, energy=True)
        only = p.execute_block(part)
        assert rxx.dtype == x.dtype and en.dtype == np.float32
        assert rxx.tobytes() == want[i][0].tobytes(), (i, "rxx")
        assert en.tobytes() == want[i][1].tobytes(), (i, "energy")
        assert only.tobytes() == want[i][0].tobytes(), (i, "rxx without energy")


def test_zero_delay_identity_on_the_gpu(ya):
    x, _ = reference("cccf", 33, 0, (T + 1,))
    rxx, en = ya.Autocorr("cccf", 33, 0).execute_block(x, energy=True)
    assert np.ascontiguousarray(rxx.real).tobytes() == en.tobytes()
    assert np.ascontiguousarray(rxx.imag).tobytes() == np.zeros(x.size, np.float32).tobytes()


@pytest.mark.parametrize("kind,W,d", [("cccf", 4, 3), ("cccf", 64, 5), ("rrrf", 64, 5), ("cccf", 7, T + 9)])
def test_per_sample_calls_clone_and_reset_continue_the_stream(ya, kind, W, d):
    lens = (T + 3, 5, 40, T + 1)
    x = acr.stream(np.random.default_rng(W + d), kind, sum(lens))
    a, b, c, e = parts(x, lens)
    q, r = ya.Autocorr(kind, W, d), acr.Autocorr(kind, W, d)
    assert q.execute_block(a).tobytes() == r.execute_block(a).tobytes()
    for v in b:                                                       # per-sample calls after a block
        q.push(v)
        r.push(v)
        assert np.array([q.execute()]).tobytes() == np.array([r.execute()]).tobytes()
        assert np.array([q.get_energy()]).tobytes() == np.array([r.get_energy()]).tobytes()
    q.write(c)                                                        # then a block after host-side pushes
    r.write(c)
    q2, r2 = q.clone(), r.clone()
    assert (q2.window_size, q2.delay) == (W, d)
    for o in (q, q2):
        rxx, en = o.execute_block(e, energy=True)
        want = r2.clone().execute_block(e, energy=True)
        assert rxx.tobytes() == want[0].tobytes() and en.tobytes() == want[1].tobytes()
    q3 = q.clone()                                                    # clone right after a block (state on the device)
    assert q3.execute_block(a).tobytes() == q.execute_block(a).tobytes()
    q.reset()
    fresh = acr.Autocorr(kind, W, d).execute_block(a)
    assert q.execute_block(a).tobytes() == fresh.tobytes()


def test_bad_arguments_are_config_errors(ya):
    for kind in ("cccf", "rrrf"):
        for W, d in [(0, 1), (WMAX + 1, 1), (8, DMAX + 1)]:
            with pytest.raises(ya.ConfigError):
                ya.Autocorr(kind, W, d)
        ya.Autocorr(kind, WMAX, DMAX)
    with pytest.raises(ya.ConfigError):
        ya.Autocorr("crcf", 8, 8)


# one non-finite sample at stream index s; the calls are cut so that both footprints cross a tile seam and a call seam
#            W   d      call lengths          s
NONFINITE = [(64, 5,     (T + 20, T),         T - 30),      # [s, s+68] holds the tile seam T and the call seam T + 20
             (7,  T + 9, (T + 12, T + 100),   T - 3)]       # [s, s+6] holds the tile seam T; [s+d, s+d+6] ends on the
                                                            # second call's tile seam 2T + 12, its delayed samples are
                                                            # the first call's (the carried history)


@pytest.mark.parametrize("part", ["re", "im"])
@pytest.mark.parametrize("value", ["nan", "+inf", "-inf"])
@pytest.mark.parametrize("W,d,lens,s", NONFINITE, ids=["W64-d5", "W7-dT+9"])
def test_non_finite_footprint_is_exact(ya, W, d, lens, s, value, part):
    x, want = reference("cccf", W, d, lens)
    n = x.size
    idx = np.arange(n)
    m_en = (idx >= s) & (idx < s + W)
    m_rxx = m_en | ((idx >= s + d) & (idx < s + d + W))
    assert m_rxx.sum() == min(2 * W, W + d) and m_rxx[-1] == 0
    xp = nfu.poison(x, s, value, part)
    q = ya.Autocorr("cccf", W, d)
    got = [q.execute_block(p, energy=True) for p in parts(xp, lens)]
    rxx, en = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
    clean_rxx, clean_en = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    nfu.check_footprint(rxx, clean_rxx, m_rxx, f"rxx W={W} d={d} {value} in {part}")
    nfu.check_footprint(en, clean_en, m_en, f"energy W={W} d={d} {value} in {part}")
    q.reset()
    again = [q.execute_block(p, energy=True) for p in parts(x, lens)]
    assert np.concatenate([g[0] for g in again]).tobytes() == clean_rxx.tobytes()
    assert np.concatenate([g[1] for g in again]).tobytes() == clean_en.tobytes()
