"""Helpers of the non-finite footprint tests (test_nonfinite_util_cpu.py, test_gpu_nonfinite.py).

A NaN / Inf sample is the one input that tells a kernel that reads a sample outside its window and multiplies it by a
zero-padded tap or a masked lane (0 * NaN = NaN) from a kernel that never touches it.  The tests place one such sample
in a stream, run the object under test and its reference model over the same calls, and compare

  * the set of non-finite outputs with the model's set, exactly (no "at most"), and
  * every output outside that set with the run on the clean stream, bit for bit.
"""
import numpy as np

VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


def poison(x, idx, value, part="re"):
    """a copy of x with sample idx (an index or a list of them) made non-finite: value is NaN, +Inf or -Inf (or a key
    of VALUES); part = "re", "im" or "both" picks the component of a complex sample (a real one has only "re")"""
    v = VALUES[value] if isinstance(value, str) else float(value)
    assert not np.isfinite(v), "poison() writes non-finite values only"
    x = np.array(x, copy=True)
    assert x.dtype.kind in "fc"
    flat = x.reshape(-1)
    for i in np.atleast_1d(idx):
        i = int(i)
        assert 0 <= i < flat.size, (i, flat.size)
        if flat.dtype.kind == "c":
            assert part in ("re", "im", "both")
            re = v if part in ("re", "both") else flat[i].real
            im = v if part in ("im", "both") else flat[i].imag
            flat[i] = flat.dtype.type(complex(re, im))
        else:
            assert part == "re", "a real sample has no imaginary part"
            flat[i] = v
    return x


def mask(y):
    """per output element: any component non-finite"""
    y = np.asarray(y)
    if y.dtype.kind == "c":
        return ~(np.isfinite(y.real) & np.isfinite(y.imag))
    return ~np.isfinite(y)


def dilate(m, extra):
    """every run of True widened to the right by `extra` elements (clipped at the end of the array)"""
    m = np.asarray(m, bool)
    assert extra >= 0
    out = m.copy()
    if extra == 0 or not m.any():
        return out
    # out[i] = any(m[i - extra .. i]): a prefix-sum difference
    c = np.concatenate([[0], np.cumsum(m.reshape(-1))])
    i = np.arange(m.size)
    return (c[i + 1] - c[np.maximum(i - extra, 0)] > 0).reshape(m.shape)


def runs(m):
    """[(first, length)] of the runs of True in a flat mask"""
    m = np.asarray(m, bool).reshape(-1)
    d = np.diff(np.concatenate([[0], m.astype(np.int8), [0]]))
    first = np.flatnonzero(d == 1)
    return list(zip(first.tolist(), (np.flatnonzero(d == -1) - first).tolist()))


def _words(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.complex64), a.dtype
    return a.reshape(-1).view(np.uint32).reshape(a.size, -1)


def _describe(m):
    r = runs(m)
    return f"{int(np.sum(m))} elements in {len(r)} runs, (first, length) {r[:6]}{' ...' if len(r) > 6 else ''}"


def check_footprint(got_poisoned, got_clean, want_mask, what=""):
    """asserts that mask(got_poisoned) == want_mask exactly, and that wherever want_mask is False got_poisoned equals
    got_clean bit for bit (uint32 views); reports the first and last differing index and the run lengths"""
    got_poisoned, got_clean = np.asarray(got_poisoned).reshape(-1), np.asarray(got_clean).reshape(-1)
    want_mask = np.asarray(want_mask, bool).reshape(-1)
    assert got_poisoned.size == got_clean.size == want_mask.size, (got_poisoned.size, got_clean.size, want_mask.size)
    assert got_poisoned.dtype == got_clean.dtype
    got_mask = mask(got_poisoned)
    diff = got_mask != want_mask
    if diff.any():
        d = np.flatnonzero(diff)
        extra, missing = got_mask & ~want_mask, want_mask & ~got_mask
        raise AssertionError(
            f"{what}: non-finite footprint differs from the expected one at {d.size} outputs, first {d[0]}, last {d[-1]}"
            f"\n  expected: {_describe(want_mask)}\n  got:      {_describe(got_mask)}"
            f"\n  poisoned but not expected: {_describe(extra)}\n  expected but finite:       {_describe(missing)}")
    keep = ~want_mask
    wp, wc = _words(got_poisoned), _words(got_clean)
    bits = (wp != wc).any(axis=1) & keep
    if bits.any():
        d = np.flatnonzero(bits)
        raise AssertionError(
            f"{what}: {d.size} finite outputs outside the footprint differ from the clean run, first {d[0]} "
            f"({got_poisoned[d[0]]!r} vs {got_clean[d[0]]!r}), last {d[-1]}; runs {_describe(bits)}")
