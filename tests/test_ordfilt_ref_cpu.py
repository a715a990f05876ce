"""tests/ordfilt_ref.py against Python's own stable sort, the counting scheme of ordfilt_kernels.hip against the
restatement, and the reference's copy test (ordfilt.rs:74-99).  No GPU."""
import re
import struct

import numpy as np
import pytest

import ordfilt_ref as ofr
from conftest import ROOT

CASES = [(1, 0), (2, 1), (5, 2), (17, 5), (64, 0), (33, 32)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def by_list_sort(n, k, x):
    """the reference's loop with list.sort(), which is stable and compares floats with `<` (so -0.0 == +0.0)"""
    win = [0.0] * n
    out = []
    for v in x:
        win = win[1:] + [float(v)]
        s = list(win)
        s.sort()
        out.append(s[k])
    return np.array(out, np.float32)


@pytest.mark.parametrize("n,k", CASES)
def test_restatement_equals_list_sort_on_ties_and_signed_zeros(n, k):
    rng = np.random.default_rng(n * 100 + k)
    x = ofr.tie_heavy(rng, 300)
    assert np.any(bits(x) == 0x80000000) and np.any(bits(x) == 0)
    got = ofr.OrdFilt(n, k).execute_block(x)
    assert bits(got).tobytes() == bits(by_list_sort(n, k, x)).tobytes()
    x = rng.standard_normal(200).astype(np.float32)
    x[::7] = np.inf
    x[3::11] = -np.inf
    got = ofr.OrdFilt(n, k).execute_block(x)
    assert bits(got).tobytes() == bits(by_list_sort(n, k, x)).tobytes()


def test_signed_zero_out_depends_on_window_position():
    q = ofr.OrdFilt(2, 0)
    y = q.execute_block(np.array([-0.0, 0.0, -0.0], np.float32))
    # windows (oldest first): [+0, -0], [-0, +0], [+0, -0]: the older zero is element 0
    assert list(bits(y)) == [0, 0x80000000, 0]


def test_key_is_monotone_and_puts_nan_beyond_the_infinities():
    pnan, nnan = struct.unpack("<f", struct.pack("<I", 0x7FC00001))[0], struct.unpack("<f", struct.pack("<I", 0xFFC00001))[0]
    v = np.array([nnan, -np.inf, -3.0, -1e-40, -0.0, 0.0, 1e-40, 2.5, np.inf, pnan], np.float32)
    v.view(np.uint32)[0], v.view(np.uint32)[-1] = 0xFFC00001, 0x7FC00001
    kk = ofr.key(v).astype(np.int64)
    assert kk[4] == kk[5]
    assert np.all(np.diff(np.delete(kk, 4)) > 0)


@pytest.mark.parametrize("n,k", CASES)
@pytest.mark.parametrize("kind", ["ties", "nan"])
def test_counting_model_has_one_match_per_window(n, k, kind):
    rng = np.random.default_rng(n * 7 + k)
    x = ofr.tie_heavy(rng, 150)
    if kind == "nan":
        u = x.view(np.uint32)
        u[rng.integers(0, x.size, 12)] = 0x7FC00000
        u[rng.integers(0, x.size, 12)] = 0xFFC00000
        u[rng.integers(0, x.size, 6)] = 0x7F800000
        u[rng.integers(0, x.size, 6)] = 0xFF800000
    win = ofr.tie_heavy(rng, n)                                   # a history with its own ties, as a later call sees it
    want = ofr.sorted_windows(win, x)[0][:, k]
    for tile in (1, 7, 16, 64, 4096):                             # tiles shorter and longer than the window
        m = ofr.counting_model(n, k, win, x, tile)
        assert all(len(c) == 1 for c in m), [i for i, c in enumerate(m) if len(c) != 1][:5]
        assert np.array([c[0] for c in m], np.uint32).tobytes() == bits(want).tobytes()


def test_copy_continues_identically():                            # test_ordfilt_copy, ordfilt.rs:74-99
    rng = np.random.default_rng(5)
    q0 = ofr.OrdFilt(17, 5)
    for v in rng.standard_normal(20).astype(np.float32):
        q0.execute_one(v)
    q1 = q0.clone()
    for v in rng.standard_normal(60).astype(np.float32):
        assert bits(q0.execute_one(v)) == bits(q1.execute_one(v))


@pytest.mark.parametrize("n,k", [(17, 5), (5, 0), (64, 63)])
def test_chunked_equals_whole_and_per_sample(n, k):
    rng = np.random.default_rng(n)
    x = ofr.tie_heavy(rng, 400)
    whole = ofr.OrdFilt(n, k).execute_block(x)
    q, parts, at = ofr.OrdFilt(n, k), [], 0
    for c in [1, 2, n - 2, n - 1, n, 70, 0, 5]:
        parts.append(q.execute_block(x[at:at + c]))
        at += c
    parts.append(q.execute_block(x[at:]))
    assert np.concatenate(parts).view(np.uint32).tobytes() == bits(whole).tobytes()
    q = ofr.OrdFilt(n, k)
    one = np.array([q.execute_one(v) for v in x[:100]], np.float32)
    assert bits(one).tobytes() == bits(whole[:100]).tobytes()


def test_medfilt_is_2m_plus_1_at_m():
    x = np.random.default_rng(3).standard_normal(100).astype(np.float32)
    q = ofr.OrdFilt.medfilt(4)
    assert (q.n, q.k) == (9, 4)
    y = q.execute_block(x)
    assert bits(y).tobytes() == bits(ofr.OrdFilt(9, 4).execute_block(x)).tobytes()
    assert bits(y[8:]).tobytes() == bits(np.median(np.lib.stride_tricks.sliding_window_view(x, 9), axis=1)).tobytes()


def test_constructor_errors_are_the_references():
    with pytest.raises(ValueError, match="filter length must be greater than zero"):
        ofr.OrdFilt(0, 0)
    with pytest.raises(ValueError, match=r"filter index must be in \[0,n-1\]"):
        ofr.OrdFilt(4, 4)


def test_named_constants_agree_across_the_layers():
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    nmax = int(re.search(r"#define YAGI_ORDFILT_NMAX (\d+)", hdr).group(1))
    tile = int(re.search(r"#define YAGI_ORDFILT_TILE (\d+)", hdr).group(1))
    py = (ROOT / "yagi_amd" / "__init__.py").read_text()
    assert int(re.search(r"^ORDFILT_NMAX = (\d+)", py, re.M).group(1)) == nmax == ofr.NMAX
    assert int(re.search(r"^ORDFILT_TILE = (\d+)", py, re.M).group(1)) == tile == ofr.TILE
    assert nmax >= 1025
    reg = int(re.search(r"#define YAGI_ORDFILT_REG_NMAX (\d+)", hdr).group(1))
    assert int(re.search(r"^ORDFILT_REG_NMAX = (\d+)", py, re.M).group(1)) == reg == ofr.REG_NMAX
