"""OrdFilt on the device (ordfilt_kernels.hip) against tests/ordfilt_ref.py.  Every output is a copy of one input
sample, so every comparison is equality of the bytes: no tolerance anywhere in this file."""
import numpy as np
import pytest

import ordfilt_ref as ofr

pytestmark = pytest.mark.gpu
T, NMAX, REG_NMAX = ofr.TILE, ofr.NMAX, ofr.REG_NMAX
AUTO, LDS, REG = 0, 1, 2                                          # OrdFilt.set_kernel


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert (yagi_amd.ORDFILT_TILE, yagi_amd.ORDFILT_NMAX, yagi_amd.ORDFILT_REG_NMAX) == (T, NMAX, REG_NMAX)
    return yagi_amd


def same(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def first_diff(got, want):
    d = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    return (int(d[0]), d.size) if d.size else None


def dev_block(ya, q, x):
    x = np.ascontiguousarray(x, np.float32)
    n = x.size
    xd = ya.DeviceArray.from_numpy(x) if n else ya.DeviceArray(1, np.float32)
    yd = ya.DeviceArray(max(n, 1), np.float32)
    q.execute_block_devptr(xd, n, yd)
    ya.synchronize()
    return yd.to_numpy(n) if n else np.zeros(0, np.float32)


def inputs(seed, size):
    rng = np.random.default_rng(seed)
    return {"ties": ofr.tie_heavy(rng, size), "normal": rng.standard_normal(size).astype(np.float32)}


@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 64, 65, 255, NMAX])
def test_shapes_bitwise(ya, n):
    blocks = sorted({1, max(n - 1, 1), n, T - 1, T, T + 1, 2 * T + 5})
    for name, x in inputs(n, 2 * T + 5).items():
        S, _ = ofr.sorted_windows(np.zeros(n, np.float32), x)     # a fresh object on a prefix gives a prefix
        for k in sorted({0, n // 2, n - 1}):
            for nb in blocks:
                q = ya.OrdFilt(n, k)
                assert (q.n, q.k) == (n, k)
                got = dev_block(ya, q, x[:nb])
                assert same(got, S[:nb, k]), (name, n, k, nb, first_diff(got, S[:nb, k]))


@pytest.mark.parametrize("n", [17, 255])
def test_chunked_stream_equals_one_call(ya, n):
    chunks = [1, 2, n - 2, n - 1, n, T + 3, 0, 5]
    x = inputs(n + 1, sum(chunks))["ties"]
    k = n // 3
    want = ofr.OrdFilt(n, k).execute_block(x)
    assert same(dev_block(ya, ya.OrdFilt(n, k), x), want)
    q, at = ya.OrdFilt(n, k), 0
    for c in chunks:
        got = dev_block(ya, q, x[at:at + c])
        assert same(got, want[at:at + c]), (n, at, c, first_diff(got, want[at:at + c]))
        at += c
    # the host-pointer form on the same cuts
    q, at = ya.OrdFilt(n, k), 0
    for c in chunks:
        assert same(q.execute_block(x[at:at + c]), want[at:at + c]), (n, at, c)
        at += c


@pytest.mark.parametrize("n,k", [(17, 5), (255, 127), (1, 0), (2, 1)])
def test_per_sample_calls_interleaved_with_blocks(ya, n, k):
    """the mirror in both directions: host calls after a device block see its window, and a device block after host calls
    sees theirs; every output equals the all-block run's at the same place in the stream"""
    x = inputs(n + 2, 3 * n + T + 64)["ties"]
    y_all = dev_block(ya, ya.OrdFilt(n, k), x)
    assert same(y_all, ofr.OrdFilt(n, k).execute_block(x))
    q, r, at = ya.OrdFilt(n, k), ofr.OrdFilt(n, k), 0
    out = {}

    def block(c):
        nonlocal at
        got = dev_block(ya, q, x[at:at + c])
        assert same(got, r.execute_block(x[at:at + c]))
        out.update({at + i: got[i] for i in range(c)})
        at += c

    def one():
        nonlocal at
        out[at] = q.execute_one(x[at])
        assert same(out[at], r.execute_one(x[at]))
        at += 1

    def push(execute):
        nonlocal at
        q.push(x[at])
        r.push(x[at])
        at += 1
        if execute:
            out[at - 1] = q.execute()
            assert same(out[at - 1], r.execute())

    block(5)
    assert same(q.execute(), r.execute())                        # straight after a block: the whole window of n
    for _ in range(3):
        one()
    push(False)
    push(True)
    block(n + 3)
    q.write(x[at:at + 4])
    r.write(x[at:at + 4])
    at += 4
    out[at - 1] = q.execute()
    assert same(out[at - 1], r.execute())
    block(max(n - 2, 1))
    one()
    block(T + 1)
    push(True)
    block(2)
    for pos, v in out.items():
        assert same(v, y_all[pos]), (n, k, pos)


def test_reset_returns_to_the_zero_window(ya):
    x = inputs(9, 300)["normal"] + np.float32(5.0)               # all positive: the zero window shows in the first outputs
    q = ya.OrdFilt(33, 4)
    first = dev_block(ya, q, x)
    assert np.all(first[:28] == 0)
    again = dev_block(ya, q, x)
    assert not same(first, again)
    q.reset()
    assert same(dev_block(ya, q, x), first)
    q.write(x[:40])
    q.reset()
    assert same(q.execute(), np.float32(0))
    assert same(dev_block(ya, q, x), first)


def test_clone_continues_identically(ya):                        # test_ordfilt_copy, ordfilt.rs:74-99
    rng = np.random.default_rng(77)
    q0, r = ya.OrdFilt(17, 5), ofr.OrdFilt(17, 5)
    for v in rng.standard_normal(20).astype(np.float32):
        assert same(q0.execute_one(v), r.execute_one(v))
    q1 = q0.clone()
    assert (q1.n, q1.k) == (17, 5)
    for v in rng.standard_normal(60).astype(np.float32):
        y0, y1 = q0.execute_one(v), q1.execute_one(v)
        assert same(y0, y1) and same(y0, r.execute_one(v))
    x = rng.standard_normal(T + 40).astype(np.float32)
    want = r.execute_block(x)
    assert same(dev_block(ya, q0, x), want)
    q2 = q0.clone()                                              # after a device block: the window comes from the device
    assert same(dev_block(ya, q1, x), want)
    x2 = rng.standard_normal(50).astype(np.float32)
    want2 = r.execute_block(x2)
    for q in (q0, q1, q2):
        assert same(dev_block(ya, q, x2), want2)


def test_medfilt(ya):
    q = ya.OrdFilt.medfilt(4)
    assert (q.n, q.k) == (9, 4)
    x = inputs(4, 500)["normal"]
    assert same(q.execute_block(x), ofr.OrdFilt.medfilt(4).execute_block(x))
    big = ya.OrdFilt.medfilt((NMAX - 1) // 2)
    assert (big.n, big.k) == (NMAX, (NMAX - 1) // 2)


def test_many_workgroups(ya):
    x = inputs(20, 1 << 20)["normal"]
    x[::1000] = np.float32(50.0)                                 # spikes the median removes
    got = dev_block(ya, ya.OrdFilt(9, 4), x)
    want = ofr.OrdFilt(9, 4).execute_block(x)
    assert same(got, want), first_diff(got, want)
    assert got.max() < 10


@pytest.mark.parametrize("n", [5, 64])
def test_nan_and_inf_at_tile_seams(ya, n):
    x = inputs(30 + n, 2 * T + 50)["normal"]
    u = x.view(np.uint32)
    specials = [0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x7FC00123, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF]
    at = [0, 1, n - 1, T - n, T - 2, T - 1, T, T + 1, T + n - 1, 2 * T - 1, 2 * T, 2 * T + 3, 2 * T + 49]
    for j, p in enumerate(at):
        u[p] = specials[j % len(specials)]
    u[T - 1], u[T] = 0x7FC00000, 0x7FC00000                       # equal NaN keys on both sides of a seam
    S, _ = ofr.sorted_windows(np.zeros(n, np.float32), x)
    for k in (0, n // 2, n - 1):
        got = dev_block(ya, ya.OrdFilt(n, k), x)
        assert same(got, S[:, k]), (n, k, first_diff(got, S[:, k]))
    assert np.isnan(S[:, n - 1]).any() and np.isnan(S[:, 0]).any()


@pytest.mark.parametrize("n", list(range(2, REG_NMAX + 1)))
def test_each_kernel_form_forced(ya, n):
    """the LDS form and the register-resident form on the same stream: the issue's block lengths, then a stream cut into
    chunks, with ties, signed zeros, NaN and inf around the tile seams; both equal the restatement, so each other"""
    blocks = sorted({1, n - 1, n, T - 1, T, T + 1, 2 * T + 5})
    x = inputs(50 + n, 2 * T + 5)["ties"]
    x[7::13] = inputs(60 + n, x[7::13].size)["normal"]
    u = x.view(np.uint32)
    for j, p in enumerate([3, T - 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 4]):
        u[p] = [0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000][j % 4]
    S, _ = ofr.sorted_windows(np.zeros(n, np.float32), x)
    chunks = [1, 2, n - 1, n, T + 3, 0, 5, T - 200]
    assert sum(chunks) + 100 <= x.size
    for form in (LDS, REG):
        for k in sorted({0, n // 2, n - 1}):
            for nb in blocks:
                q = ya.OrdFilt(n, k)
                q.set_kernel(form)
                got = dev_block(ya, q, x[:nb])
                assert same(got, S[:nb, k]), (form, n, k, nb, first_diff(got, S[:nb, k]))
            q, at = ya.OrdFilt(n, k), 0
            q.set_kernel(form)
            for c in chunks:
                got = dev_block(ya, q, x[at:at + c])
                assert same(got, S[at:at + c, k]), (form, n, k, at, c, first_diff(got, S[at:at + c, k]))
                at += c
            clone = q.clone()                                     # the forced form travels with the clone
            assert same(dev_block(ya, clone, x[at:at + 100]), S[at:at + 100, k])


def test_set_kernel_errors(ya):
    q = ya.OrdFilt(REG_NMAX + 1, 0)
    with pytest.raises(ya.ConfigError, match=str(REG_NMAX)):
        q.set_kernel(REG)
    with pytest.raises(ya.ConfigError):
        ya.OrdFilt(1, 0).set_kernel(REG)
    with pytest.raises(ya.ConfigError):
        q.set_kernel(3)
    q.set_kernel(LDS)
    x = inputs(2, 100)["ties"]
    assert same(dev_block(ya, q, x), ofr.OrdFilt(REG_NMAX + 1, 0).execute_block(x))


def test_many_workgroups_lds_form(ya):
    x = inputs(21, 1 << 20)["normal"]
    q = ya.OrdFilt(9, 4)
    q.set_kernel(LDS)
    got = dev_block(ya, q, x)
    want = ofr.OrdFilt(9, 4).execute_block(x)
    assert same(got, want), first_diff(got, want)


@pytest.mark.parametrize("n,nb", [(5, 1), (5, 3), (64, T + 1), (255, 2 * T + 5), (NMAX, T)])
def test_host_pointer_form_equals_device_pointer_form(ya, n, nb):
    x = inputs(n + nb, 2 * nb)["ties"]
    qh, qd = ya.OrdFilt(n, n // 2), ya.OrdFilt(n, n // 2)
    for part in (x[:nb], x[nb:]):
        yh = qh.execute_block(part)
        assert same(yh, dev_block(ya, qd, part))
    y = np.empty(nb, np.float32)
    assert qh.execute_block(x[:nb], y) is y
    with pytest.raises(ya.ConfigError):
        qh.execute_block(x[:nb], np.empty(nb + 1, np.float32))


def test_errors_leave_the_object_usable(ya):
    with pytest.raises(ya.ConfigError, match="filter length must be greater than zero"):
        ya.OrdFilt(0, 0)
    with pytest.raises(ya.ConfigError, match=r"filter index must be in \[0,n-1\]"):
        ya.OrdFilt(7, 7)
    with pytest.raises(ya.ConfigError, match=str(NMAX)):
        ya.OrdFilt(NMAX + 1, 0)
    with pytest.raises(ya.ConfigError, match=str(NMAX)):
        ya.OrdFilt.medfilt(NMAX // 2 + 1)
    x = inputs(1, 200)["ties"]
    q, r = ya.OrdFilt(17, 8), ofr.OrdFilt(17, 8)
    assert same(dev_block(ya, q, x[:50]), r.execute_block(x[:50]))
    buf = ya.DeviceArray(4096, np.float32)
    buf.zero()
    for xo, yo in ((0, 0), (0, 63), (63, 0), (10, 20)):
        with pytest.raises(ya.ConfigError, match="overlap"):
            q.execute_block_devptr(buf.ptr + 4 * xo, 64, buf.ptr + 4 * yo)
    q.execute_block_devptr(buf.ptr, 0, buf.ptr)                   # nothing to do: no error, no state change
    assert same(dev_block(ya, q, x[50:]), r.execute_block(x[50:]))
