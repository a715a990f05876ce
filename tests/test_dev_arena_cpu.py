"""The arena checker of tests/dev_arena.py catches what it is for, shown on the CPU with a numpy-backed stand-in for
the device array; and every `_dev` method of yagi_amd has a row in tests/test_gpu_dev_buffers.py or a stated reason."""
import ctypes as C
import inspect

import numpy as np
import pytest

from dev_arena import GUARD_MIN, SENTINEL, Arena, ArenaError


class FakeArray:
    """DeviceArray's surface (ptr, to_numpy, free) over host memory"""

    def __init__(self, n, dtype):
        self.dtype, self.n = np.dtype(dtype), int(n)
        self.mem = np.zeros(self.n, self.dtype)
        self.ptr = self.mem.ctypes.data

    def to_numpy(self, n=None, offset=0):
        n = self.n - offset if n is None else n
        return self.mem[offset:offset + n].copy()

    def free(self):
        self.mem = None


class FakeLib:
    @staticmethod
    def yagi_hip_memset_dev(ptr, value, nbytes):
        C.memset(ptr, value, nbytes)
        return 0

    @staticmethod
    def yagi_hip_memcpy_h2d(dst, src, nbytes):
        C.memmove(dst, src, nbytes)
        return 0


class FakeYa:
    DeviceArray = FakeArray
    lib = FakeLib

    @staticmethod
    def synchronize():
        pass


DTYPES = [np.float32, np.complex64, np.uint32]


def values(dtype, n):
    v = np.arange(1, n + 1)
    return (v + 1j * (v + 0.5)).astype(dtype) if np.dtype(dtype).kind == "c" else v.astype(dtype)


def kernel_writes(arena, host, at=0):
    """what a correct kernel does: host.size elements stored from element `at` of the operand on"""
    arena.dev.mem[arena.first + at:arena.first + at + host.size] = host


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_clean_case_passes(dtype, off):
    n = 37
    x = values(dtype, n)
    a = Arena(FakeYa, dtype, n, off, GUARD_MIN).load(x)
    assert a.ptr == a.dev.ptr + (GUARD_MIN + off) * np.dtype(dtype).itemsize
    assert a.dev.n == GUARD_MIN + off + n + GUARD_MIN
    a.assert_input_intact(x)
    y = Arena(FakeYa, dtype, n, off, GUARD_MIN)
    assert np.all(y.dev.mem.view(np.uint32) == SENTINEL)
    kernel_writes(y, x)
    assert np.array_equal(y.fetch_output(), x)
    # a call that reports a count below its capacity: exactly that many written
    z = Arena(FakeYa, dtype, n + 7, off, GUARD_MIN)
    kernel_writes(z, x)
    assert np.array_equal(z.fetch_output(n), x)
    with pytest.raises(ArenaError, match="sentinel survived"):
        z.fetch_output(n + 1)
    with pytest.raises(ArenaError, match="behind"):
        z.fetch_output(n - 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_word_in_front_is_reported(dtype):
    n, off = 16, 1
    x = values(dtype, n)
    y = Arena(FakeYa, dtype, n, off, GUARD_MIN)
    kernel_writes(y, x)
    y.dev.mem.view(np.uint32)[y.first * (y.dtype.itemsize // 4) - 1] = 0          # the last word in front
    with pytest.raises(ArenaError, match="in front"):
        y.fetch_output()
    # also inside the `off` elements, and at the allocation's first word
    for word in (0, GUARD_MIN * (y.dtype.itemsize // 4)):
        y = Arena(FakeYa, dtype, n, off, GUARD_MIN)
        kernel_writes(y, x)
        y.dev.mem.view(np.uint32)[word] = 7
        with pytest.raises(ArenaError, match="in front"):
            y.fetch_output()
    a = Arena(FakeYa, dtype, n, off, GUARD_MIN).load(x)
    a.dev.mem.view(np.uint32)[5] = 0
    with pytest.raises(ArenaError, match="in front"):
        a.assert_input_intact(x)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_word_behind_is_reported(dtype):
    n, off = 16, 1
    x = values(dtype, n)
    for back in (0, 1, GUARD_MIN - 1):                       # first word behind, the next, the allocation's last element
        y = Arena(FakeYa, dtype, n, off, GUARD_MIN)
        kernel_writes(y, x)
        y.dev.mem[y.first + n + back] = x[0]
        with pytest.raises(ArenaError, match="behind"):
            y.fetch_output()
    a = Arena(FakeYa, dtype, n, off, GUARD_MIN).load(x)
    a.dev.mem[a.first + n] = x[0]
    with pytest.raises(ArenaError, match="behind"):
        a.assert_input_intact(x)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_sentinel_left_inside_is_reported(dtype):
    n = 16
    x = values(dtype, n)
    for hole in (0, 7, n - 1):
        y = Arena(FakeYa, dtype, n, 0, GUARD_MIN)
        kernel_writes(y, x[:hole])
        kernel_writes(y, x[hole + 1:], hole + 1)
        with pytest.raises(ArenaError, match="sentinel survived"):
            y.fetch_output()
    if np.dtype(dtype).kind == "c":                          # half an element: the imaginary word alone
        y = Arena(FakeYa, dtype, n, 0, GUARD_MIN)
        kernel_writes(y, x)
        y.dev.mem.view(np.uint32)[2 * (y.first + 3) + 1] = SENTINEL
        with pytest.raises(ArenaError, match="sentinel survived"):
            y.fetch_output()


@pytest.mark.parametrize("dtype", [np.float32, np.complex64])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_nan_left_inside_is_reported(dtype, bad):
    n = 16
    x = values(dtype, n)
    x[9] = bad                                               # the canonical quiet NaN is not the sentinel pattern
    y = Arena(FakeYa, dtype, n, 3, GUARD_MIN)
    kernel_writes(y, x)
    with pytest.raises(ArenaError, match="non-finite"):
        y.fetch_output()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_changed_input_element_is_reported(dtype):
    n = 16
    x = values(dtype, n)
    a = Arena(FakeYa, dtype, n, 1, GUARD_MIN).load(x)
    a.dev.mem[a.first + 4] = x[5]
    with pytest.raises(ArenaError, match="input operand changed"):
        a.assert_input_intact(x)
    if np.dtype(dtype).kind == "f":                          # -0.0 for +0.0 is a change: the comparison is on bits
        z = np.zeros(n, dtype)
        a = Arena(FakeYa, dtype, n, 1, GUARD_MIN).load(z)
        a.dev.mem[a.first + 2] = -0.0
        with pytest.raises(ArenaError, match="input operand changed"):
            a.assert_input_intact(z)


def test_guard_has_a_floor():
    with pytest.raises(AssertionError):
        Arena(FakeYa, np.float32, 8, 0, GUARD_MIN - 1)


def dev_entry_points(ya):
    """'Class.method' for every method of the package's classes whose name ends in _dev, and the module's own functions"""
    names = set()
    for cname, cls in inspect.getmembers(ya, inspect.isclass):
        if cls.__module__ != ya.__name__ or cname.startswith("_"):      # private bases: seen through their subclasses
            continue
        for mname, _ in inspect.getmembers(cls, lambda m: inspect.isfunction(m) or inspect.ismethod(m)):
            if mname.endswith("_dev") and not mname.startswith("_"):
                names.add(f"{cname}.{mname}")
    for fname, fn in inspect.getmembers(ya, inspect.isfunction):
        if fn.__module__ == ya.__name__ and fname.endswith("_dev"):
            names.add(fname)
    return names


def test_every_dev_entry_point_has_a_row_or_a_reason():
    import yagi_amd as ya
    import test_gpu_dev_buffers as t
    have = dev_entry_points(ya)
    assert len(have) >= 30                                   # the introspection itself works (39 as of this writing)
    rows = {r.entry for r in t.ROWS}
    excluded = set(t.EXCLUDED)
    assert all(isinstance(v, str) and v for v in t.EXCLUDED.values())
    assert not rows & excluded, rows & excluded
    assert rows | excluded == have, {"no row and no reason": sorted(have - rows - excluded),
                                     "not an entry point": sorted((rows | excluded) - have)}
    assert len({r.id for r in t.ROWS}) == len(t.ROWS)
