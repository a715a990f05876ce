"""Guarded, offset, poisoned device buffers for the tests of the C ABI's `_dev` entry points (a helper, not a conftest).

An Arena is ONE allocation of guard + off + n + guard elements, every byte 0xFF (each f32 word a NaN, each u32 the
sentinel 0xFFFFFFFF, a bit pattern no kernel here produces from finite samples).  The operand handed to the kernel is
the n elements that start guard + off elements in: `off` moves it off the allocation's 256-byte boundary in steps of
the element size, and the guards are wide enough (>= GUARD_MIN elements, and at least the largest tile or halo of the
kernel under test) that no access a wrong kernel could plausibly make leaves the allocation.  Stray accesses are found
by reading the memory back, never by faulting:

  a write outside the operand        -> a guard word is no longer the sentinel          (fetch_output, assert_input_intact)
  an output element never written    -> a sentinel word survives inside the operand     (fetch_output)
  a read outside the input that is   -> the NaN reaches an output element               (fetch_output: finite)
  USED in a result

An over-read whose value is discarded leaves no trace in memory and is NOT caught.

`ya` is the yagi_amd module or anything with its DeviceArray / synchronize / lib.yagi_hip_memset_dev /
lib.yagi_hip_memcpy_h2d surface (tests/test_dev_arena_cpu.py drives the checker with a numpy-backed fake)."""
import ctypes as C

import numpy as np

SENTINEL = 0xFFFFFFFF
GUARD_MIN = 4096


class ArenaError(AssertionError):
    pass


class Arena:
    def __init__(self, ya, dtype, n, off=0, guard=GUARD_MIN):
        self.ya, self.dtype = ya, np.dtype(dtype)
        assert self.dtype.itemsize % 4 == 0, "the sentinel check works on 32-bit words"
        assert guard >= GUARD_MIN and off >= 0 and n >= 0
        self.n, self.off, self.guard = int(n), int(off), int(guard)
        self.first = self.guard + self.off                      # the operand's first element in the allocation
        self.size = self.first + self.n + self.guard
        self.dev = ya.DeviceArray(self.size, self.dtype)
        rc = ya.lib.yagi_hip_memset_dev(self.dev.ptr, 0xFF, self.size * self.dtype.itemsize)
        assert rc == 0

    @property
    def ptr(self):
        return self.dev.ptr + self.first * self.dtype.itemsize

    def load(self, host):
        host = np.ascontiguousarray(host, self.dtype)
        assert host.size == self.n, (host.size, self.n)
        if self.n:
            rc = self.ya.lib.yagi_hip_memcpy_h2d(self.ptr, host.ctypes.data_as(C.c_void_p), host.nbytes)
            assert rc == 0
        return self

    def _words(self):
        """the whole arena as (elements, u32 words, words per element) after a synchronize"""
        self.ya.synchronize()
        a = self.dev.to_numpy()
        return a, a.view(np.uint32), self.dtype.itemsize // 4

    def _check_guards(self, u, w, hi_elem=None):
        lo = self.first * w
        hi = (self.first + (self.n if hi_elem is None else hi_elem)) * w
        bad = np.flatnonzero(u[:lo] != SENTINEL)
        if bad.size:
            raise ArenaError(f"wrote in front of the operand: word {int(bad[-1]) - lo} (relative to its start), "
                             f"{bad.size} words in all")
        bad = np.flatnonzero(u[hi:] != SENTINEL)
        if bad.size:
            raise ArenaError(f"wrote behind the operand: word {int(bad[0])} past its end, {bad.size} words in all")

    def fetch_output(self, count=None):
        """the operand after a kernel wrote it.  Every word in front of and behind it is still the sentinel, no sentinel
        word survives inside it and every value in it is finite.  count < n (a call that reports how many of its n
        elements of capacity it wrote): exactly the first count elements are written, the rest count as guard."""
        count = self.n if count is None else int(count)
        assert 0 <= count <= self.n
        a, u, w = self._words()
        self._check_guards(u, w, count)
        lo, hi = self.first * w, (self.first + count) * w
        left = np.flatnonzero(u[lo:hi] == SENTINEL)
        if left.size:
            raise ArenaError(f"a sentinel survived inside the operand: word {int(left[0])} of {hi - lo}, "
                             f"{left.size} words in all")
        y = a[self.first:self.first + count].copy()
        f = y.view(np.float32) if self.dtype.kind in "fc" else None
        if f is not None and not np.all(np.isfinite(f)):
            raise ArenaError(f"a non-finite value inside the operand: f32 word {int(np.flatnonzero(~np.isfinite(f))[0])}")
        return y

    def assert_input_intact(self, host):
        """the operand still holds exactly what load() wrote and both guards are still sentinel"""
        host = np.ascontiguousarray(host, self.dtype)
        assert host.size == self.n
        a, u, w = self._words()
        self._check_guards(u, w)
        got = u[self.first * w:(self.first + self.n) * w]
        diff = np.flatnonzero(got != host.view(np.uint32))
        if diff.size:
            raise ArenaError(f"the input operand changed: word {int(diff[0])}, {diff.size} words in all")

    def free(self):
        self.dev.free()
