"""OrdFilt (src/filter/ordfilt.rs) restated in numpy, and a plain-Python model of the counting scheme of
yagi_amd/csrc/ordfilt_kernels.hip (a helper, not a test module).

The restatement: the window is the last n samples, oldest first, zeros after new / reset.  Every sample is pushed, the
window is sorted with a STABLE sort and element k (0-based, ascending) is the output.  The sort compares key(), a u32
that is monotone in the f32 value with -0.0 folded onto +0.0: for windows without NaN that is the reference's
partial_cmp exactly (equal keys are bit-identical samples, or zeros of either sign, which the stable sort leaves in
age order).  NaN, which the reference leaves unspecified, sorts above +inf with the sign bit clear and below -inf with
it set -- the rule include/yagi_hip.h documents."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

NMAX = 1025          # YAGI_ORDFILT_NMAX
TILE = 4096          # YAGI_ORDFILT_TILE
REG_NMAX = 9         # YAGI_ORDFILT_REG_NMAX


def key(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    u = np.where(u == 0x80000000, np.uint32(0), u)
    return np.where(u & 0x80000000 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def sorted_windows(win, x):
    """(S, window after): S[i] = the window after pushing x[i], stably sorted under key(); shared by every k"""
    win = np.ascontiguousarray(win, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    n = win.size
    stream = np.concatenate([win, x])
    if x.size == 0:
        return np.zeros((0, n), np.float32), win.copy()
    w = sliding_window_view(stream, n)[1:]                       # row i: stream[i + 1 .. i + n], oldest first
    order = np.argsort(sliding_window_view(key(stream), n)[1:], axis=1, kind="stable")
    return np.take_along_axis(w, order, axis=1), stream[-n:].copy()


class OrdFilt:
    def __init__(self, n, k):
        if n == 0:
            raise ValueError("filter length must be greater than zero")
        if k >= n:
            raise ValueError("filter index must be in [0,n-1]")
        self.n, self.k = n, k
        self.reset()

    @classmethod
    def medfilt(cls, m):
        return cls(2 * m + 1, m)

    def reset(self):
        self.win = np.zeros(self.n, np.float32)

    def clone(self):
        new = OrdFilt(self.n, self.k)
        new.win = self.win.copy()
        return new

    def push(self, x):
        self.win = np.concatenate([self.win[1:], np.array([x], np.float32)])

    def write(self, x):
        for v in np.asarray(x, np.float32):
            self.push(v)

    def execute(self):
        order = np.argsort(key(self.win), kind="stable")
        return self.win[order[self.k]]

    def execute_one(self, x):
        self.push(x)
        return self.execute()

    def execute_block(self, x):
        S, self.win = sorted_windows(self.win, x)
        return S[:, self.k].copy()


def counting_model(n, k, win, x, tile=TILE):
    """The kernel's scheme, one tile after another, in plain Python on integers.  Returns matches[i] = the list of u32
    bit patterns that candidates wrote into output slot i (the scheme is right when every list has one entry).
    tile = 4096 is a workgroup of the LDS form; tile = 16 is a lane of the register-resident form, which runs the same
    scheme over its own 16 outputs."""
    hist = [int(v) for v in np.ascontiguousarray(win, np.float32).view(np.uint32)]
    xs = [int(v) for v in np.ascontiguousarray(x, np.float32).view(np.uint32)]
    assert len(hist) == n
    halo = n - 1
    matches = [[] for _ in xs]
    for t0 in range(0, len(xs), tile):
        cnt = min(tile, len(xs) - t0)
        W = cnt + halo
        raw = [xs[t0 + p - halo] if t0 + p - halo >= 0 else hist[n + t0 + p - halo] for p in range(W)]
        ks = [int(v) for v in key(np.array(raw, np.uint32).view(np.float32))] if W else []
        for p in range(W):
            kp = ks[p]
            i0, i1 = max(p - halo, 0), min(p, cnt - 1)
            r = sum(ks[l] <= kp for l in range(i0, p)) + sum(ks[l] < kp for l in range(p + 1, i0 + halo + 1))
            if r == k:
                matches[t0 + i0].append(raw[p])
            for i in range(i0 + 1, i1 + 1):
                r -= ks[i - 1] <= kp
                r += ks[i + halo] < kp
                if r == k:
                    matches[t0 + i].append(raw[p])
    return matches


def tie_heavy(rng, size):
    """integer-valued samples in [-3, 3], zeros of either sign"""
    x = rng.integers(-3, 4, size).astype(np.float32)
    neg = rng.integers(0, 2, size).astype(bool)
    x[(x == 0) & neg] = np.float32(-0.0)
    return x
