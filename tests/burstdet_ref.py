"""BurstDetector (include/yagi_hip.h) restated twice in numpy f32 on top of autocorr_ref.Autocorr (a
helper, not a test module).

With rxx[n], energy[n] Autocorr(W, d)'s outputs, thr2 = fl(threshold^2), all in f32 and every operation rounded on its own:

    m = fl(fl(re^2) + fl(im^2)) of rxx (rrrf: fl(rxx^2)),  q = fl(energy^2)
    hit = energy > energy_floor and m > fl(thr2 q),         r = m / q where hit

A run is a maximal set of consecutive hits, its peak the index of its largest r (the earliest on ties); the first non-hit
after it closes it; a run that reaches the last sample seen is pending.  An event is a closed run of min_length or more.
Capacity: a call's hits, cut at every TILE samples counted from the call's first, fall into segments; a call with more
than tiles + SEGMAX of them reports overflow, returns no events and drops the pending run.

BurstDetector is the fast form: hits, run boundaries and the segment count vectorised, one argmax per run.
SlowBurstDetector is a per-sample state machine in numpy f32 scalars that knows nothing of tiles but for the capacity
rule.  tests/test_burstdet_ref_cpu.py pins one against the other; the GPU tests compare with the fast form.  Either takes
any object with Autocorr's execute_block / reset / clone as its correlator, so that the detection can be applied to the
GPU Autocorr's own output."""
import numpy as np

import autocorr_ref as acr

TILE = acr.TILE
SEGMAX = 8192        # YAGI_BURSTDET_SEGMAX
EVENT = np.dtype([("start", np.uint64), ("length", np.uint64), ("peak", np.uint64), ("ratio", np.float32),
                  ("energy", np.float32), ("rxx_re", np.float32), ("rxx_im", np.float32)])
f32 = np.float32


def _check(threshold, energy_floor, min_length):
    if not (np.isfinite(threshold) and threshold > 0 and np.isfinite(energy_floor) and energy_floor >= 0
            and min_length >= 1):
        raise ValueError("threshold, energy floor or minimum length out of range")


def _events(runs, min_length):
    out = np.zeros(len(runs), EVENT)
    for i, r in enumerate(runs):
        out[i] = tuple(r)
    return out[out["length"] >= min_length]


class _Base:
    def __init__(self, kind, window_size, delay, threshold, energy_floor=0.0, min_length=1, autocorr=None):
        _check(threshold, energy_floor, min_length)
        self.kind = kind
        self.ac = autocorr if autocorr is not None else acr.Autocorr(kind, window_size, delay)
        self.thr2 = f32(threshold) * f32(threshold)
        self.floor, self.min_length = f32(energy_floor), int(min_length)
        self.position, self.run = 0, None                          # run: the pending run as a list in EVENT's order

    def reset(self):
        self.ac.reset()
        self.position, self.run = 0, None

    def clone(self):
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new.ac = self.ac.clone()
        new.run = None if self.run is None else list(self.run)
        return new

    @property
    def pending(self):
        return None if self.run is None else _events([self.run], 1)[0]

    def flush(self):
        runs, self.run = ([] if self.run is None else [self.run]), None
        return _events(runs, self.min_length)

    def _sums(self, x):
        rxx, en = self.ac.execute_block(x, energy=True)
        if rxx.dtype.kind == "c":
            return np.ascontiguousarray(rxx.real), np.ascontiguousarray(rxx.imag), en
        return rxx, np.zeros(rxx.size, f32), en


class BurstDetector(_Base):
    def detect_block(self, x):
        """(events, overflow)"""
        re, im, en = self._sums(x)
        n, pos0 = en.size, self.position
        self.position += n
        with np.errstate(all="ignore"):
            m = re * re + im * im if self.kind == "cccf" else re * re
            q = en * en
            hit = (en > self.floor) & (m > self.thr2 * q)
        assert m.dtype == q.dtype == f32
        first = hit.copy()                                         # a hit that starts a segment
        first[1:] &= ~hit[:-1]
        first[::TILE] = hit[::TILE]
        if int(first.sum()) > (n + TILE - 1) // TILE + SEGMAX:
            self.run = None
            return np.zeros(0, EVENT), True
        edge = np.diff(np.concatenate([[0], hit.astype(np.int8), [0]]))
        closed, cur = [], self.run
        for s, e in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)):
            with np.errstate(all="ignore"):
                r = m[s:e] / q[s:e]
            k = s + int(np.argmax(r))                              # the first of the largest
            piece = [pos0 + s, e - s, pos0 + k, r[k - s], en[k], re[k], im[k]]
            if cur is not None and cur[0] + cur[1] == piece[0]:
                cur[1] += piece[1]
                if piece[3] > cur[3]:
                    cur[2:] = piece[2:]
            else:
                if cur is not None:
                    closed.append(cur)
                cur = piece
        if cur is not None and cur[0] + cur[1] != pos0 + n:
            closed.append(cur)
            cur = None
        self.run = cur
        return _events(closed, self.min_length), False


class SlowBurstDetector(_Base):
    def detect_block(self, x):
        re, im, en = self._sums(x)
        n, closed, segments, before = en.size, [], 0, False
        cplx = self.kind == "cccf"
        with np.errstate(all="ignore"):
            for i in range(n):
                a, b, e = re[i], im[i], en[i]
                m = f32(f32(a * a) + f32(b * b)) if cplx else f32(a * a)
                q = f32(e * e)
                hit = bool(e > self.floor) and bool(m > f32(self.thr2 * q))
                if hit:
                    if i % TILE == 0 or not before:
                        segments += 1
                    r, at = f32(m / q), self.position + i
                    if self.run is None:
                        self.run = [at, 1, at, r, e, a, b]
                    else:
                        self.run[1] += 1
                        if r > self.run[3]:
                            self.run[2:] = [at, r, e, a, b]
                elif self.run is not None:
                    closed.append(self.run)
                    self.run = None
                before = hit
        self.position += n
        if segments > (n + TILE - 1) // TILE + SEGMAX:
            self.run = None
            return np.zeros(0, EVENT), True
        return _events(closed, self.min_length), False


def cut(x, lens):
    at = 0
    for n in lens:
        yield x[at:at + n]
        at += n
    assert at == x.size


def run_calls(det, x, lens):
    """[(events, overflow, pending, position)] per call"""
    out = []
    for part in cut(x, lens):
        ev, over = det.detect_block(part)
        out.append((ev, over, det.pending, det.position))
    return out


def bursts(kind, W, d, n, spans, seed):
    """autocorr_ref.stream noise plus, over each (offset, length) of spans, a period-d sequence of modulus 4"""
    rng = np.random.default_rng(seed)
    x = acr.stream(rng, kind, n).copy()
    for at, length in spans:
        k = np.arange(length) % max(d, 1)
        if kind == "cccf":
            ph = rng.uniform(0, 2 * np.pi, max(d, 1))
            x[at:at + length] += (4 * np.exp(1j * ph[k])).astype(np.complex64)
        else:
            x[at:at + length] += (4 * rng.choice([-1.0, 1.0], max(d, 1))[k]).astype(np.float32)
    return x


T = TILE
#         name     W     d     n          threshold  min_length  (offset, length) of the bursts
SHAPES = [("W16",   16,   16,   3 * T + 5, 0.5,       8,          [(300, 400), (T - 200, 500), (2 * T + 100, 600)]),
          ("W64",   64,   5,    2 * T + 1, 0.7,       1,          [(500, 300), (T - 100, 400)]),
          ("W1024", 1024, 1024, 6 * T,     0.5,       1,          [(T // 2, 1024 + 3 * T + T // 2)]),
          ("W1",    1,    0,    T + 1,     0.5,       1,          [])]
SMALL = {"W16": 7, "W64": 13, "W1024": 1000, "W1": 1}              # a call shorter than W + d (W1: as short as calls get)
_CASE = {}


def case(kind, name):
    """(x, make, runs, cuts) of a stream of SHAPES, computed once: make(autocorr=None) builds the fast form, runs are
    the events of the whole stream in one call plus flush(), and cuts maps a label to call lengths:
        one                the whole stream
        1, T-1, T, T+1     a first call of that length
        small              calls of SMALL[name] samples (W1: fifty of them, then the rest)
        start              the longest run's first sample is a call's (and so a tile's) first
        end                the longest run's last sample is the last of a tile of the second call
        pending            the first call ends on the longest run's last sample: the next call's first sample closes it"""
    if (kind, name) not in _CASE:
        _, W, d, n, thr, minlen, spans = next(s for s in SHAPES if s[0] == name)
        x = bursts(kind, W, d, n, spans, seed=W * 7 + d + len(kind))
        x.setflags(write=False)

        def make(autocorr=None, cls=BurstDetector, min_length=minlen):
            return cls(kind, W, d, thr, 0.0, min_length, autocorr=autocorr)

        det = make()
        runs = np.concatenate([det.detect_block(x)[0], det.flush()])
        ends = [(int(r["start"]), int(r["start"] + r["length"])) for r in runs]
        # the longest run that ends behind the first tile; W1 has none (n = T + 1), there the longest: its "end" cut
        # puts no run's end on a tile's, which the other shapes do
        s, e = max([se for se in ends if T < se[1] < n] or [se for se in ends if 0 < se[0] and se[1] < n],
                   key=lambda se: se[1] - se[0])
        assert 0 < s < e < n
        small = SMALL[name]
        cuts = {"one": (n,), "1": (1, n - 1), "T-1": (T - 1, n - T + 1), "T": (T, n - T), "T+1": (T + 1, n - T - 1),
                "small": (small,) * 50 + (n - 50 * small,) if name == "W1" else
                         (small,) * (n // small) + ((n % small,) if n % small else ()),
                "start": (s, n - s), "end": (e % T, n - e % T), "pending": (e, n - e)}
        _CASE[kind, name] = (x, make, runs, cuts)
    return _CASE[kind, name]


_WANT = {}


def want(kind, name, label):
    """run_calls of the fast form on case(kind, name) cut at `label`, computed once and shared"""
    if (kind, name, label) not in _WANT:
        x, make, _, cuts = case(kind, name)
        _WANT[kind, name, label] = run_calls(make(), x, cuts[label])
    return _WANT[kind, name, label]


def same(a, b):
    """two run_calls results are equal byte for byte"""
    if len(a) != len(b):
        return False
    for (ev, over, pend, pos), (ev2, over2, pend2, pos2) in zip(a, b):
        if ev.tobytes() != ev2.tobytes() or over != over2 or pos != pos2 or (pend is None) != (pend2 is None):
            return False
        if pend is not None and pend.tobytes() != pend2.tobytes():
            return False
    return True


def alternating(kind, n):
    """1, 0, 1, 0, ...: at W = 1, d = 0 every other sample is a run of one, TILE / 2 segments a tile"""
    x = np.zeros(n, acr.DTYPES[kind])
    x[::2] = 1
    return x
