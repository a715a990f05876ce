"""PreambleDetector (include/yagi_hip.h) restated twice (a helper, not a test module).

The definition: X = the stream since reset(), X[j] = 0 for j < 0.  With the K templates v_k (L taps each), ep the f32 sum
from +0.0 of fl(fl(p.re^2) + fl(p.im^2)) and thr2 = fl(threshold^2), after sample n, with w[i] = X[n-L+1+i]:

    rxy_k[n]  = dotprod(w, v_k)    the sequential sum from +0.0; every product and add rounded on its own; the complex
                                   product is num-complex's (a.re b.re - a.im b.im, a.re b.im + a.im b.re)
    energy[n] = sum_i fl(fl(w[i].re^2) + fl(w[i].im^2))      in the same order from +0.0
    m_k = fl(fl(re^2) + fl(im^2)) of rxy_k;  kb = 0, then for k = 1 .. K-1 kb = k where m_k > m_kb;  m = m_kb
    q = fl(energy ep);  hit = energy > energy_floor and m > fl(thr2 q);  r = m / q where hit

Runs, peaks, the pending run, events and the capacity rule are BurstDetector's (tests/burstdet_ref.py), with the best
hypothesis kb at the peak carried in the event.

The templates are an input: the tests hand over the library's own (preamble_templates / get_templates), so that a host
libm never decides a comparison; templates_f64 is the numpy-f64 evaluation they are held against to 1 ulp.

Correlator is the fast form of the bank: numpy float32, vectorised over n, Python loops over i and k, real and imaginary
parts as separate float32 arrays.  SlowCorrelator is made only of oracle.Window and oracle.dotprod.  PreambleDetector is
the fast detection (hits, run boundaries and the segment count vectorised, one argmax per run), SlowPreambleDetector a
per-sample state machine in numpy f32 scalars.  Either detector takes any object with correlate_block / reset / clone as
its correlator, so that the detection can be applied to the GPU object's own correlate_block."""
import numpy as np

LMAX = 1024          # YAGI_PDET_LMAX
KMAX = 32            # YAGI_PDET_KMAX
TILE = 2048          # YAGI_PDET_TILE
SEGMAX = 8192        # YAGI_PDET_SEGMAX
EVENT = np.dtype([("start", np.uint64), ("length", np.uint64), ("peak", np.uint64), ("ratio", np.float32),
                  ("energy", np.float32), ("rxy_re", np.float32), ("rxy_im", np.float32), ("hypothesis", np.uint32),
                  ("pad", np.uint32)])
f32 = np.float32


def templates_f64(p, dphi):
    """conj(p[i]) e^{-j dphi_k i} in numpy f64 from the f32 inputs, not rounded: [K, L] complex128"""
    p = np.asarray(p, np.complex64).astype(np.complex128)
    i = np.arange(p.size, dtype=np.float64)
    return np.array([np.conj(p) * np.exp(-1j * (np.float64(d) * i)) for d in np.asarray(dphi, np.float32)])


def preamble_energy(p):
    ep = f32(0.0)
    for z in np.asarray(p, np.complex64):
        ep = f32(ep + f32(f32(z.real * z.real) + f32(z.imag * z.imag)))
    return ep


class Correlator:
    def __init__(self, templates):
        self.V = np.ascontiguousarray(templates, np.complex64)
        assert self.V.ndim == 2 and 1 <= self.V.shape[0] <= KMAX and 1 <= self.V.shape[1] <= LMAX
        self.K, self.L = self.V.shape
        self.reset()

    def reset(self):
        self.hist = np.zeros(self.L - 1, np.complex64)            # the last L - 1 samples, oldest first

    def clone(self):
        new = Correlator(self.V)
        new.hist = self.hist.copy()
        return new

    def correlate_block(self, x):
        """(rxy[K, n], energy[n]) after each sample of x"""
        x = np.asarray(x, np.complex64)
        n, K, L = x.size, self.K, self.L
        s = np.concatenate([self.hist, x])
        sr, si = np.ascontiguousarray(s.real, f32), np.ascontiguousarray(s.imag, f32)
        vr, vi = np.ascontiguousarray(self.V.real, f32), np.ascontiguousarray(self.V.imag, f32)
        re, im, en = np.zeros((K, n), f32), np.zeros((K, n), f32), np.zeros(n, f32)
        with np.errstate(all="ignore"):
            for i in range(L):
                ar, ai = sr[i:i + n], si[i:i + n]
                en = en + (ar * ar + ai * ai)
                for k in range(K):
                    re[k] = re[k] + (ar * vr[k, i] - ai * vi[k, i])
                    im[k] = im[k] + (ar * vi[k, i] + ai * vr[k, i])
        assert re.dtype == im.dtype == en.dtype == f32
        self.hist = s[s.size - (L - 1):].copy()
        out = np.empty((K, n), np.complex64)
        out.real, out.imag = re, im
        return out, en


class SlowCorrelator:
    """the definition word for word: w = Window(L); rxy_k = dotprod(w, v_k); the energy is the real part of
    dotprod(w, conj(w)), whose terms are fl(re^2) - fl(im (-im)) = fl(fl(re^2) + fl(im^2)) summed in the same order"""

    def __init__(self, oracle, templates, _w=None):
        self.o, self.V = oracle, np.ascontiguousarray(templates, np.complex64)
        self.K, self.L = self.V.shape
        self.w = _w if _w is not None else oracle.Window(self.L, np.complex64)

    def reset(self):
        self.w.reset()

    def clone(self):
        return SlowCorrelator(self.o, self.V, _w=self.w.clone())

    def correlate_block(self, x):
        x = np.asarray(x, np.complex64)
        rxy, en = np.empty((self.K, x.size), np.complex64), np.empty(x.size, f32)
        for i, v in enumerate(x):
            self.w.push(v)
            w = self.w.read()
            for k in range(self.K):
                rxy[k, i] = self.o.dotprod("ccc", w, self.V[k])
            en[i] = f32(np.real(self.o.dotprod("ccc", w, np.conj(w))))
        return rxy, en


def _check(threshold, energy_floor, min_length, ep):
    if not (np.isfinite(threshold) and threshold > 0 and np.isfinite(energy_floor) and energy_floor >= 0
            and min_length >= 1 and np.isfinite(ep) and ep > 0):
        raise ValueError("threshold, energy floor, minimum length or preamble energy out of range")


def _events(runs, min_length):
    out = np.zeros(len(runs), EVENT)
    for i, r in enumerate(runs):
        out[i] = tuple(r)
    return out[out["length"] >= min_length]


class _Base:
    def __init__(self, p, templates, threshold, energy_floor=0.0, min_length=1, correlator=None):
        self.ep = preamble_energy(p)
        _check(threshold, energy_floor, min_length, self.ep)
        self.co = correlator if correlator is not None else Correlator(templates)
        self.thr2 = f32(threshold) * f32(threshold)
        self.floor, self.min_length = f32(energy_floor), int(min_length)
        self.position, self.run = 0, None                          # run: the pending run as a list in EVENT's order

    def reset(self):
        self.co.reset()
        self.position, self.run = 0, None

    def clone(self):
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new.co = self.co.clone()
        new.run = None if self.run is None else list(self.run)
        return new

    @property
    def pending(self):
        return None if self.run is None else _events([self.run], 1)[0]

    def flush(self):
        runs, self.run = ([] if self.run is None else [self.run]), None
        return _events(runs, self.min_length)

    def _sums(self, x):
        rxy, en = self.co.correlate_block(x)
        return np.ascontiguousarray(rxy.real), np.ascontiguousarray(rxy.imag), en


class PreambleDetector(_Base):
    def detect_block(self, x):
        """(events, overflow)"""
        re, im, en = self._sums(x)
        n, pos0 = en.size, self.position
        self.position += n
        with np.errstate(all="ignore"):
            m = re * re + im * im
            kb, mb = np.zeros(n, np.int64), m[0].copy()
            for k in range(1, m.shape[0]):
                take = m[k] > mb
                mb[take], kb[take] = m[k][take], k
            q = en * self.ep
            hit = (en > self.floor) & (mb > self.thr2 * q)
        assert m.dtype == q.dtype == mb.dtype == f32
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
                r = mb[s:e] / q[s:e]
            k = s + int(np.argmax(r))                              # the first of the largest
            piece = [pos0 + s, e - s, pos0 + k, r[k - s], en[k], re[kb[k], k], im[kb[k], k], kb[k], 0]
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


class SlowPreambleDetector(_Base):
    def detect_block(self, x):
        re, im, en = self._sums(x)
        n, closed, segments, before = en.size, [], 0, False
        with np.errstate(all="ignore"):
            for i in range(n):
                e = en[i]
                kb, m = 0, f32(f32(re[0, i] * re[0, i]) + f32(im[0, i] * im[0, i]))
                for k in range(1, re.shape[0]):
                    mk = f32(f32(re[k, i] * re[k, i]) + f32(im[k, i] * im[k, i]))
                    if mk > m:
                        kb, m = k, mk
                q = f32(e * self.ep)
                hit = bool(e > self.floor) and bool(m > f32(self.thr2 * q))
                if hit:
                    if i % TILE == 0 or not before:
                        segments += 1
                    r, at = f32(m / q), self.position + i
                    if self.run is None:
                        self.run = [at, 1, at, r, e, re[kb, i], im[kb, i], kb, 0]
                    else:
                        self.run[1] += 1
                        if r > self.run[3]:
                            self.run[2:] = [at, r, e, re[kb, i], im[kb, i], kb, 0]
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


def same_sums(a, b):
    """two correlate_block results are equal byte for byte"""
    return a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


T = TILE
N = 3 * T + 500
THRESHOLD = 0.6
#         name     L     K   the hypotheses span -+ this
SHAPES = [("L1",    1,    1,  0.0),
          ("L5",    5,    3,  0.2),
          ("L8",    8,    32, 0.3),
          ("L16",   16,   3,  0.2),
          ("L64",   64,   9,  0.1),
          ("L257",  257,  5,  0.02),
          ("L1024", 1024, 4,  0.004)]
NAMES = [s[0] for s in SHAPES]
FAMILIES = ("noise", "plateau")
SMALL = {"L1": 1, "L5": 3, "L8": 5, "L16": 11, "L64": 50, "L257": 200, "L1024": 1000}   # a call shorter than L - 1
LABELS = ("one", "1", "T-1", "T", "T+1", "small", "start", "end", "pending")


def hypotheses(name):
    _, L, K, span = next(s for s in SHAPES if s[0] == name)
    return np.linspace(-span, span, K).astype(f32) if K > 1 else np.zeros(1, f32)


def preamble_starts(L):
    """family "noise": the first copy lies inside a tile, the second and third each end across a tile seam, the fourth
    ends 7 samples before the stream's end"""
    return [300, T - L // 2 - 1, 2 * T - 1, N - L - 7]


def preamble_offsets(dphi):
    """the carrier offsets of the four copies: the first, the middle and the last hypothesis, and one 0.3 of a step off the
    second hypothesis"""
    K = dphi.size
    step = float(dphi[1] - dphi[0]) if K > 1 else 0.0
    return [float(dphi[0]), float(dphi[K // 2]), float(dphi[-1]), float(dphi[min(1, K - 1)]) + 0.3 * step]


def plateau_spans(L):
    """family "plateau": (offset, length, value) of the stretches.  The first spans three tiles, the second crosses the
    seam at 3 T; there are more than L zeros between them, so that the first one's run closes"""
    return [(300, 2 * T - 150, 2 + 1j), (3 * T - 450, 550, 0.5 - 1.5j)]


def stream(name, family):
    """(p, dphi, x) of a shape: x holds N samples"""
    _, L, K, _ = next(s for s in SHAPES if s[0] == name)
    rng = np.random.default_rng(1000 * L + K + 3)
    dphi = hypotheses(name)
    if family == "noise":
        # unit-modulus QPSK preamble in noise 10 dB below it
        p = np.exp(1j * np.pi / 2 * rng.integers(0, 4, L)).astype(np.complex64)
        x = (np.sqrt(0.05) * (rng.standard_normal(N) + 1j * rng.standard_normal(N))).astype(np.complex64)
        if L == 1:
            x[::7] = 0                                             # r = 1 wherever there is energy: runs of six
        for s, o in zip(preamble_starts(L), preamble_offsets(dphi)):
            x[s:s + L] += (p * np.exp(1j * (o * np.arange(L) + 0.7))).astype(np.complex64)
    else:
        p = np.ones(L, np.complex64)
        dphi = np.concatenate([np.zeros(1, f32), dphi[1:]])
        x = np.zeros(N, np.complex64)
        for at, length, c in plateau_spans(L):
            x[at:at + length] = c
    return p, dphi, x


_CASE = {}


def case(name, family, templates_of):
    """(p, dphi, x, make, runs, cuts) of a stream, computed once: templates_of(p, dphi) gives the K x L templates (the
    library's); make(correlator=None, cls=PreambleDetector, **kw) builds a detector at THRESHOLD; runs are the events of
    the whole stream in one call plus flush(), and cuts maps a label to call lengths:
        one                the whole stream
        1, T-1, T, T+1     a first call of that length
        small              up to sixty calls of SMALL[name] samples (shorter than L - 1; L1: single samples), then the rest
        start              the longest run's first sample is a call's (and so a tile's) first
        end                the longest run's last sample is the last of a tile of the second call
        pending            the first call ends on the longest run's last sample: the next call's first sample closes it"""
    if (name, family) not in _CASE:
        p, dphi, x = stream(name, family)
        for a in (p, dphi, x):
            a.setflags(write=False)
        V = np.array(templates_of(p, dphi), np.complex64)
        V.setflags(write=False)

        def make(correlator=None, cls=PreambleDetector, threshold=THRESHOLD, energy_floor=0.0, min_length=1):
            return cls(p, V, threshold, energy_floor, min_length, correlator=correlator)

        det = make()
        runs = np.concatenate([det.detect_block(x)[0], det.flush()])
        ends = [(int(r["start"]), int(r["start"] + r["length"])) for r in runs]
        # the longest run that ends behind the first tile and in front of the stream's end
        s, e = max([se for se in ends if T < se[1] < N], key=lambda se: se[1] - se[0])
        assert 0 < s < e < N
        small = SMALL[name]
        few = min(60, N // small)
        cuts = {"one": (N,), "1": (1, N - 1), "T-1": (T - 1, N - T + 1), "T": (T, N - T), "T+1": (T + 1, N - T - 1),
                "small": (small,) * few + ((N - few * small,) if N > few * small else ()),
                "start": (s, N - s), "end": (e % T, N - e % T), "pending": (e, N - e)}
        _CASE[name, family] = (p, dphi, x, make, runs, cuts)
    return _CASE[name, family]


_WANT = {}


def want(name, family, label, templates_of):
    """run_calls of the fast form on case(name, family) cut at `label`, computed once and shared"""
    if (name, family, label) not in _WANT:
        _, _, x, make, _, cuts = case(name, family, templates_of)
        _WANT[name, family, label] = run_calls(make(), x, cuts[label])
    return _WANT[name, family, label]


def alternating(n):
    """1, 0, 1, 0, ...: at L = 1, K = 1, p = [1] every other sample is a run of one, TILE / 2 segments a tile"""
    x = np.zeros(n, np.complex64)
    x[::2] = 1
    return x
