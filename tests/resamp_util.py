"""Restatement of Resamp::execute (src/filter/resampler/resamp.rs:95-165) for the -m gpu tests: the reference's
per-sample loop with its u32 phase over the golden-pinned oracle.FirPfbFilter, plus closed forms of the same schedule
(output j of a call: A_j = p0 + j step, after input A_j >> 24, branch (A_j & 0xFFFFFF) >> (24 - bits)).
Test infrastructure only."""
import numpy as np

U24 = 1 << 24


def rust_step(rate):
    """((1 << 24) as f32 / rate).round() as u32: f32 division, rounding half away from zero"""
    v = np.float32(16777216.0) / np.float32(rate)
    return int(np.floor(np.float64(v) + 0.5))


def designed_taps(oracle, m, fc, as_, npfb):
    """resamp.rs:47-56: Kaiser taps normalised to DC gain npfb with a sequential f32 sum (iter().sum())"""
    n = 2 * m * npfb + 1
    hf = oracle.fir_design_kaiser(n, float(np.float32(fc) / np.float32(npfb)), as_, 0.0).astype(np.float32)
    gain = np.add.accumulate(hf, dtype=np.float32)[-1]
    gain = np.float32(npfb) / gain
    return (hf * gain).astype(np.float32)


class RefResamp:
    """the reference loop over oracle.FirPfbFilter(kind, npfb, h, 2 m npfb)"""

    def __init__(self, oracle, kind, rate, m, npfb, h):
        self.pfb = oracle.FirPfbFilter(kind, npfb, h, 2 * m * npfb)
        self.tdt = self.pfb.tdt
        self.bits = int(npfb).bit_length() - 1
        self.m = m
        self.set_rate(rate)
        self.phase = 0

    def set_rate(self, rate):
        self.r = np.float32(rate)
        self.step = rust_step(self.r)

    def adjust_rate(self, gamma):
        self.set_rate(np.float32(self.r * np.float32(gamma)))

    def get_num_output(self, n):
        return num_output(self.phase, self.step, n)[0]

    def execute(self, x):
        self.pfb.push(x)
        y = []
        while self.phase <= 0xFFFFFF:
            y.append(self.pfb.execute(self.phase >> (24 - self.bits)))
            self.phase = (self.phase + self.step) & 0xFFFFFFFF
        self.phase -= U24
        return y

    def execute_block(self, xs):
        y = []
        for v in xs:
            y += self.execute(v)
        return np.array(y, dtype=self.tdt)


def loop_count(phase, step, n):
    """get_num_output (:128-139) as the reference writes it; returns (count, phase after the call)"""
    cnt = 0
    for _ in range(n):
        while phase <= 0xFFFFFF:
            cnt += 1
            phase += step
        phase -= U24
    return cnt, phase


def num_output(phase, step, n):
    """closed form: N = max(0, ceil((2^24 n - p0) / step)), p' = p0 + N step - 2^24 n"""
    end = n * U24
    cnt = max(0, -((phase - end) // step))
    return cnt, phase + cnt * step - end


def closed_form(hb, win, x, step, p0, bits, chunk=1 << 22):
    """y[j] = sum_k hb[b_j][k] X[i_j - k] for integer-valued data (every partial sum exact in f32); hb [npfb][Ls] in
    natural order, win = the Ls samples before x[0].  Returns (y, phase after the call)."""
    Ls = hb.shape[1]
    X = np.concatenate([win, x])
    ny, p1 = num_output(p0, step, len(x))
    y = np.empty(ny, x.dtype)
    for j0 in range(0, ny, chunk):
        j = np.arange(j0, min(ny, j0 + chunk), dtype=np.uint64)
        a = np.uint64(p0) + j * np.uint64(step)
        i = (a >> np.uint64(24)).astype(np.int64) + Ls
        b = ((a & np.uint64(0xFFFFFF)) >> np.uint64(24 - bits)).astype(np.int64)
        acc = np.zeros(len(j), x.dtype)
        for k in range(Ls):
            acc += hb[b, k] * X[i - k]
        y[j0:j0 + len(j)] = acc
    return y, p1


def bank(h, m, npfb):
    """FirPfbFilter::new(npfb, h, 2 m npfb) in natural order: hb[i][k] = h[i + k npfb]"""
    Ls = 2 * m
    return np.ascontiguousarray(np.asarray(h)[: Ls * npfb].reshape(Ls, npfb).T)
