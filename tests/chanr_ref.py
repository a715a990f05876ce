"""Vectorised complex128 restatement of the firpfbchr analyzer and synthesizer (M channels, P inputs per step), in the
style of tests/chan_ref.py: torch, so that the same code runs on CPU tensors (tests/test_chanr_ref_cpu.py pins it to
three independent evaluations and to FirPfbChRef / FirPfbCh2Ref) and on device tensors (the GPU tests check every step
against it).  It calls neither the oracle nor yagi_amd.  Only h[0 : 2 M m] is used.  State -- analyzer history,
synthesizer transforms, both step counters -- is carried across calls and starts at zero, like the library's.

With L = 2 M m, stream index t from 0, s the step index counted from the start of the stream:
  analyzer     u_s[i] = sum_{n < 2m} h[i + n M] x[(s+1) P - 1 - i - n M]
               Z_s[(i - s P) mod M] = u_s[i];   y_s = IDFT_M(Z_s) / M          (torch.fft.ifft)
               = (1/M) sum_{l < L} h[l] x[(s+1) P - 1 - l] exp(+j 2 pi k (l - s P) / M)
  synthesizer  V_s = IDFT_M(X_s) M
               y[t] = (P/M) sum_{r >= 0, j + r P < L} h[j + r P] V_{floor(t/P) - r}[t mod M],   j = t mod P
"""
import math

import torch

from chan_ref import _c128

CHUNK_VALUES = 1 << 22           # complex128 values of the largest temporary of a chunk (64 MiB)
# per-step bound of the GPU tests: 3 x the worst ||e_s|| / (||r_s|| + rho) measured on the MI355X over every case of
# tests/test_gpu_chanr.py (the rule GPU_FRAME_TAU follows).  Measured worst: 2.17e-7, the synthesizer at M 512, P 1, m 1
# (step 1286), where a step is ONE output sample, a 1024-term sum; next 1.05e-7 (synthesizer M 6, P 1, m 2), and
# 5e-8 ... 9.7e-8 for every analyzer case, general and column kernel alike.
CHANR_FRAME_TAU = 6.5e-7


class FirPfbChrRef:
    """firpfbchr: M channels, P inputs per analyzer step (1 <= P <= M), branch length 2m"""

    def __init__(self, M, P, m, h, device=None):
        assert M >= 2 and 1 <= P <= M and m >= 1
        self.M, self.P, self.m, self.device = M, P, m, device
        self.L = 2 * M * m
        h = torch.as_tensor(h).to(dtype=torch.float64).flatten()
        assert h.numel() >= self.L, (h.numel(), self.L)
        self._h = h[: self.L]
        self.rows = -(-self.L // P) - 1              # synthesizer history: ceil(L/P) - 1 steps
        self._ana = None                             # last L - P input samples
        self._ana_steps = 0
        self._syn = None                             # last `rows` inverse transforms
        self._syn_steps = 0

    def analyzer_chunks(self, x, chunk=None):
        """x: flat complex block of whole steps -> yields (first step, complex128 [steps, M])"""
        M, P, L = self.M, self.P, self.L
        x = torch.as_tensor(x).reshape(-1)
        assert x.numel() % P == 0
        nsteps = x.numel() // P
        dev = self.device if self.device is not None else x.device
        hr = self._h.to(dev).flip(0)                 # hr[L-1-l] = h[l]: pairs with a window stored oldest first
        if self._ana is None:
            self._ana = torch.zeros(L - P, dtype=torch.complex128, device=dev)
        step = max(1, (chunk or CHUNK_VALUES) // L)
        cols = torch.arange(M, device=dev)
        for s0 in range(0, nsteps, step):
            N = min(step, nsteps - s0)
            xe = torch.cat([self._ana, _c128(x[s0 * P: (s0 + N) * P], dev)])
            win = xe.unfold(0, L, P)                 # win[s][a] = x[(s0+s) P + P - L + a]: the L samples ending at (s+1) P - 1
            assert win.shape[0] == N
            # u_s[i] = sum_n h[i + n M] x[top - i - n M]: fold the products, newest first, by l mod M
            u = (win * hr).flip(1).reshape(N, 2 * self.m, M).sum(dim=1)
            sg = torch.arange(N, device=dev) + (self._ana_steps % M)
            src = (cols[None, :] + (sg * P)[:, None]) % M            # Z_s[b] = u_s[(b + s P) mod M]
            Z = torch.gather(u, 1, src)
            self._ana = xe[N * P:].clone()
            self._ana_steps += N
            yield s0, torch.fft.ifft(Z, dim=1)

    def synthesizer_chunks(self, X, chunk=None):
        """X: steps of M channel samples -> yields (first step, complex128 [steps, P] time samples)"""
        M, P, L, B = self.M, self.P, self.L, self.rows
        X = torch.as_tensor(X).reshape(-1, M)
        dev = self.device if self.device is not None else X.device
        h = torch.cat([self._h.to(dev), torch.zeros((B + 1) * P - L, dtype=torch.float64, device=dev)]).reshape(B + 1, P)
        if self._syn is None:
            self._syn = torch.zeros(B, M, dtype=torch.complex128, device=dev)
        step = max(1, (chunk or CHUNK_VALUES) // M)
        j = torch.arange(P, device=dev)
        for s0 in range(0, X.shape[0], step):
            v = torch.fft.ifft(_c128(X[s0: s0 + step], dev), dim=1) * M
            N = v.shape[0]
            ve = torch.cat([self._syn, v])
            sg = torch.arange(N, device=dev) + (self._syn_steps % M)
            col = ((sg * P)[:, None] + j[None, :]) % M               # t mod M of output (s, j)
            y = torch.zeros(N, P, dtype=torch.complex128, device=dev)
            for r in range(B + 1):
                y += h[r] * torch.gather(ve[B - r: B - r + N], 1, col)
            self._syn = ve[N:].clone()
            self._syn_steps += N
            yield s0, y * (P / M)

    def analyzer_execute(self, x, chunk=None):
        return torch.cat([y for _, y in self.analyzer_chunks(x, chunk)])

    def synthesizer_execute(self, X, chunk=None):
        return torch.cat([y for _, y in self.synthesizer_chunks(X, chunk)])


def auto_takes_column(M, P, m, nsteps):
    """kernel choice auto of the analyzer, restated: the column kernel only where profiles/r13_kbench_chanr.txt has it
    ahead of the general kernel at both measured block lengths (tests/test_chanr_table_cpu.py checks this rule against
    the committed table, tests/test_gpu_chanr.py checks the library against this rule)"""
    if not (M in (64, 128, 256) and (8 * P) % M == 0 and 2 * m <= 16):
        return False
    if (nsteps + 1) * P <= (1 << 20):              # nothing shorter than floor(2^20 / P) steps was measured
        return False
    D, p = P // math.gcd(M, P), 2 * m
    if D == 1:
        return p >= 4                              # zero-padded lengths too: ahead even of the general kernel at half the taps
    if p == 16:
        return D in (3, 5) or (D == 7 and M == 64)
    if p == 8:
        return D == 3 and M <= 128
    return False
