"""Vectorised complex128 restatement of the firpfbch / firpfbch2 analyzers and synthesizers.

Written in torch so that the same code runs on CPU tensors (the CPU tests pin it to the oracle) and on device tensors
(the GPU tests check every output frame of long blocks against it).  It restates the semantics of the oracle
(oracle/yagi_oracle.c yo_firpfbch*_analyzer_execute, oracle/oracle.py FirPfbCh*.synthesizer_execute) in closed form
and does not call either of them or yagi_amd.  Only h[0 : M p] is used (the Kaiser prototypes of the tests are
M p + 1 long).  State -- analyzer history, synthesizer windows, step parity -- is carried across calls and starts at
zero, like the library's.  Blocks are processed in chunks of frames, each with its p - 1 frame halo, so that peak
memory stays bounded whatever the block length.

With hs[n][i] = h[i + n M] and xf[f][j] = x[f M + j]:
  firpfbch analyzer     X[f][j] = sum_n hs[n][M-1-j] xf[f-n][j];  y[f] = DFT_M(X[f])                 (forward)
  firpfbch synthesizer  v[f] = IDFT_M(X[f]) M;  y[f][i] = sum_n hs[n][i] v[f-n][i]
  firpfbch2 analyzer    step s takes z[s] = x[s M/2 : (s+1) M/2]; zr[s][c] = z[s][M/2-1-c];
                        A[s] = sum_n hs[n][:M/2] zr[s-2n],  B[s] = sum_n hs[n][M/2:] zr[s-1-2n];
                        X[s] = [A, B] on even steps, [B, A] on odd ones;  y[s] = IDFT_M(X[s]) / M
  firpfbch2 synthesizer v[s] = IDFT_M(X[s]) M / 2;
                        F[s][b] = sum_n hs[n][b mod M/2] v[s-2n][b] + hs[n][M/2 + b mod M/2] v[s-1-2n][b];
                        y[s] = F[s][:M/2] on even steps, F[s][M/2:] on odd ones
(s counts steps from the start of the stream: the parity is carried across calls.)
"""
import torch

CHUNK_SAMPLES = 1 << 22          # input samples per chunk (complex128 temporaries of 64 MiB)
# per-frame bound of the GPU tests: the worst frame measured over every case of test_gpu_chan_shapes.py and the
# full-size C4 / C5 blocks was 1.35e-7 (firpfbch2 analyzer, M 8, m 4); 3x headroom
GPU_FRAME_TAU = 4e-7


def shard_columns(y, r, R):
    """the sub-band shard of rank r of R: channels k = r + R q"""
    return y[..., r::R]


def _c128(x, device):
    x = torch.as_tensor(x)
    return x.to(device=device if device is not None else x.device, dtype=torch.complex128)


def _taps(h, M, p, device):
    h = torch.as_tensor(h).to(dtype=torch.float64).flatten()
    assert h.numel() >= M * p, (h.numel(), M, p)
    return h[: M * p].reshape(p, M).to(device)                  # hs[n][i] = h[i + n M]


class FirPfbChRef:
    """firpfbch: M channels, p taps per branch"""

    def __init__(self, M, p, h, device=None):
        self.M, self.p, self.device = M, p, device
        self._h = torch.as_tensor(h)
        self._ana = None
        self._syn = None

    def _hs(self, device):
        return _taps(self._h, self.M, self.p, device)

    def analyzer_chunks(self, x, chunk=None):
        """x: flat complex block of whole frames -> yields (first frame, complex128 [frames, M]) chunk by chunk"""
        M, p = self.M, self.p
        x = torch.as_tensor(x).reshape(-1, M)
        dev = self.device if self.device is not None else x.device
        hr = self._hs(dev).flip(1)                               # hr[n][j] = h[n M + M-1-j]
        if self._ana is None:
            self._ana = torch.zeros(p - 1, M, dtype=torch.complex128, device=dev)
        step = max(1, (chunk or CHUNK_SAMPLES) // M)
        for f0 in range(0, x.shape[0], step):
            xe = torch.cat([self._ana, _c128(x[f0: f0 + step], dev)])
            N = xe.shape[0] - (p - 1)
            X = torch.zeros(N, M, dtype=torch.complex128, device=dev)
            for n in range(p):
                X += hr[n] * xe[p - 1 - n: p - 1 - n + N]
            self._ana = xe[N:].clone()
            yield f0, torch.fft.fft(X, dim=1)

    def synthesizer_chunks(self, X, chunk=None):
        """X: frames of M channel samples -> yields (first frame, complex128 [frames, M] time samples)"""
        M, p = self.M, self.p
        X = torch.as_tensor(X).reshape(-1, M)
        dev = self.device if self.device is not None else X.device
        hs = self._hs(dev)
        if self._syn is None:
            self._syn = torch.zeros(p - 1, M, dtype=torch.complex128, device=dev)
        step = max(1, (chunk or CHUNK_SAMPLES) // M)
        for f0 in range(0, X.shape[0], step):
            v = torch.fft.ifft(_c128(X[f0: f0 + step], dev), dim=1) * M
            ve = torch.cat([self._syn, v])
            N = v.shape[0]
            y = torch.zeros(N, M, dtype=torch.complex128, device=dev)
            for n in range(p):
                y += hs[n] * ve[p - 1 - n: p - 1 - n + N]
            self._syn = ve[N:].clone()
            yield f0, y

    def analyzer_execute(self, x, chunk=None):
        return torch.cat([y for _, y in self.analyzer_chunks(x, chunk)])

    def synthesizer_execute(self, X, chunk=None):
        return torch.cat([y for _, y in self.synthesizer_chunks(X, chunk)])


class FirPfbCh2Ref:
    """firpfbch2 (2x oversampled): M channels (even), branch length 2m, M/2 inputs per analyzer step"""

    def __init__(self, M, m, h, device=None):
        assert M % 2 == 0 and m >= 1
        self.M, self.m, self.device = M, m, device
        self._h = torch.as_tensor(h)
        self._ana = None                 # last 2p - 1 input steps, reversed within the step
        self._ana_steps = 0
        self._syn = None                 # last 2p - 1 inverse transforms
        self._syn_steps = 0

    def _hs(self, device):
        return _taps(self._h, self.M, 2 * self.m, device)

    def analyzer_chunks(self, x, chunk=None):
        """x: flat complex block of whole steps -> yields (first step, complex128 [steps, M])"""
        M, M2, p = self.M, self.M // 2, 2 * self.m
        H = 2 * p - 1
        x = torch.as_tensor(x).reshape(-1, M2)
        dev = self.device if self.device is not None else x.device
        hs = self._hs(dev)
        if self._ana is None:
            self._ana = torch.zeros(H, M2, dtype=torch.complex128, device=dev)
        step = max(1, (chunk or CHUNK_SAMPLES) // M2)
        for s0 in range(0, x.shape[0], step):
            ze = torch.cat([self._ana, _c128(x[s0: s0 + step], dev).flip(1)])
            N = ze.shape[0] - H
            A = torch.zeros(N, M2, dtype=torch.complex128, device=dev)
            B = torch.zeros(N, M2, dtype=torch.complex128, device=dev)
            for n in range(p):
                A += hs[n, :M2] * ze[H - 2 * n: H - 2 * n + N]
                B += hs[n, M2:] * ze[H - 1 - 2 * n: H - 1 - 2 * n + N]
            odd = ((torch.arange(N, device=dev) + self._ana_steps) % 2 == 1)[:, None]
            X = torch.cat([torch.where(odd, B, A), torch.where(odd, A, B)], dim=1)
            self._ana = ze[N:].clone()
            self._ana_steps += N
            yield s0, torch.fft.ifft(X, dim=1)

    def synthesizer_chunks(self, X, chunk=None):
        """X: steps of M channel samples -> yields (first step, complex128 [steps, M/2] time samples)"""
        M, M2, p = self.M, self.M // 2, 2 * self.m
        H = 2 * p - 1
        X = torch.as_tensor(X).reshape(-1, M)
        dev = self.device if self.device is not None else X.device
        hs = self._hs(dev)
        hA, hB = hs[:, :M2].repeat(1, 2), hs[:, M2:].repeat(1, 2)
        if self._syn is None:
            self._syn = torch.zeros(H, M, dtype=torch.complex128, device=dev)
        step = max(1, (chunk or CHUNK_SAMPLES) // M)
        for s0 in range(0, X.shape[0], step):
            v = torch.fft.ifft(_c128(X[s0: s0 + step], dev), dim=1) * M2
            ve = torch.cat([self._syn, v])
            N = v.shape[0]
            F = torch.zeros(N, M, dtype=torch.complex128, device=dev)
            for n in range(p):
                F += hA[n] * ve[H - 2 * n: H - 2 * n + N] + hB[n] * ve[H - 1 - 2 * n: H - 1 - 2 * n + N]
            odd = ((torch.arange(N, device=dev) + self._syn_steps) % 2 == 1)[:, None]
            self._syn = ve[N:].clone()
            self._syn_steps += N
            yield s0, torch.where(odd, F[:, M2:], F[:, :M2])

    def analyzer_execute(self, x, chunk=None):
        return torch.cat([y for _, y in self.analyzer_chunks(x, chunk)])

    def synthesizer_execute(self, X, chunk=None):
        return torch.cat([y for _, y in self.synthesizer_chunks(X, chunk)])


class FrameCheck:
    """per-frame check ||y_f - r_f|| <= tau ||r_f|| + tau rho, rho = rms frame norm of the reference block.
    Feed it (first frame, reference chunk) pairs and the matching rows of the output under test."""

    def __init__(self, nframes, device=None):
        self.err = torch.zeros(nframes, dtype=torch.float64, device=device)
        self.ref = torch.zeros(nframes, dtype=torch.float64, device=device)

    def add(self, f0, ref, got):
        ref = ref.reshape(ref.shape[0], -1)
        got = torch.as_tensor(got).reshape(ref.shape[0], -1).to(device=ref.device, dtype=torch.complex128)
        n = ref.shape[0]
        self.err[f0: f0 + n] = torch.linalg.vector_norm(got - ref, dim=1).to(self.err.device)
        self.ref[f0: f0 + n] = torch.linalg.vector_norm(ref, dim=1).to(self.ref.device)

    def worst(self):
        """(worst ratio ||e_f|| / (||r_f|| + rho), its frame, global rel L2)"""
        rho = float(torch.sqrt(torch.mean(self.ref ** 2)))
        ratio = self.err / (self.ref + rho + 1e-300)
        f = int(torch.argmax(ratio))
        rel = float(torch.sqrt(torch.sum(self.err ** 2)) / (torch.sqrt(torch.sum(self.ref ** 2)) + 1e-300))
        return float(ratio[f]), f, rel
