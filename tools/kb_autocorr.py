#!/usr/bin/env python3
"""Autocorr block form (GPU box): execute_block_devptr at W in {16, 64, 256, 1024} with d = W on one block of 2^24
samples, cccf and rrrf, with and without the energy output, beside the general direct-form cccf FirFilter kernel
(set_kernel(1)) at L = W on the same block: the same W complex products per output on paper.  Autocorr forms each
product once per sample and then only adds (autocorr_kernels.hip), so what it does per output is W complex adds, W + 1
with the energy.
Three rounds, the calls alternating inside each; a round is HIP events around ITERS calls after WARM warm-up calls; the
table gives the fastest round and the slowest / fastest spread.
Msmp/s is samples over time.  Gadd/s is the kernel's own work, W packed adds of two floats per output (W more f32 adds
with the energy for cccf; rrrf carries the energy in the same packed add), to be read against the packed-f32 vector
rate.  GB/s is algorithmic bytes over time: the samples in, rxx (and the energy) out.
Usage: python tools/kb_autocorr.py"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
ROUNDS = 3
N = 1 << 24


def timed(fn, warm, iters):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


xc = torch.randn(N, dtype=torch.complex64, device=dev)
yc = torch.empty(N, dtype=torch.complex64, device=dev)
xr = torch.randn(N, dtype=torch.float32, device=dev)
yr = torch.empty(N, dtype=torch.float32, device=dev)
en = torch.empty(N, dtype=torch.float32, device=dev)
rng = np.random.default_rng(1)

print(f"# one block of {N} samples, d = W; ms is the fastest of {ROUNDS} rounds, spread the slowest over it")
print(f"{'kind':>5s} {'W':>5s} {'energy':>6s} {'ms':>9s} {'spread':>7s} {'Msmp/s':>9s} {'Gadd/s':>8s} {'GB/s':>7s} "
      f"{'fir ms':>9s} {'spread':>7s} {'fir Msmp/s':>11s} {'autocorr/fir':>13s}")
for W in (16, 64, 256, 1024):
    h = (rng.standard_normal(W) + 1j * rng.standard_normal(W)).astype(np.complex64)
    fir = ya.FirFilter("cccf", h)
    fir.set_stream(st.cuda_stream)
    fir.set_kernel(1)
    fir_call = lambda: fir.execute_block_dev(xc, N, yc)
    heavy = W >= 256
    warm, iters = (2, 4) if heavy else (5, 20)
    rows = []
    for kind, x, y, esz in (("cccf", xc, yc, 8), ("rrrf", xr, yr, 4)):
        for with_e in (False, True):
            q = ya.Autocorr(kind, W, W)
            q.set_stream(st.cuda_stream)
            call = (lambda q=q, x=x, y=y: q.execute_block_devptr(x, N, y, en)) if with_e else \
                   (lambda q=q, x=x, y=y: q.execute_block_devptr(x, N, y))
            rows.append((kind, with_e, esz, q, call, []))
    fir_ms = []
    for _ in range(ROUNDS):
        for row in rows:
            row[5].append(timed(row[4], warm, iters))
        fir_ms.append(timed(fir_call, 1 if heavy else 3, 2 if heavy else 10))
    tf = min(fir_ms)
    for kind, with_e, esz, q, call, ms in rows:
        t = min(ms)
        adds = W * (2 if (kind == "cccf" and with_e) else 1)
        gbs = N * (2 * esz + (4 if with_e else 0)) / t / 1e6
        print(f"{kind:>5s} {W:5d} {'yes' if with_e else 'no':>6s} {t:9.4f} {max(ms) / t:7.3f} {N / t / 1e3:9.1f} "
              f"{adds * N / t / 1e6:8.1f} {gbs:7.1f} {tf:9.3f} {max(fir_ms) / tf:7.3f} {N / tf / 1e3:11.1f} {t / tf:13.4f}",
              flush=True)
    del rows, fir
