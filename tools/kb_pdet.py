#!/usr/bin/env python3
"""PreambleDetector block form (GPU box): detect_block_devptr at (L, K) in {(64, 8), (256, 16), (1024, 32)}, threshold 0.6,
on one block of 2^24 samples of N(0, 1) noise (the operating point: no hit, nothing written but the tile table), beside
what a caller could assemble without the object: K FirFilter("cccf") block calls with the reversed templates as taps,
each writing a full-rate stream, plus Autocorr(L, 0) with the energy output.  That composition is a timing comparator
only: FirFilter runs its default direct forms, whose sums are fused multiply-adds (half the instructions per tap), so
its words differ from the detector's, and the thresholding and peak picking a caller would still have to do are not in it.
Three rounds, the two sides alternating inside each; a round is HIP events around ITERS calls after WARM warm-up calls; the
table gives the fastest round and the slowest / fastest spread.  `ceiling` is the derived bound of DESIGN.md section 4:
8 unfused f32 operations per tap, hypothesis and sample against half the f32 FMA rate of the VALUs: from 53.5 T
operations per second (half the 107 TFLOP/s measured for VALU FMA) to 78.6 T (half the 157.3 TFLOP/s peak).  events /
overflow are the status words of the last call.
Usage: python tools/kb_pdet.py"""
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
CAP = 1 << 16
VALU_OPS = (53.5e12, 78.6e12)                                        # unfused f32 operations per second, low and high


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


rng = np.random.default_rng(1)
noise = torch.randn(N, dtype=torch.complex64, device=dev)
y = torch.empty(N, dtype=torch.complex64, device=dev)               # every filter's stream goes here: written, never read
rxx = torch.empty(N, dtype=torch.complex64, device=dev)
en = torch.empty(N, dtype=torch.float32, device=dev)
events = torch.empty(CAP * ya.PREAMBLE_EVENT.itemsize, dtype=torch.uint8, device=dev)
status = torch.zeros(2, dtype=torch.int32, device=dev)


def row(L, K):
    warm, iters = {64: (3, 10), 256: (2, 4), 1024: (1, 2)}[L]
    p = np.exp(1j * np.pi / 2 * rng.integers(0, 4, L)).astype(np.complex64)
    dphi = np.linspace(-0.5 / L * K, 0.5 / L * K, K).astype(np.float32)
    q = ya.PreambleDetector(p, dphi, 0.6)
    V = q.get_templates()
    firs = [ya.FirFilter("cccf", np.ascontiguousarray(V[k][::-1])) for k in range(K)]   # y[n] = sum_i v[i] x[n-L+1+i]
    ac = ya.Autocorr("cccf", L, 0)
    for o in [q, ac] + firs:
        o.set_stream(st.cuda_stream)
    fused = lambda: q.detect_block_devptr(noise, N, events, CAP, status)

    def composed():
        for f in firs:
            f.execute_block_dev(noise, N, y)
        ac.execute_block_devptr(noise, N, rxx, en)

    tf, tc = [], []
    for _ in range(ROUNDS):
        tf.append(timed(fused, warm, iters))
        tc.append(timed(composed, warm, iters))
    count, over = (int(v) for v in status.cpu())
    ff, fc = min(tf), min(tc)
    ops = 8.0 * L * K
    lo, hi = (v / ops / 1e9 for v in VALU_OPS)
    print(f"{L:5d} {K:3d} {ff:10.4f} {max(tf) / ff:7.3f} {fc:10.4f} {max(tc) / fc:7.3f} {ff / fc:9.3f} {N / ff / 1e6:9.3f} "
          f"{lo:6.2f}-{hi:<6.2f} {N / ff / 1e6 / hi:7.2f} {count:7d} {over:8d}", flush=True)


print(f"# one block of {N} samples of noise, threshold 0.6; ms is the fastest of {ROUNDS} rounds, spread the slowest over it")
print(f"{'L':>5s} {'K':>3s} {'fused ms':>10s} {'spread':>7s} {'compos ms':>10s} {'spread':>7s} {'fused/co':>9s} {'Gsmp/s':>9s} "
      f"{'ceiling Gsmp/s':>13s} {'of it':>7s} {'events':>7s} {'overflow':>8s}")
for L, K in ((64, 8), (256, 16), (1024, 32)):
    row(L, K)
