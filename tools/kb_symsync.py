#!/usr/bin/env python3
"""SymSync block form (GPU box): execute_devptr with the Arkaiser design k = 2, m = 7, beta = 0.35, npfb = 32 (Ls = 28) on
C in {64, 1024, 16384} channels, n chosen so that C n = 2^24 samples, of N(0, 0.5) noise scaled by 0.1 so that the loop
neither clamps nor stalls (`stalled` is the count of stalled channels after the last call: it must read 0).  Beside it, as
a timing comparator only, execute_host over the same block on one core: the same words, one channel after the other.
Three rounds; a round is HIP events around ITERS calls after WARM warm-up calls (the state is carried from call to call, as
in a stream); the table gives the fastest round and the slowest / fastest spread.  `ceiling` is
derived, not measured: 8 unfused f32 operations per tap and output for the two sums, k_out / k
outputs per sample, against half the f32 FMA rate of the VALUs -- 53.5 T operations per second (half the 107 TFLOP/s
measured for VALU FMA) to 78.6 T (half the 157.3 TFLOP/s peak) -- scaled by the share of the chip's 1024 SIMDs that
ceil(C / 64) one-wave workgroups can occupy.
Usage: python tools/kb_symsync.py [--no-host]"""
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
ROUNDS, WARM, ITERS = 3, 1, 2
TOTAL = 1 << 24
K, M, BETA, NPFB = 2, 7, 0.35, 32
SIMDS = 1024
VALU_OPS = (53.5e12, 78.6e12)                                        # unfused f32 operations per second, low and high
HOST = "--no-host" not in sys.argv


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


def row(C):
    n = TOTAL // C
    q = ya.SymSync.rnyquist(C, ya.FirFilterShape.Arkaiser, K, M, BETA, NPFB)
    q.set_stream(st.cuda_stream)
    ls = q.branch_length
    x = (torch.randn(n, C, dtype=torch.complex64, device=dev) * 0.1).contiguous()
    ycap = q.default_ycap(n)
    y = torch.empty(ycap * C, dtype=torch.complex64, device=dev)
    status = torch.zeros(2 * C, dtype=torch.int32, device=dev)

    def call():
        q.execute_devptr(x, C, n, y, C, ycap, status)

    t = [timed(call, WARM, ITERS) for _ in range(ROUNDS)]
    s = status.cpu().numpy()
    best = min(t)
    ops = 8.0 * ls / K                                               # per input sample, k_out = 1
    share = min(-(-C // 64), SIMDS) / SIMDS
    lo, hi = (v * share / ops / 1e6 for v in VALU_OPS)
    rate = TOTAL / best / 1e3
    host = float("nan")
    if HOST:
        h = ya.SymSync.rnyquist_taps(ya.FirFilterShape.Arkaiser, K, M, BETA, NPFB)
        xh = x.cpu().numpy()
        t0 = time.perf_counter()
        ya.SymSync.execute_host(C, K, NPFB, h, xh, ycap)
        host = TOTAL / (time.perf_counter() - t0) / 1e6
    print(f"{C:6d} {n:7d} {best:10.3f} {max(t) / best:7.3f} {rate:10.1f} {lo:9.0f}-{hi:<9.0f} {rate / hi:7.3f} {host:10.1f} "
          f"{rate / host:8.1f} {int(s[:C].min()):7d}-{int(s[:C].max()):<7d} {int(s[C:].sum()):7d}", flush=True)


print(f"# Arkaiser k = {K}, m = {M}, beta = {BETA}, npfb = {NPFB}; C n = {TOTAL} samples; ms is the fastest of {ROUNDS} rounds, "
      f"spread the slowest over it")
print(f"{'C':>6s} {'n':>7s} {'ms':>10s} {'spread':>7s} {'Msmp/s':>10s} {'ceiling Msmp/s':>19s} {'of it':>7s} {'host Msmp/s':>10s} "
      f"{'dev/host':>8s} {'ny':>15s} {'stalled':>7s}")
for C in (64, 1024, 16384):
    row(C)
