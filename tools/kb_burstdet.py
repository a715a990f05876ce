#!/usr/bin/env python3
"""BurstDetector block form (GPU box): detect_block_devptr at W in {16, 64, 256, 1024} with d = W and threshold 0.5 on one
block of 2^24 samples, cccf and rrrf, beside Autocorr.execute_block_devptr with the energy output on the same block: the
same sums, but two full-rate streams out where the detector writes events.
Three inputs and a fourth for the record:
  noise      N(0, 1) samples, the operating point: no hit for W >= 64, nothing written but the tile table.  At W = 16
             noise alone crosses the threshold often enough that the call overflows its segment pool (the status says so).
  quiet      W <= 64, for the record: the same noise under an energy floor of 1e30, so that no sample is a hit and the
             call is the tile kernel's no-hit path and an empty stitch (no bar)
  all-hit    a period-d stream of constant modulus: every sample after the first W + d is a hit, one segment per tile,
             one run that stays pending from call to call
  half-dense W = 1, d = 0 on 1, 0, 1, 0, ...: 1024 one-sample segments per tile (its own two rows; the call overflows)
Three rounds, the two objects alternating inside each; a round is HIP events around ITERS calls after WARM warm-up calls;
the table gives the fastest round and the slowest / fastest spread.  `bar` is the Autocorr time multiplied by its own
spread: on the noise rows the detector is to be no slower than that.  all-hit / half-dense get no bar; their times show
that the cost does not grow with the length of a run.  events / overflow are the status words of the last call.
Usage: python tools/kb_burstdet.py"""
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
noise = {"cccf": torch.randn(N, dtype=torch.complex64, device=dev), "rrrf": torch.randn(N, dtype=torch.float32, device=dev)}
rxx = {"cccf": torch.empty(N, dtype=torch.complex64, device=dev), "rrrf": torch.empty(N, dtype=torch.float32, device=dev)}
en = torch.empty(N, dtype=torch.float32, device=dev)
events = torch.empty(CAP * ya.BURST_EVENT.itemsize, dtype=torch.uint8, device=dev)
status = torch.zeros(2, dtype=torch.int32, device=dev)


def periodic(kind, d):
    k = np.arange(N) % d
    if kind == "cccf":
        return torch.from_numpy(np.exp(1j * rng.uniform(0, 2 * np.pi, d))[k].astype(np.complex64)).to(dev)
    return torch.from_numpy(rng.choice([-1.0, 1.0], d)[k].astype(np.float32)).to(dev)


def alternating(kind):
    x = np.zeros(N, np.complex64 if kind == "cccf" else np.float32)
    x[::2] = 1
    return torch.from_numpy(x).to(dev)


def row(kind, W, d, label, x, floor=0.0):
    heavy = W >= 256
    warm, iters = (2, 4) if heavy else (5, 20)
    b = ya.BurstDetector(kind, W, d, 0.5, floor)
    a = ya.Autocorr(kind, W, d)
    for o in (a, b):
        o.set_stream(st.cuda_stream)
    burst = lambda: b.detect_block_devptr(x, N, events, CAP, status)
    auto = lambda: a.execute_block_devptr(x, N, rxx[kind], en)
    tb, ta = [], []
    for _ in range(ROUNDS):
        tb.append(timed(burst, warm, iters))
        ta.append(timed(auto, warm, iters))
    count, over = (int(v) for v in status.cpu())
    fb, fa = min(tb), min(ta)
    bar = max(ta)                                                   # the fastest round times the slowest / fastest spread
    verdict = ("ok" if fb <= bar else "MISSED") if label == "noise" else "-"
    print(f"{kind:>5s} {W:5d} {label:>10s} {fb:9.4f} {max(tb) / fb:7.3f} {fa:9.4f} {max(ta) / fa:7.3f} {fb / fa:9.3f} "
          f"{bar:9.4f} {verdict:>7s} {N / fb / 1e3:9.1f} {count:8d} {over:8d}", flush=True)


print(f"# one block of {N} samples, threshold 0.5; ms is the fastest of {ROUNDS} rounds, spread the slowest over it")
print(f"{'kind':>5s} {'W':>5s} {'input':>10s} {'burst ms':>9s} {'spread':>7s} {'autoc ms':>9s} {'spread':>7s} {'burst/ac':>9s} "
      f"{'bar ms':>9s} {'noise':>7s} {'Msmp/s':>9s} {'events':>8s} {'overflow':>8s}")
for W in (16, 64, 256, 1024):
    for kind in ("cccf", "rrrf"):
        row(kind, W, W, "noise", noise[kind])
        if W <= 64:
            row(kind, W, W, "quiet", noise[kind], floor=1e30)
        row(kind, W, W, "all-hit", periodic(kind, W))
for kind in ("cccf", "rrrf"):
    row(kind, 1, 0, "half-dense", alternating(kind))
