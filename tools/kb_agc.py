#!/usr/bin/env python3
"""Agc block form (GPU box): execute_block_devptr, crcf, at C = 64, 4096 and 65536 channels, squelch off / on, status
plane off / on.  The input is unit-power noise at per-channel levels spread over 1e-4 .. 1e2, so every lane runs the
ln / exp branch on every sample; bandwidth 0.01, threshold -50 dB.
Three rounds; a round is HIP events around ITERS calls after WARM warm-up calls (the state is carried from call to call,
as in a stream); the table gives the fastest round and the slowest / fastest spread, in millions of channel-samples per
second, and the cycles one wave spends per sample at 2.4 GHz where every wave has a SIMD of its own (C <= 65536: at most
1024 waves on 1024 SIMDs).
Usage: python tools/kb_agc.py"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
ROUNDS, WARM, ITERS = 3, 2, 10
CLOCK = 2.4e9
ROWS = {64: 8192, 4096: 4096, 65536: 1024}


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


def row(C, squelch, status):
    n = ROWS[C]
    q = ya.Agc(C, "crcf")
    q.set_stream(st.cuda_stream)
    q.set_bandwidth(0.01)
    q.squelch_set_threshold(-50.0)
    if squelch:
        q.squelch_enable()
    amp = 10.0 ** (-4.0 + 6.0 * torch.rand(C, device=dev))
    x = (torch.randn(n, C, dtype=torch.complex64, device=dev) * amp).contiguous()
    y = torch.empty_like(x)
    plane = torch.empty(n, C, dtype=torch.uint8, device=dev) if status else None

    def call():
        q.execute_block_devptr(x, C, n, y, C, plane, C)

    t = [timed(call, WARM, ITERS) for _ in range(ROUNDS)]
    best = min(t)
    rate = n * C / (best * 1e-3)
    cycles = best * 1e-3 * CLOCK / n
    finite = bool(torch.isfinite(torch.view_as_real(y)).all())
    print(f"{C:7d} {str(squelch):>7s} {str(status):>6s} {n:6d} {best:10.3f} {max(t) / best:7.3f} {rate / 1e6:12.1f} "
          f"{cycles:10.0f} {str(finite):>7s}", flush=True)


print(f"# execute_block_devptr, crcf; ms is the fastest of {ROUNDS} rounds of {ITERS} calls, spread the slowest over it; "
      f"Msample/s counts channel-samples; cycles = per sample and wave at 2.4 GHz")
print(f"{'C':>7s} {'squelch':>7s} {'status':>6s} {'rows':>6s} {'ms':>10s} {'spread':>7s} {'Msample/s':>12s} {'cycles':>10s} "
      f"{'finite':>7s}")
for C in (64, 4096, 65536):
    for squelch in (False, True):
        for status in (False, True):
            row(C, squelch, status)
