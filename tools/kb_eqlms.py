#!/usr/bin/env python3
"""EqLms block form (GPU box): decim_block_devptr at C = 4096 channels, k = 2, in each update mode at h_len = 29 and at
h_len = 128.  The input is noise smoothed over three samples (an oversampled signal; on white input the update after the
k - 1 trailing pushes sees a window uncorrelated with the error and the weights wander off), TRAIN's symbols are the
sample the default tap selects, DECISION runs against the 16-QAM table; `finite` says the weights stayed finite.
Three rounds; a round is HIP events around ITERS calls after WARM warm-up calls (the state is carried from call to call,
as in a stream); the table gives the fastest round and the slowest / fastest spread, in millions of channel-symbols per
second.
Beside it two bounds, derived and not measured, both per symbol and wave from the built kernel:
  VALU   issue cycles of the two inner loops as tools/isa_stats.py and the listing count them: the sum takes 17 VALU
         instructions per 4 taps, the update 134 per 4 taps of which 112 are f64 and 8 are v_rcp_f64; an instruction is
         taken as 4 cycles for a wave of 64 and a v_rcp_f64 as 16 (quarter rate), so a tap costs 17 cycles in the sum and
         158 in the update; one wave per SIMD, ceil(C / 64) of the chip's 1024 SIMDs busy, 2.4 GHz
  LDS    16 bytes per tap and lane for the sum (w and r), 24 more for the update (r, w, w back): 40 bytes, against 128
         bytes per clock and CU, ceil(C / 64) of 256 CUs busy
Usage: python tools/kb_eqlms.py"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
ROUNDS, WARM, ITERS = 3, 1, 3
C, K = 4096, 2
CLOCK = 2.4e9
SUM_CYCLES, UPD_CYCLES = 17.0, (134 - 8) * 4 / 4 + 8 * 16 / 4       # per tap and wave
LDS_SUM, LDS_UPD, LDS_RATE = 16.0, 24.0, 128.0                      # bytes per tap and lane; bytes per clock and CU
U = ya.EqLmsUpdate


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


def row(h_len, mode, nsym):
    n = nsym * K
    q = ya.EqLms(C, h_len)
    q.set_stream(st.cuda_stream)
    q.set_bw(0.05)
    pts = np.array([-3, -1, 1, 3]) / np.sqrt(10.0)
    q.set_constellation((pts[:, None] + 1j * pts[None, :]).reshape(-1).astype(np.complex64))
    s = torch.randn(n, C, dtype=torch.complex64, device=dev) * 0.35
    x = (s + 0.5 * (torch.roll(s, 1, 0) + torch.roll(s, -1, 0))).contiguous()
    lag = h_len - 1 - h_len // 2                                     # y of the default tap is x[i k - lag]
    d = x[(torch.arange(nsym, device=dev) * K - lag).clamp(min=0)].contiguous()
    y = torch.empty(nsym * C, dtype=torch.complex64, device=dev)

    def call():
        q.decim_block_devptr(K, mode, x, C, n, d if mode == U.TRAIN else None, C, y, C)

    t = [timed(call, WARM, ITERS) for _ in range(ROUNDS)]
    best = min(t)
    rate = nsym * C / (best * 1e-3)                                  # channel-symbols per second
    waves = -(-C // 64)
    upd = mode != U.NONE
    valu = min(waves, 1024) * 64 * CLOCK / (h_len * (SUM_CYCLES + (UPD_CYCLES if upd else 0.0)))
    lds = min(waves, 256) * 64 * CLOCK / (h_len * (LDS_SUM + (LDS_UPD if upd else 0.0)) * 64 / LDS_RATE)
    finite = bool(np.isfinite(q.get_coefficients()).all())
    print(f"{h_len:5d} {mode.name:>9s} {nsym:7d} {best:10.3f} {max(t) / best:7.3f} {rate / 1e6:10.1f} {valu / 1e6:10.0f} "
          f"{lds / 1e6:10.0f} {rate / min(valu, lds):7.3f} {'VALU' if valu < lds else 'LDS':>6s} {str(finite):>7s}", flush=True)


print(f"# decim_block, C = {C}, k = {K}; ms is the fastest of {ROUNDS} rounds of {ITERS} calls, spread the slowest over it; "
      f"Msym/s counts channel-symbols")
print(f"{'h_len':>5s} {'mode':>9s} {'nsym':>7s} {'ms':>10s} {'spread':>7s} {'Msym/s':>10s} {'VALU bound':>10s} {'LDS bound':>10s} "
      f"{'of it':>7s} {'bound':>6s} {'finite':>7s}")
for h_len, nsym in ((29, 8192), (128, 2048)):
    for mode in (U.NONE, U.TRAIN, U.BLIND, U.DECISION):
        row(h_len, mode, nsym)
