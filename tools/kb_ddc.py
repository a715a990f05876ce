#!/usr/bin/env python3
"""Ddc / Duc (GPU box): the fused launch (kernel choice auto) against the two-launch route of the same build
(set_kernel(1)) and against separate Osc + FirDecimationFilter / FirInterpolationFilter objects with a buffer in
between, which is what a caller had before the objects existed.  crcf, NCO, M or I in {2, 4, 8, 16}, 16 taps per phase,
2^24 and 2^26 full-rate samples.  HIP events around 20 calls after 10 warm-up calls; reports ms, the GB/s of the
object's algorithmic traffic (8 B per full-rate sample + 8 B per low-rate sample) and the ratios.
Usage: python tools/kb_ddc.py [label]     (YAGI_HIP_LIB selects an A/B build of the library)"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
label = sys.argv[1] if len(sys.argv) > 1 else "default"
FREQ = 2 * np.pi * 0.1234


def timed(fn):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(20):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 20


def on_stream(q):
    q.set_stream(st.cuda_stream)
    return q


print(f"# library: {label}")
print(f"{'object':6s} {'rate':>4s} {'full-rate n':>11s} {'kernel':>6s} {'fused ms':>9s} {'GB/s':>7s} {'2-launch ms':>11s} {'GB/s':>7s} "
      f"{'parts ms':>9s} {'GB/s':>7s} {'2l/fused':>8s} {'parts/fused':>11s}")
for lg in (24, 26):
    n_full = 1 << lg
    full = torch.randn(n_full, dtype=torch.complex64, device=dev)
    mid = torch.empty_like(full)
    for obj in ("Ddc", "Duc"):
        for rate in (2, 4, 8, 16):
            h = ya.fir_design_kaiser(16 * rate, 0.4 / rate, 60.0)
            n_low = n_full // rate
            low = torch.randn(n_low, dtype=torch.complex64, device=dev)
            nbytes = 8 * (n_full + n_low)
            osc = on_stream(ya.Osc(ya.OscScheme.Nco))
            osc.set_frequency(FREQ)
            ms = {}
            if obj == "Ddc":
                fir = on_stream(ya.FirDecimationFilter("crcf", rate, h))
                for choice in (0, 1):
                    q = on_stream(ya.Ddc("crcf", ya.OscScheme.Nco, rate, h))
                    q.set_frequency(FREQ)
                    q.set_kernel(choice)
                    ms[choice] = timed(lambda: q.execute_block_devptr(full, n_low, low))
                    if choice == 0:
                        kernel = q.get_last_kernel()

                def parts():
                    osc.mix_block_down_dev(full, n_full, mid)
                    fir.execute_block_dev(mid, n_low, low)
            else:
                fir = on_stream(ya.FirInterpolationFilter("crcf", rate, h))
                for choice in (0, 1):
                    q = on_stream(ya.Duc("crcf", ya.OscScheme.Nco, rate, h))
                    q.set_frequency(FREQ)
                    q.set_kernel(choice)
                    ms[choice] = timed(lambda: q.execute_block_devptr(low, n_low, full))
                    if choice == 0:
                        kernel = q.get_last_kernel()

                def parts():
                    fir.execute_block_dev(low, n_low, mid)
                    osc.mix_block_up_dev(mid, n_full, full)
            ms["parts"] = timed(parts)
            gbs = {k: nbytes / v / 1e6 for k, v in ms.items()}
            print(f"{obj:6s} {rate:4d} {n_full:11d} {kernel:6d} {ms[0]:9.4f} {gbs[0]:7.0f} {ms[1]:11.4f} {gbs[1]:7.0f} "
                  f"{ms['parts']:9.4f} {gbs['parts']:7.0f} {ms[1] / ms[0]:8.2f} {ms['parts'] / ms[0]:11.2f}", flush=True)
            del low
    del full, mid
