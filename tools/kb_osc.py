#!/usr/bin/env python3
"""Osc block mixing (GPU box): mix_block_up_dev / mix_block_down_dev for both schemes on 2^20, 2^24 and 2^26-sample
blocks, at an ordinary frequency and at the adversarial strides of 16, 32, 64 and 512 table entries per sample (the
lanes of a wave on one LDS bank).  HIP events around 20 calls after 10 warm-up calls; reports
Gsample/s and the fraction of 8 TB/s at 16 B/sample (8 B in, 8 B out).
Usage: python tools/kb_osc.py [label]     (YAGI_HIP_LIB selects an A/B build of the library)"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
label = sys.argv[1] if len(sys.argv) > 1 else "default"


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


FREQS = [("ordinary f=0.1234", 2 * np.pi * 0.1234)] + [(f"stride {s:3d} entries", 2 * np.pi * s / 1024)
                                                        for s in (16, 32, 64, 512)]
print(f"# library: {label}")
print(f"{'scheme':6s} {'dir':4s} {'frequency':22s} {'n':>9s} {'ms':>9s} {'Gsample/s':>10s} {'of 8TB/s':>9s}")
for lg in (20, 24, 26):
    n = 1 << lg
    x = torch.randn(n, dtype=torch.complex64, device=dev)
    y = torch.empty_like(x)
    for scheme in (ya.OscScheme.Nco, ya.OscScheme.Vco):
        for down in (False, True):
            if down and lg != 24:
                continue
            for name, w in FREQS:
                q = ya.Osc(scheme)
                q.set_stream(st.cuda_stream)
                q.set_frequency(w)
                fn = q.mix_block_down_dev if down else q.mix_block_up_dev
                ms = timed(lambda: fn(x, n, y))
                print(f"{scheme.name:6s} {'down' if down else 'up':4s} {name:22s} {n:9d} {ms:9.4f} "
                      f"{n / ms / 1e6:10.1f} {16 * n / ms / 1e9 / 8:9.3f}", flush=True)
    del x, y
