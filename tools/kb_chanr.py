#!/usr/bin/env python3
"""FirPfbChr (GPU box): the general analyzer kernel (set_kernel(1)) against the column kernel (set_kernel(2)) at every
shape the column kernel serves -- M in {64, 128, 256}, P = a M / 8 for a = 1 .. 8, 2m = 4, 8, 16 taps per branch (the
three built branch lengths) -- on blocks of 2^24 and 2^20 input samples; `best` is the faster of the two, `auto` what
kernel choice 0 took (SLOWER marks a row where auto took the column kernel and the general one was faster); and the
synthesizer (transform + combine launches).  HIP events around 20 calls after 10 warm-up calls; reports ms and the GB/s
of the object's algorithmic traffic (analyzer 8 + 8 M/P bytes per input sample, synthesizer 8 M/P + 8 per output sample).
The last column is what tools/kb_stream_probe reached for the nearest read : write mix (profiles/r11_stream_probe.txt).
Usage: python tools/kb_chanr.py [label]     (YAGI_HIP_LIB selects an A/B build of the library)"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
label = sys.argv[1] if len(sys.argv) > 1 else "default"
# write words per read word -> TB/s of the copy probe with that mix (profiles/r11_stream_probe.txt, plain stores)
PROBE = {1: 5.57, 2: 5.40, 4: 5.01, 8: 5.26}


def probe(ratio):
    k = min(PROBE, key=lambda r: abs(np.log2(r) - np.log2(ratio)))
    return f"1:{k} {PROBE[k]:.2f} TB/s"


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


def proto(M, m, fc):
    h = ya.fir_design_kaiser(2 * M * m + 1, fc, 60.0)
    return (h * M / h.sum()).astype(np.float32)


def analyzer(M, P, m, n_in):
    ns = n_in // P
    x = torch.randn(ns * P, dtype=torch.complex64, device=dev)
    y = torch.empty(ns * M, dtype=torch.complex64, device=dev)
    h = proto(M, m, 0.5 / P)
    ms = {}
    for choice in (1, 2, 0):
        q = ya.FirPfbChr(M, P, m, h)
        q.set_stream(st.cuda_stream)
        q.set_kernel(choice)
        ms[choice] = timed(lambda: q.analyzer_execute_devptr(x, ns, y))
        if choice == 0:
            auto = q.get_last_kernel()
    nbytes = 8 * ns * (P + M)
    best = 2 if ms[2] < ms[1] else 1
    print(f"ana {M:4d} {P:4d} {2 * m:3d} {ns * P:9d} {ms[1]:9.4f} {nbytes / ms[1] / 1e6:7.0f} {ms[2]:9.4f} {nbytes / ms[2] / 1e6:7.0f} "
          f"{ms[1] / ms[2]:8.2f} {best:4d} {auto:4d} {'SLOWER' if auto == 2 and best == 1 else '':8s} {probe(M / P)}", flush=True)


def synthesizer(M, P, m, n_out):
    ns = n_out // P
    X = torch.randn(ns * M, dtype=torch.complex64, device=dev)
    y = torch.empty(ns * P, dtype=torch.complex64, device=dev)
    q = ya.FirPfbChr(M, P, m, proto(M, m, 0.5 / M))
    q.set_stream(st.cuda_stream)
    t = timed(lambda: q.synthesizer_execute_devptr(X, ns, y))
    nbytes = 8 * ns * (P + M)
    print(f"syn {M:4d} {P:4d} {2 * m:3d} {ns * P:9d} {t:9.4f} {nbytes / t / 1e6:7.0f}", flush=True)


print(f"# library: {label}")
print(f"{'op':3s} {'M':>4s} {'P':>4s} {'2m':>3s} {'samples':>9s} {'gen ms':>9s} {'GB/s':>7s} {'col ms':>9s} {'GB/s':>7s} {'gen/col':>8s} "
      f"{'best':>4s} {'auto':>4s} {'':8s} probe")
for lg in (24, 20):
    for M in (64, 128, 256):
        for m in (2, 4, 8):
            for a in range(1, 9):
                analyzer(M, a * M // 8, m, 1 << lg)
print(f"{'op':3s} {'M':>4s} {'P':>4s} {'2m':>3s} {'samples':>9s} {'ms':>9s} {'GB/s':>7s}")
for lg in (24, 20):
    for M, P, m in ((64, 48, 4), (64, 16, 4), (128, 80, 2), (256, 192, 4), (256, 192, 8), (512, 384, 4), (100, 75, 5)):
        synthesizer(M, P, m, 1 << lg)
