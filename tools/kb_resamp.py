#!/usr/bin/env python3
"""Resamp / MsResamp block calls (GPU box): execute_block_dev / execute_dev on 2^26-input crcf blocks, HIP events
around 20 calls after 10 warm-up calls.  Algorithmic bytes: 8 nx + 8 ny (crcf, cccf), 4 nx + 4 ny (rrrf), reported as
a fraction of 8 TB/s.  Usage: python tools/kb_resamp.py [log2 of the block length, default 26]"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 26)
x = torch.empty(n, dtype=torch.complex64, device=dev)
ya.gen_complex_dev(5, n, out=x, stream=st.cuda_stream)


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


def report(name, q, call, rate):
    q.set_stream(st.cuda_stream)
    cap = int(n * rate * 1.01) + 64
    y = torch.empty(cap, dtype=torch.complex64, device=dev)
    ny = q.get_num_output(n)
    ms = timed(lambda: call(x, n, y, cap))
    tbs = 8 * (n + ny) / 1e9 / ms                   # GB per ms = TB/s
    print(f"{name:44s} {ms:8.4f} ms  {n / ms / 1e6:7.1f} Gsamples/s in  {ny / ms / 1e6:7.1f} out  {tbs:5.2f} TB/s  "
          f"{tbs / 8:5.3f} of 8 TB/s")
    del y


for rate in (0.3, 0.9, 1.1, 3.7):
    q = ya.Resamp.new_default("crcf", rate)
    report(f"resamp_crcf default (m 7, npfb 256) r={rate}", q, q.execute_block_dev, rate)
q = ya.Resamp("crcf", 0.9, 20, 0.45, 60.0, 2048)
report("resamp_crcf m 20, npfb 2048 r=0.9", q, q.execute_block_dev, 0.9)
for rate in (0.127, 7.3):
    q = ya.MsResamp("crcf", rate, 60.0)
    _, s, ra = q.get_params()
    report(f"msresamp_crcf r={rate} ({s} stages, arb {ra:.4f})", q, q.execute_dev, rate)
