#!/usr/bin/env python3
"""IirFilter block calls (GPU box): execute_block_dev on 2^16, 2^20 and 2^24-sample blocks, HIP events around 20
calls after 10 warm-up calls.  Reports Gsample/s, the fraction of 8 TB/s at the algorithmic 16 B/sample (crcf: x in,
y out; 8 B/sample for rrrf) and at the bytes the three phases move (x read twice, y written once, plus the chunk
states).  Usage: python tools/kb_iir.py [kind ...]   (default: rrrf crcf cccf)"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
TDT = {"rrrf": torch.float32, "crcf": torch.complex64, "cccf": torch.complex64}
CDT = {"rrrf": np.float32, "crcf": np.float32, "cccf": np.complex64}
SB = {"rrrf": 4, "crcf": 8, "cccf": 8}


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


def chunk_len(S):
    T = 64
    while T < 256 and T < 8 * S:
        T *= 2
    return T


def make(kind, form, order):
    if form == "sos":
        a = np.tile([1.0, -1.2, 0.5], order).astype(CDT[kind])
        b = np.tile([0.1, 0.2, 0.1], order).astype(CDT[kind])
        return ya.IirFilter.new_sos(kind, b, a, order), 2 * order, (order + 15) // 16
    a = np.poly(0.6 * np.exp(2j * np.pi * np.arange(order - 1) / (order - 1))).real if order > 1 else np.ones(1)
    return ya.IirFilter(kind, np.full(order, 0.1, CDT[kind]), a.astype(CDT[kind])), order - 1, 1


print(f"{'case':28s} {'n':>9s} {'ms':>9s} {'Gsample/s':>10s} {'alg 8TB/s':>10s} {'moved 8TB/s':>12s}")
for kind in sys.argv[1:] or ("rrrf", "crcf", "cccf"):
    for form, order in (("sos", 1), ("sos", 4), ("sos", 8), ("tf", 3), ("tf", 7)):
        q, S, groups = make(kind, form, order)
        q.set_stream(st.cuda_stream)
        for lg in (16, 20, 24):
            n = 1 << lg
            x = torch.randn(n, dtype=TDT[kind], device=dev)
            y = torch.empty_like(x)
            ms = timed(lambda: q.execute_block_dev(x, n, y))
            sb = SB[kind]
            T = chunk_len(S // groups if form == "sos" else S)
            moved = groups * (3 * sb * n + 2 * sb * S * n / T)     # per group: x twice, y once, z written and read
            alg = 2 * sb * n
            print(f"{kind} {form}{order:<3d}{'':18s} {n:9d} {ms:9.4f} {n / ms / 1e6:10.1f} {alg / ms / 1e9 / 8:10.3f} "
                  f"{moved / ms / 1e9 / 8:12.3f}")
            del x, y
