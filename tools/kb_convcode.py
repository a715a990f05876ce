#!/usr/bin/env python3
"""ConvCode block forms (GPU box): decode_block_devptr and encode_block_devptr for v27, v29 and v27p34 at n in {256, 1024,
8192} message bits (where the code's limit allows) and F in {64, 4096, 65536} frames, on random soft bytes (no codewords:
every survivor decision is data dependent, as on a noisy link) and random messages.
Part 1 runs every shape at the planner's arrangement.  Part 2 sweeps the admissible arrangements (waves per workgroup, and
frames per wave where S < 64: a K = 5 code stands in for those) on the decoder; `plan` marks the planner's own choice.
Three rounds; a round is HIP events around ITERS calls after WARM warm-up calls; the table gives the fastest round, the
slowest / fastest spread, decoded (or encoded) Mbit/s of message and the algorithmic bytes moved per second (soft or coded
bytes, message bytes and the metric words).  At F = 64 the operands stay cache resident; from F = 4096 at n >= 1024 on they
exceed the L2 of an XCD, and at F = 65536 the Infinity Cache at n >= 1024.
Usage: python tools/kb_convcode.py [--quick]"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
QUICK = "--quick" in sys.argv
ROUNDS, WARM, ITERS = 3, 1, 3
CODES = (("v27", ya.ConvCode.v27), ("v29", ya.ConvCode.v29), ("v27p34", ya.ConvCode.v27p34))
NS = (256,) if QUICK else (256, 1024, 8192)
FS = (64,) if QUICK else (64, 4096, 65536)


def timed(fn):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(ITERS):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / ITERS)
    return min(t), max(t) / min(t)


class Shape:
    def __init__(self, name, make, n, F):
        self.name, self.n, self.F = name, n, F
        self.q = make()
        self.q.set_stream(st.cuda_stream)
        self.nb, self.nc = (n + 7) // 8, self.q.ncoded(n)
        self.soft = torch.randint(0, 256, (F * self.nc,), dtype=torch.uint8, device=dev)
        self.msg = torch.randint(0, 256, (F * self.nb,), dtype=torch.uint8, device=dev)
        self.coded = torch.empty(F * self.nc, dtype=torch.uint8, device=dev)
        self.out = torch.empty(F * self.nb, dtype=torch.uint8, device=dev)
        self.metric = torch.empty(F, dtype=torch.int32, device=dev)
        self.bytes = F * (self.nc + self.nb + 4)

    def decode(self):
        self.q.decode_block_devptr(self.soft, self.nc, self.n, self.F, self.out, self.nb, self.metric)

    def encode(self):
        self.q.encode_block_devptr(self.msg, self.nb, self.n, self.F, self.coded, self.nc)

    def row(self, what, fpw=0, waves=0):
        self.q.set_shape(fpw, waves)
        s = self.q.get_shape(self.n, self.F)
        if s["lds_bytes"] > 160 * 1024:                       # the arrangement does not hold frames this long
            self.q.set_shape(0, 0)
            return None
        self.q.set_shape(0, 0)
        plan = self.q.get_shape(self.n, self.F)
        self.q.set_shape(fpw, waves)
        best, spread = timed(self.decode if what == "decode" else self.encode)
        print(f"{self.name:>7s} {what:>6s} {self.n:5d} {self.F:6d} {s['frames_per_wave']:4d} {s['waves']:5d} "
              f"{'plan' if s == plan else '':>4s} {s['lds_bytes']:7d} {best:10.4f} {spread:6.3f} "
              f"{self.n * self.F / (best * 1e-3) / 1e6:10.1f} {self.bytes / (best * 1e-3) / 1e9:8.2f}", flush=True)
        return best


HEAD = (f"{'code':>7s} {'call':>6s} {'n':>5s} {'F':>6s} {'fpw':>4s} {'waves':>5s} {'':>4s} {'LDS':>7s} {'ms':>10s} {'spread':>6s} "
        f"{'Mbit/s':>10s} {'GB/s':>8s}")
print(f"# ms is the fastest of {ROUNDS} rounds of {ITERS} calls, spread the slowest over it; Mbit/s counts message bits; GB/s "
      f"is algorithmic (coded + message bytes + 4 per frame)")
print("# part 1: every shape at the planner's arrangement")
print(HEAD)
for name, make in CODES:
    for n in NS:
        if n > make().nmax():
            continue
        for F in FS:
            s = Shape(name, make, n, F)
            s.row("decode")
            s.row("encode")
            del s

print("# part 2: the decoder at every admissible arrangement")
print(HEAD)
K5 = ("k5", lambda: ya.ConvCode(5, (0x17, 0x19)))
for (name, make), fpws in ((CODES[0], (1,)), (CODES[1], (1,)), (K5, (1, 2, 4))):
    for n in NS:
        if n > make().nmax():
            continue
        for F in FS[1:] or FS:
            s = Shape(name, make, n, F)
            for fpw in fpws:
                for waves in (1, 2, 4):
                    s.row("decode", fpw, waves)
            del s
