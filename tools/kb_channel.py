#!/usr/bin/env python3
"""Channel block forms (GPU box): execute_devptr / execute_bcast_devptr for channels in {1, 64, 4096, 65536} at 2^24 and
2^26 output samples in all, L in {1, 8, 32}, pitched and broadcast input, with noise (set_awgn) and with nstd = 0.
Part 1 runs every shape at the planner's arrangement.  Part 2 sweeps the arrangements (links per workgroup row x outputs
per lane, set_shape) at 2^26 outputs, pitched; `plan` marks the planner's own choice.  Part 3, at channels = 1, times
the composed route on the same build (FirFilter cccf -> Osc.mix_block_up -> scale -> gen_complex_dev -> add, torch for
the two elementwise steps) beside the fused kernel.
Three rounds; a round is HIP events around ITERS calls after WARM warm-up calls; the table gives the fastest round, the
slowest / fastest spread, and the algorithmic traffic over that time: 16 B per output pitched, 8 B per output broadcast.
Usage: python tools/kb_channel.py [--quick]"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
QUICK = "--quick" in sys.argv
ROUNDS, WARM, ITERS = 3, 2, 5
BANKS, TAPS = (1, 64, 4096, 65536), (1, 8, 32)
TOTALS = (1 << 16,) if QUICK else (1 << 24, 1 << 26)
LINKS, ROWS = (1, 2, 4, 8, 16, 32, 64), (1, 2, 4, 8, 16)


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


def taps(L, c):
    r = np.random.default_rng(c)
    return ((r.standard_normal(L) + 1j * r.standard_normal(L)) * 0.7 ** np.arange(L)).astype(np.complex64)


def bank(C, L, noise):
    q = ya.Channel(C, L)
    q.set_stream(st.cuda_stream)
    q.set_seed(1)
    q.set_multipath_all(np.stack([taps(L, i) for i in range(16)])[np.arange(C) % 16])
    q.set_carrier_offset_all(np.full(C, 0.0123, np.float32), np.zeros(C, np.float32))
    if noise:
        q.set_awgn_all(np.full(C, -20.0, np.float32), np.full(C, 10.0, np.float32))
    return q


class Shape:
    def __init__(self, C, L, total, bcast, noise):
        self.C, self.L, self.n, self.bcast, self.noise = C, L, total // C, bcast, noise
        self.q = bank(C, L, noise)
        self.x = torch.randn(self.n if bcast else self.n * C, dtype=torch.complex64, device=dev)
        self.y = torch.empty(self.n * C, dtype=torch.complex64, device=dev)

    def call(self):
        if self.bcast:
            self.q.execute_bcast_devptr(self.x, self.n, self.y, self.C)
        else:
            self.q.execute_devptr(self.x, self.C, self.n, self.y, self.C)

    def row(self, links=0, rows=0):
        self.q.set_shape(links, rows)
        s = self.q.get_shape(self.n, self.bcast)
        plan = ya.channel_plan(self.C, self.L, self.n, bcast=self.bcast)
        best, spread = timed(self.call)
        tbs = self.n * self.C * (8 if self.bcast else 16) / (best * 1e-3) / 1e12
        print(f"{self.C:6d} {self.L:3d} {self.n:9d} {'bcast' if self.bcast else 'pitch':>5s} {'on' if self.noise else 'off':>5s} "
              f"{s['links']:5d} {s['rows']:4d} {'plan' if s == plan else '':>4s} {s['lds_bytes']:7d} {best:9.4f} {spread:6.3f} "
              f"{tbs:7.3f} {self.n * self.C / (best * 1e-3) / 1e9:8.2f}", flush=True)
        return best


HEAD = (f"{'C':>6s} {'L':>3s} {'n':>9s} {'input':>5s} {'noise':>5s} {'links':>5s} {'rows':>4s} {'':>4s} {'LDS':>7s} {'ms':>9s} "
        f"{'spread':>6s} {'TB/s':>7s} {'Gsmp/s':>8s}")
print(f"# ms is the fastest of {ROUNDS} rounds of {ITERS} calls, spread the slowest over it; TB/s is algorithmic (16 B per "
      f"output pitched, 8 B broadcast)")
print("# part 1: every shape at the planner's arrangement")
print(HEAD)
fused = {}
for total in TOTALS:
    for C in BANKS:
        for L in TAPS:
            for bcast in (False, True):
                for noise in (True, False):
                    s = Shape(C, L, total, bcast, noise)
                    fused[(C, L, total, bcast, noise)] = s.row()
                    del s

print("# part 2: the arrangements, pitched input, the larger total")
print(HEAD)
for C in BANKS:
    for L in TAPS:
        for noise in (True, False):
            s = Shape(C, L, TOTALS[-1], False, noise)
            for links in LINKS:
                for rows in ROWS:
                    s.row(links, rows)
            del s

print("# part 3: channels = 1, the composed route (FirFilter cccf, Osc.mix_block_up, scale, gen_complex_dev, add) on the "
      "same build; ratio = composed / fused")
print(f"{'L':>3s} {'n':>9s} {'noise':>5s} {'composed ms':>11s} {'spread':>6s} {'fused ms':>9s} {'ratio':>6s}")
for total in TOTALS:
    for L in TAPS:
        for noise in (True, False):
            n = total
            fir, osc = ya.FirFilter("cccf", taps(L, 0)), ya.Osc(ya.OscScheme.Nco)
            fir.set_stream(st.cuda_stream), osc.set_stream(st.cuda_stream)
            osc.set_frequency(0.0123)
            x = torch.randn(n, dtype=torch.complex64, device=dev)
            a, b, g = (torch.empty(n, dtype=torch.complex64, device=dev) for _ in range(3))
            gamma, nstd = ya.channel_awgn_words(-20.0, 10.0)
            pos = [0]

            def composed():
                fir.execute_block_dev(x, n, a)
                osc.mix_block_up_dev(a, n, b)
                if noise:
                    ya.gen_complex_dev(1, n, out=g, first=pos[0], stream=st.cuda_stream)
                    pos[0] += n
                    torch.mul(b, float(gamma), out=b)
                    torch.add(b, g, alpha=float(nstd), out=a)
                else:
                    torch.mul(b, float(gamma), out=a)

            best, spread = timed(composed)
            f = fused[(1, L, total, False, noise)]
            print(f"{L:3d} {n:9d} {'on' if noise else 'off':>5s} {best:11.4f} {spread:6.3f} {f:9.4f} {best / f:6.2f}", flush=True)
            del x, a, b, g
