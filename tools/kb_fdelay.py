#!/usr/bin/env python3
"""Fdelay block and track forms (GPU box): execute_block_dev and execute_track_dev of the three kinds at the default
shape (nmax 200, m 8, npfb 64: 16 taps per output) on 2^20, 2^24 and 2^26 samples, beside what a caller could do before
the object existed: FirPfbFilter.execute_block_dev(i, ...) on a buffer shifted by the whole-sample lag (right only while
the delay never changes).  Three rounds, the fused and the composed call alternating inside each; every round is HIP
events around 20 calls after 10 warm-up calls; the table gives the fastest round and the slowest / fastest spread.
Rates are algorithmic bytes over time: a sample in and a sample out, plus 4 B of delay per sample for the track form.
Given the output of tools/kb_stream_probe (run in the same session), each row is also read against the better of the
plain and nt probe rows of its read : write mix (block 1 : 1; track rrrf 2 : 1; track crcf / cccf 3 : 2, read against
the higher of the 1 : 1 and 2 : 1 rows).  cccf spends 8 unfused flop per byte at 16 taps; its GFLOP/s column says how
close that form is to the vector rate.
Usage: python tools/kb_fdelay.py [stream_probe_output.txt]"""
import re
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
NMAX, M, NPFB = 200, 8, 64
DELAY = 17.3                                   # lag 18 whole samples, branch 45
ROUNDS = 3

probe = {}
if len(sys.argv) > 1:
    for line in Path(sys.argv[1]).read_text().splitlines():
        mt = re.match(r"read (\d) : write (\d)\b.*?([\d.]+) TB/s", line)
        if mt:
            k = (int(mt.group(1)), int(mt.group(2)))
            probe[k] = max(probe.get(k, 0.0), float(mt.group(3)))


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


def ceiling(form, kind):
    if form == "block":
        return probe.get((1, 1))
    if kind == "rrrf":
        return probe.get((2, 1))
    both = [probe[k] for k in ((1, 1), (2, 1)) if k in probe]
    return max(both) if both else None


print(f"# probe ceilings (TB/s, better of plain / nt): {probe}")
print(f"{'form':6s} {'kind':5s} {'n':>9s} {'ms':>9s} {'spread':>7s} {'Gsmp/s':>8s} {'TB/s':>6s} {'of probe':>9s} "
      f"{'GFLOP/s':>9s} {'composed ms':>12s} {'spread':>7s} {'fused/composed':>15s}")
verdict = []
for lg in (20, 24, 26):
    n = 1 << lg
    for kind in ("rrrf", "crcf", "cccf"):
        cplx = kind != "rrrf"
        esz = 8 if cplx else 4
        lead = 256                                            # samples in front of x for the shifted composed read
        buf = torch.randn((n + lead) * (2 if cplx else 1), dtype=torch.float32, device=dev)
        y = torch.empty(n * (2 if cplx else 1), dtype=torch.float32, device=dev)
        x_ptr = buf.data_ptr() + lead * esz
        track = torch.linspace(0, NMAX, n, dtype=torch.float32, device=dev)     # a ramp over the whole range
        q = ya.Fdelay(kind, NMAX, M, NPFB)
        q.set_stream(st.cuda_stream)
        q.set_delay(DELAY)
        bank = ya.FirPfbFilter.default(kind, NPFB, M)
        bank.set_stream(st.cuda_stream)
        lag, branch = 18, 45                                  # what set_delay(17.3) selects: w = 182, f = 45
        forms = {"block": lambda: q.execute_block_dev(x_ptr, n, y),
                 "track": lambda: q.execute_track_dev(track, x_ptr, n, y),
                 "composed": lambda: bank.execute_block_dev(branch, x_ptr - lag * esz, n, y)}
        ms = {k: [] for k in forms}
        for _ in range(ROUNDS):
            for k, fn in forms.items():
                ms[k].append(timed(fn))
        comp = min(ms["composed"])
        for form in ("block", "track"):
            t = min(ms[form])
            nbytes = (2 * esz + (4 if form == "track" else 0)) * n
            tbs = nbytes / t / 1e9
            ceil = ceiling(form, kind)
            frac = tbs / ceil if ceil else float("nan")
            flop = (2 if kind == "rrrf" else 4 if kind == "crcf" else 8) * 2 * M * n
            print(f"{form:6s} {kind:5s} {n:9d} {t:9.4f} {max(ms[form]) / t:7.3f} {n / t / 1e6:8.1f} {tbs:6.2f} {frac:9.3f} "
                  f"{flop / t / 1e6:9.0f} {comp:12.4f} {max(ms['composed']) / comp:7.3f} {t / comp:15.3f}", flush=True)
            if form == "block" and lg == 26:
                verdict.append(f"{kind}: fused {t:.4f} ms vs composed {comp:.4f} ms = {t / comp:.3f}")
        del buf, y, track, q, bank
print("# fixed-delay block form against the composed parent path (2^26 samples): " + "; ".join(verdict))
