#!/usr/bin/env python3
"""FirHilbertFilter block forms (GPU box): decim / interp / r2c / c2r *_execute_block_dev at m = 2, 12, 25, 64 on
2^20, 2^24 and 2^26 units (decim: outputs; the others: inputs).  HIP events around 20 calls after 10 warm-up calls.
Rates are algorithmic bytes over time: 16 B per unit (decim 8 in + 8 out, interp and c2r 8 + 8), r2c 12 B (4 + 8).
Given the output of tools/kb_stream_probe (run in the same session), each row is also read against the better of the
plain and nt probe rows at its read : write mix (1 : 1, r2c 1 : 2); the bar is 0.80 of it at m = 12 and 2^26 units.
Usage: python tools/kb_firhilb.py [stream_probe_output.txt]"""
import re
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
BAR = 0.80

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


# mode: (input floats per unit, output floats per unit, probe mix)
MODES = {"decim": (2, 2, (1, 1)), "interp": (2, 2, (1, 1)), "c2r": (2, 2, (1, 1)), "r2c": (1, 2, (1, 2))}
print(f"# probe ceilings (TB/s, better of plain / nt): {probe}")
print(f"{'mode':6s} {'m':>3s} {'n':>9s} {'ms':>9s} {'Gunit/s':>9s} {'TB/s':>7s} {'of 8TB/s':>9s} {'of probe':>9s}")
verdict = []
for lg in (20, 24, 26):
    n = 1 << lg
    for mode, (fi, fo, mix) in MODES.items():
        x = torch.randn(fi * n, dtype=torch.float32, device=dev)
        y = torch.empty(fo * n, dtype=torch.float32, device=dev)
        for m in (2, 12, 25, 64):
            q = ya.FirHilbertFilter(m, 60.0)
            q.set_stream(st.cuda_stream)
            fn = getattr(q, mode + "_execute_block_dev")
            ms = timed(lambda: fn(x, n, y))
            tbs = 4 * (fi + fo) * n / ms / 1e9
            frac = tbs / probe[mix] if mix in probe else float("nan")
            print(f"{mode:6s} {m:3d} {n:9d} {ms:9.4f} {n / ms / 1e6:9.1f} {tbs:7.2f} {tbs / 8:9.3f} {frac:9.3f}",
                  flush=True)
            if m == 12 and lg == 26:
                verdict.append(f"{mode}: {frac:.3f} of probe -> {'meets' if frac >= BAR else 'MISSES'} {BAR}")
        del x, y
print("# bar (m = 12, 2^26 units): " + "; ".join(verdict))
