#!/usr/bin/env python3
"""OrdFilt block form (GPU box): execute_block_devptr at the median rank for n in {3, 5, 9, 33, 129, 1025} on 2^20, 2^24
and 2^26 samples, beside what a caller could do before the object existed:
`x.unfold(0, n, 1).kthvalue(k + 1, dim=1).values` in torch on the same device, on the whole block where its n-fold
intermediate fits TORCH_BYTES and on a shorter block otherwise (its time is then scaled to the row's length, marked *).
Three rounds, the fused and the composed call alternating inside each; a round is HIP events around ITERS calls after
WARM warm-up calls; the table gives the fastest round and the slowest / fastest spread.
TB/s is algorithmic bytes over time: 4 B in, 4 B out per sample.  Given the output of tools/kb_stream_probe (run in the
same session), it is also read against the better of the plain and nt 1 : 1 probe rows.  Gcmp/s is the kernel's own
work, 3 n (T + n - 1) / T compare-accumulates per output (n - 1 for a candidate's first rank, 2 per window it walks,
over the T + n - 1 candidates a tile of T outputs has), to be read against the integer vector rate.
Where the register-resident kernel form exists (n <= ORDFILT_REG_NMAX) the row is measured with each form forced
(set_kernel), in the same alternation: the first columns are the form named under "form", "other ms" is the LDS form.
Usage: python tools/kb_ordfilt.py [stream_probe_output.txt]"""
import re
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
ROUNDS = 3
TORCH_BYTES = 1 << 30
T = ya.ORDFILT_TILE

probe = 0.0
if len(sys.argv) > 1:
    for line in Path(sys.argv[1]).read_text().splitlines():
        mt = re.match(r"read 1 : write 1\b.*?([\d.]+) TB/s", line)
        if mt:
            probe = max(probe, float(mt.group(1)))


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


print(f"# 1 : 1 probe ceiling (TB/s, better of plain / nt): {probe or 'not given'}")
print(f"{'n':>5s} {'samples':>9s} {'ms':>9s} {'spread':>7s} {'Gsmp/s':>8s} {'TB/s':>6s} {'of probe':>9s} {'Gcmp/s':>9s} "
      f"{'torch ms':>10s} {'spread':>7s} {'fused/torch':>12s} {'form':>5s} {'other ms':>9s} {'spread':>7s}")
for lg in (20, 24, 26):
    N = 1 << lg
    x = torch.randn(N, dtype=torch.float32, device=dev)
    y = torch.empty(N, dtype=torch.float32, device=dev)
    for n in (3, 5, 9, 33, 129, 1025):
        k = n // 2
        q = ya.OrdFilt(n, k)
        q.set_stream(st.cuda_stream)
        nt = min(N, max(n, TORCH_BYTES // (4 * n)))               # samples of the composed call
        xt = x[:nt]
        heavy = n >= 129 and lg >= 24
        fused = lambda: q.execute_block_devptr(x, N, y)
        composed = lambda: xt.unfold(0, n, 1).kthvalue(k + 1, dim=1).values
        two = 2 <= n <= ya.ORDFILT_REG_NMAX
        if two:
            qo = ya.OrdFilt(n, k)
            qo.set_stream(st.cuda_stream)
            q.set_kernel(2)                                       # first columns: the register form; "other": the LDS form
            qo.set_kernel(1)
        other = lambda: qo.execute_block_devptr(x, N, y)
        ms = {"fused": [], "torch": [], "other": []}
        for _ in range(ROUNDS):
            ms["fused"].append(timed(fused, 3 if heavy else 10, 5 if heavy else 20))
            if two:
                ms["other"].append(timed(other, 10, 20))
            ms["torch"].append(timed(composed, 2, 4) * (N / (nt - n + 1)))
        t, tt = min(ms["fused"]), min(ms["torch"])
        tbs = 8 * N / t / 1e9
        cmp_per_out = 3 * n * (T + n - 1) / T
        print(f"{n:5d} {N:9d} {t:9.4f} {max(ms['fused']) / t:7.3f} {N / t / 1e6:8.2f} {tbs:6.2f} "
              f"{tbs / probe if probe else float('nan'):9.3f} {cmp_per_out * N / t / 1e6:9.0f} "
              f"{tt:9.3f}{'*' if nt < N else ' '} {max(ms['torch']) / tt:7.3f} {t / tt:12.4f} "
              + (f"{'reg':>5s} {min(ms['other']):9.4f} {max(ms['other']) / min(ms['other']):7.3f}" if two else f"{'lds':>5s}"),
              flush=True)
        del q
    del x, y
