#!/usr/bin/env python3
"""SymStreamR block form (GPU box): write_samples_devptr beside the composition of the two objects on device buffers --
SymStream(k = 2).write_samples_devptr(need) into scratch, then MsResamp("crcf", 0.5 / bw).execute_dev -- for bw in
{0.9, 0.6, 0.4, 0.26, 0.2, 0.05, 0.001}, m in {7, 12}, Qpsk and Qam64, Arkaiser at beta 0.3, one call of 2^24 outputs
(the composition pushes the `need` of plan_symstreamr for that call from phase 0, which gives as many outputs or a few
more).  The two forms write the same words (tests/test_gpu_symstreamr.py); here they are timed.  Three rounds, the
forms alternating inside each; a round is HIP events around ITERS calls after WARM warm-up calls; the table gives the
fastest round and the slowest / fastest spread.
GB/s is 8 B per output sample over time: what the fused call writes at zero half-band stages, where it reads nothing.
Usage: python tools/kb_symstreamr.py [bw ...]      (other bandwidths than the list above)"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
ROUNDS, WARM, ITERS = 3, 2, 5
N = 1 << 24
GEN = (23, 4325376)
BWS = [float(a) for a in sys.argv[1:]] or [0.9, 0.6, 0.4, 0.26, 0.2, 0.05, 0.001]


def timed(fn):
    for _ in range(WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(ITERS):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


y = torch.empty(N + (1 << 12), dtype=torch.complex64, device=dev)
s = torch.empty(2 * N + (1 << 12), dtype=torch.complex64, device=dev)

print(f"# one call of {N} outputs; ms is the fastest of {ROUNDS} rounds, spread the slowest over it")
print(f"{'scheme':>6s} {'bw':>6s} {'m':>3s} {'stages':>6s} {'rate_arb':>9s} {'fused':>6s} {'ms':>9s} {'spread':>7s} "
      f"{'GB/s':>7s} {'comp ms':>9s} {'spread':>7s} {'comp GB/s':>10s} {'fused/comp':>11s}")
for scheme in (ya.ModulationScheme.Qpsk, ya.ModulationScheme.Qam64):
    for bw in BWS:
        for m in (7, 12):
            src = ya.MSequence(*GEN)
            src.set_stream(st.cuda_stream)
            q = ya.SymStreamR(ya.FirFilterShape.Arkaiser, bw, m, 0.3, scheme, src)
            q.set_stream(st.cuda_stream)
            sym = ya.SymStream(ya.FirFilterShape.Arkaiser, 2, m, 0.3, scheme, src)
            sym.set_stream(st.cuda_stream)
            rs = ya.MsResamp("crcf", np.float32(0.5) / np.float32(bw), 60.0)
            rs.set_stream(st.cuda_stream)
            plan = ya.plan_symstreamr(bw, m, N)
            need = plan.need

            def fused():
                q.write_samples_devptr(y, N)

            def comp():
                sym.write_samples_devptr(s, need)
                rs.execute_dev(s, need, y, y.numel())

            tf, tc = [], []
            for _ in range(ROUNDS):
                tf.append(timed(fused))
                tc.append(timed(comp))
            a, b = min(tf), min(tc)
            print(f"{scheme.name:>6s} {bw:6.3f} {m:3d} {plan.stages:6d} {float(plan.rate_arb):9.5f} "
                  f"{'yes' if q.is_fused() else 'no':>6s} {a:9.4f} {max(tf) / a:7.3f} {8 * N / a / 1e6:7.1f} "
                  f"{b:9.4f} {max(tc) / b:7.3f} {8 * N / b / 1e6:10.1f} {a / b:11.4f}", flush=True)
            del q, sym, rs, src
