#!/usr/bin/env python3
"""SymStream block form (GPU box): fused write_samples_devptr beside the three-object composition on device buffers --
MSequence.generate_symbols_block_devptr, Modem.modulate_block_devptr, x gain on the float32 view (one torch kernel),
FirInterpolationFilter("crcf").execute_block_dev -- for k in {2, 4, 8}, m in {7, 12}, Qpsk and Qam64, Arkaiser at
beta 0.3, one call of 2^22 symbols.  The two forms write the same words (tests/test_gpu_symstream.py); here they are
timed.  Three rounds, the forms alternating inside each; a round is HIP events around ITERS calls after WARM warm-up
calls; the table gives the fastest round and the slowest / fastest spread.
GB/s is algorithmic bytes over time.  Fused: the 8 B per output sample it writes, nothing read.  Composition: per
symbol 1 B written and read (symbols), 8 B written, read, written and read again (points, gain in place) and 8 k B of
samples written = 34 + 8 k B.  Modem.modulate_block_devptr reads its range flag back, so the composition's time
includes that host round trip per call, as a user of the three objects pays it.
Usage: python tools/kb_symstream.py"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
ROUNDS, WARM, ITERS = 3, 3, 10
NSYM = 1 << 22
GEN = (23, 4325376)
GAIN = 0.5


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


sym = torch.empty(NSYM, dtype=torch.uint8, device=dev)
pts = torch.empty(NSYM, dtype=torch.complex64, device=dev)
ptsf = torch.view_as_real(pts)
y = torch.empty(NSYM * 8, dtype=torch.complex64, device=dev)

print(f"# one call of {NSYM} symbols; ms is the fastest of {ROUNDS} rounds, spread the slowest over it")
print(f"{'scheme':>6s} {'k':>3s} {'m':>3s} {'fused':>6s} {'ms':>9s} {'spread':>7s} {'Msmp/s':>9s} {'GB/s':>7s} "
      f"{'comp ms':>9s} {'spread':>7s} {'comp GB/s':>10s} {'fused/comp':>11s}")
for scheme in (ya.ModulationScheme.Qpsk, ya.ModulationScheme.Qam64):
    for k in (2, 4, 8):
        for m in (7, 12):
            src = ya.MSequence(*GEN)
            src.set_stream(st.cuda_stream)
            q = ya.SymStream(ya.FirFilterShape.Arkaiser, k, m, 0.3, scheme, src)
            q.set_stream(st.cuda_stream)
            q.set_gain(GAIN)
            mod = ya.Modem(scheme)
            mod.set_stream(st.cuda_stream)
            fir = ya.FirInterpolationFilter.new_prototype("crcf", ya.FirFilterShape.Arkaiser, k, m, 0.3)
            fir.set_stream(st.cuda_stream)
            bps = mod.get_bps()
            n = NSYM * k

            def fused():
                q.write_samples_devptr(y, n)

            def comp():
                src.generate_symbols_block_devptr(bps, NSYM, sym)
                mod.modulate_block_devptr(sym, NSYM, pts)
                ptsf.mul_(GAIN)
                fir.execute_block_dev(pts, NSYM, y)

            tf, tc = [], []
            for _ in range(ROUNDS):
                tf.append(timed(fused))
                tc.append(timed(comp))
            a, b = min(tf), min(tc)
            print(f"{scheme.name:>6s} {k:3d} {m:3d} {'yes' if q.is_fused() else 'no':>6s} {a:9.4f} {max(tf) / a:7.3f} "
                  f"{n / a / 1e3:9.1f} {8 * n / a / 1e6:7.1f} {b:9.4f} {max(tc) / b:7.3f} "
                  f"{NSYM * (34 + 8 * k) / b / 1e6:10.1f} {a / b:11.4f}", flush=True)
            del q, mod, fir, src
