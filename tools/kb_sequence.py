#!/usr/bin/env python3
"""MSequence and BSequence block forms (GPU box).
Generator: generate_bits_block_devptr and generate_symbols_block_devptr(bps in {2, 8}) on 2^26 symbols for m in {8, 31},
in Gsym/s, Gbit/s and TB/s (one byte written per symbol), read against the write-only row of tools/kb_stream_probe.
Correlator: push_correlate_block_devptr on 2^24 symbols for N in {63, 255, 1023, 8191} and bps in {1, 2, 8}, in
Gout/s and TB/s (1 byte read, 4 written per output), read against the 1 : 4 probe row, and in Gwordop/s: the W = ceil(N /
32) window words an output visits, each one LDS read, one funnel shift, one xor and one bit count.
Three rounds; a round is HIP events around ITERS calls after WARM warm-up calls; the table gives the fastest round and
the slowest / fastest spread.
Usage: python tools/kb_sequence.py [stream_probe_output.txt]"""
import re
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
ROUNDS = 3

probe_w, probe_14 = 0.0, 0.0
if len(sys.argv) > 1:
    for line in Path(sys.argv[1]).read_text().splitlines():
        mt = re.match(r"write only\b.*?([\d.]+) TB/s", line)
        if mt:
            probe_w = max(probe_w, float(mt.group(1)))
        mt = re.match(r"read 1 : write 4\b.*?([\d.]+) TB/s", line)
        if mt:
            probe_14 = max(probe_14, float(mt.group(1)))


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


def best(fn, warm, iters):
    ms = [timed(fn, warm, iters) for _ in range(ROUNDS)]
    return min(ms), max(ms) / min(ms)


GEN = {2: 0x3, 8: 0xB8, 31: 0x40000004}
print(f"# write-only probe ceiling (TB/s, better of plain / nt): {probe_w or 'not given'}")
print(f"{'m':>3s} {'form':>6s} {'symbols':>9s} {'ms':>9s} {'spread':>7s} {'Gsym/s':>8s} {'Gbit/s':>8s} {'TB/s':>6s} {'of probe':>9s}")
N = 1 << 26
y = torch.empty(N + 16, dtype=torch.uint8, device=dev)
for m in (8, 31):
    for form, bps in (("bits", 1), ("sym", 2), ("sym", 8)):
        q = ya.MSequence(m, GEN[m])
        q.set_stream(st.cuda_stream)
        fn = (lambda: q.generate_bits_block_devptr(N, y)) if form == "bits" else (lambda: q.generate_symbols_block_devptr(bps, N, y))
        t, sp = best(fn, 5, 20)
        tbs = N / t / 1e9
        print(f"{m:3d} {form + str(bps):>6s} {N:9d} {t:9.4f} {sp:7.3f} {N / t / 1e6:8.2f} {N * bps / t / 1e6:8.2f} {tbs:6.2f} "
              f"{tbs / probe_w if probe_w else float('nan'):9.3f}", flush=True)
        del q
# the same at an output that is not 16-byte aligned: the byte-store path of the kernel
q = ya.MSequence(31, GEN[31])
q.set_stream(st.cuda_stream)
t, sp = best(lambda: q.generate_bits_block_devptr(N, y.data_ptr() + 1), 5, 20)
print(f"{31:3d} {'bits1':>6s} {N:9d} {t:9.4f} {sp:7.3f} {N / t / 1e6:8.2f} {N / t / 1e6:8.2f} {N / t / 1e9:6.2f} "
      f"{N / t / 1e9 / probe_w if probe_w else float('nan'):9.3f}   (y + 1: unaligned)", flush=True)
del q, y

print(f"# 1 : 4 probe ceiling (TB/s, better of plain / nt): {probe_14 or 'not given'}")
print(f"{'N':>5s} {'bps':>4s} {'symbols':>9s} {'ms':>9s} {'spread':>7s} {'Gout/s':>8s} {'TB/s':>6s} {'of probe':>9s} {'Gwordop/s':>10s}")
n = 1 << 24
sym = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev)
rxy = torch.empty(n, dtype=torch.int32, device=dev)
for Nb in (63, 255, 1023, 8191):
    ref = ya.BSequence(Nb)
    ref.init((np.arange(1024) * 37 % 251).astype(np.uint8))
    W = (Nb + 31) // 32
    for bps in (1, 2, 8):
        q = ya.BSequence(Nb)
        q.set_stream(st.cuda_stream)
        heavy = Nb >= 1023
        t, sp = best(lambda: q.push_correlate_block_devptr(ref, sym, n, bps, rxy), 3 if heavy else 10, 5 if heavy else 20)
        tbs = 5 * n / t / 1e9
        print(f"{Nb:5d} {bps:4d} {n:9d} {t:9.4f} {sp:7.3f} {n / t / 1e6:8.2f} {tbs:6.2f} "
              f"{tbs / probe_14 if probe_14 else float('nan'):9.3f} {W * n / t / 1e6:10.1f}", flush=True)
        del q
