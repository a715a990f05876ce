#!/usr/bin/env python3
"""Modem block forms (GPU box): modulate_block_dev, demodulate_block_dev and demodulate_soft_block_dev per scheme on 2^24
symbols, in symbols/s and algorithmic bytes/s (modulate 1 B in, 8 out; hard demodulate 8 in, 1 out; soft 8 in, 1 + bps
out).  Three rounds of HIP events around 20 calls after 10 warm-up calls; the fastest round and the slowest / fastest
spread.  Given the output of tools/kb_stream_probe (run in the same session) each row is also read against the probe's
row of the same read : write mix (1 : 8 modulate, 8 : 1 hard, 8 : 1 + bps soft; the nearest row where the probe output
given has no such row).  Arb-256 soft is bound by arithmetic: its VALU estimate is printed beside it.
Usage: python tools/kb_modem.py [stream_probe_output.txt]"""
import re
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

st = torch.cuda.current_stream()
N = 1 << 24
ROUNDS = 3
SCHEMES = ["Bpsk", "Qpsk", "Ook", "Ask4", "Ask256", "Qam16", "Qam64", "Qam256", "Psk8", "Psk256", "Dpsk8", "Dpsk256",
           "Arb16", "Arb256"]

probe = {}
if len(sys.argv) > 1:
    for line in Path(sys.argv[1]).read_text().splitlines():
        mt = re.match(r"read (\d) : write (\d)\b.*?([\d.]+) TB/s", line)
        if mt:
            k = (int(mt.group(1)), int(mt.group(2)))
            probe[k] = max(probe.get(k, 0.0), float(mt.group(3)))


def nearest(rd, wr):
    if not probe:
        return None
    if (rd, wr) in probe:
        return (rd, wr), probe[(rd, wr)]
    want = rd / (rd + wr)
    k = min(probe, key=lambda q: abs(q[0] / (q[0] + q[1]) - want))
    return k, probe[k]


def timed(fn):
    best, worst = 1e30, 0.0
    for _ in range(ROUNDS):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(20):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) / 20
        best, worst = min(best, t), max(worst, t)
    return best, worst / best


def make(name):
    if name.startswith("Arb"):
        M = int(name[3:])
        rng = np.random.default_rng(M)
        return ya.Modem.from_table((rng.standard_normal(M) + 1j * rng.standard_normal(M)).astype(np.complex64))
    return ya.Modem(ya.ModulationScheme[name])


print(f"# probe rows (TB/s, better of plain / nt): {probe}")
print(f"{'scheme':8s} {'form':9s} {'ms':>8s} {'spread':>7s} {'Gsym/s':>8s} {'TB/s':>7s} {'probe row':>10s} {'of probe':>9s}")
for name in SCHEMES:
    m = make(name)
    m.set_stream(st.cuda_stream)
    bps, M = m.get_bps(), m.get_constellation_size()
    sym = torch.randint(0, M, (N,), dtype=torch.uint8, device="cuda")
    x = torch.empty(N, dtype=torch.complex64, device="cuda")
    xh = torch.empty(N, dtype=torch.complex64, device="cuda")
    out = torch.empty(N, dtype=torch.uint8, device="cuda")
    soft = torch.empty(N * bps, dtype=torch.uint8, device="cuda")
    m.modulate_block_devptr(sym, N, x)
    x += 0.1 * torch.randn(N, dtype=torch.complex64, device="cuda")
    forms = [("modulate", lambda: m.modulate_block_devptr(sym, N, xh), 1, 8),
             ("hard", lambda: m.demodulate_block_devptr(x, N, out), 8, 1),
             ("soft", lambda: m.demodulate_soft_block_devptr(x, N, out, soft), 8, 1 + bps)]
    for form, fn, rd, wr in forms:
        ms, spread = timed(fn)
        tbs = N * (rd + wr) / (ms * 1e-3) / 1e12
        near = nearest(rd, wr)
        tail = f"{near[0][0]} : {near[0][1]:<6d} {tbs / near[1]:9.2f}" if near else f"{'-':>10s} {'-':>9s}"
        print(f"{name:8s} {form:9s} {ms:8.3f} {spread:7.2f} {N / (ms * 1e-3) / 1e9:8.2f} {tbs:7.3f} {tail}")
    if name == "Arb256":
        # per candidate point and sample: 2 sub, 2 mul, 1 add, compare + 2 selects, and per bit a bit test, two compares
        # and four selects (about 7): 8 + 7 * 8 = 64 lane-operations, 256 candidates per sample; the device issues
        # 256 CUs x 4 SIMDs x 16 lanes per clock at 2.4 GHz
        ops = 256 * (8 + 7 * bps)
        print(f"# Arb256 soft: VALU estimate {ops} lane-ops per sample -> {256 * 64 * 2.4e9 / ops / 1e9:.2f} Gsym/s at full issue rate")
