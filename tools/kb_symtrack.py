#!/usr/bin/env python3
"""SymTrack block form (GPU box): execute_devptr at C = 64, 1024 and 16384 channels, k = 2, m = 7, npfb = 16, eq_len = 9,
QPSK, constant-modulus equalizer, in millions of channel-symbols per second.  The input is QPSK at two samples per symbol
through a three-tap pulse (the symbol, then the mean of it and the next one), a different carrier offset per channel and
a little noise: the loops lock on it, so a sample gives one synchroniser output and every other output a symbol, as in
service.
Beside it, the summed time of the five standalone block calls at the same shape: Agc.execute_block, SymSync.execute at
k_out = 2, one Osc.mix_block_down over the plane, EqLms.decim_block(2, BLIND) and Modem.demodulate_block.  They cannot
replace SymTrack (no carrier loop, the equalizer decides on a rotating sample); they do the same arithmetic open loop
with four intermediate planes through HBM.  The ratio is a record, not a pass condition.
Three rounds; a round is HIP events around ITERS calls after WARM warm-up calls (the state is carried from call to call,
as in a stream); the table gives the fastest round and the slowest / fastest spread.
Usage: python tools/kb_symtrack.py"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
ROUNDS, WARM, ITERS = 3, 1, 3
K, M, NPFB, EQ_LEN, BETA = 2, 7, 16, 9, 0.3
FT = ya.FirFilterShape.Arkaiser


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


def fastest(fn):
    t = [timed(fn, WARM, ITERS) for _ in range(ROUNDS)]
    return min(t), max(t) / min(t)


def stimulus(C, nsym):
    g = torch.Generator(device=dev).manual_seed(24)
    bits = torch.randint(0, 4, (nsym + 1, C), device=dev, generator=g)
    s = (((bits & 1) * -2 + 1) + 1j * ((bits >> 1) * -2 + 1)).to(torch.complex64) * (0.5 ** 0.5)
    x = torch.empty(2 * nsym, C, dtype=torch.complex64, device=dev)
    x[0::2] = s[:-1]
    x[1::2] = 0.5 * (s[:-1] + s[1:])
    f = 0.02 * ((torch.arange(C, device=dev) % 9) - 4) / 4.0
    rot = torch.exp(1j * (torch.arange(2 * nsym, device=dev)[:, None] * f[None, :]))
    noise = torch.randn(2 * nsym, C, dtype=torch.complex64, device=dev, generator=g) * 0.03
    return (0.3 * x * rot + noise).contiguous()


def row(C, nsym):
    n = nsym * K
    x = stimulus(C, nsym)
    ycap = nsym + 64
    q = ya.SymTrack(C, FT, K, M, BETA, ya.ModulationScheme.Qpsk, ya.OscScheme.Nco, NPFB, EQ_LEN)
    q.set_stream(st.cuda_stream)
    y = torch.empty(ycap * C, dtype=torch.complex64, device=dev)
    sym = torch.empty(ycap * C, dtype=torch.uint8, device=dev)
    status = torch.zeros(3 * C, dtype=torch.int32, device=dev)
    fused, spread = fastest(lambda: q.execute_devptr(x, C, n, y, C, sym, C, ycap, status))
    torch.cuda.synchronize()
    ny = status[:C].cpu().numpy()
    stalled = int((status[C:2 * C] != 0).sum())

    agc = ya.Agc(C)
    agc.set_bandwidth(0.018)
    ss = ya.SymSync.rnyquist(C, FT, K, M, BETA, NPFB)
    ss.set_output_rate(2)
    ss.set_lf_bw(0.0009)
    osc = ya.Osc(ya.OscScheme.Nco)
    osc.set_frequency(0.01)
    eq = ya.EqLms.lowpass(C, EQ_LEN, 0.45)
    eq.set_bw(0.018)
    modem = ya.Modem(ya.ModulationScheme.Qpsk)
    for o in (agc, ss, osc, eq, modem):
        o.set_stream(st.cuda_stream)
    cap2 = n + 128
    v = torch.empty(n * C, dtype=torch.complex64, device=dev)
    s2 = torch.zeros(cap2 * C, dtype=torch.complex64, device=dev)
    u = torch.empty(cap2 * C, dtype=torch.complex64, device=dev)
    d = torch.empty(cap2 * C, dtype=torch.complex64, device=dev)
    sy = torch.empty(cap2 * C, dtype=torch.uint8, device=dev)
    st2 = torch.zeros(2 * C, dtype=torch.int32, device=dev)
    parts = [fastest(lambda: agc.execute_block_devptr(x, C, n, v, C))[0],
             fastest(lambda: ss.execute_devptr(v, C, n, s2, C, cap2, st2))[0],
             fastest(lambda: osc.mix_block_down_dev(s2, n * C, u))[0],
             fastest(lambda: eq.decim_block_devptr(2, ya.EqLmsUpdate.BLIND, u, C, n, None, C, d, C))[0],
             fastest(lambda: modem.demodulate_block_devptr(d, nsym * C, sy))[0]]
    total = sum(parts)
    rate = float(ny.sum()) / (fused * 1e-3)
    print(f"{C:6d} {nsym:6d} {fused:9.3f} {spread:7.3f} {rate / 1e6:10.1f} {ny.min():6d} {ny.max():6d} {stalled:7d} | "
          + " ".join(f"{p:8.3f}" for p in parts) + f" {total:9.3f} {fused / total:7.3f}", flush=True)


print(f"# SymTrack.execute_devptr, k = {K}, m = {M}, npfb = {NPFB}, eq_len = {EQ_LEN}, QPSK, CM; ms is the fastest of "
      f"{ROUNDS} rounds of {ITERS} calls, spread the slowest over it; Msym/s counts channel-symbols of the fused call; "
      f"parts: Agc, SymSync, Osc, EqLms, Modem and their sum in ms; ratio = fused / sum")
print(f"{'C':>6s} {'nsym':>6s} {'fused ms':>9s} {'spread':>7s} {'Msym/s':>10s} {'ny min':>6s} {'ny max':>6s} {'stalled':>7s} | "
      f"{'agc':>8s} {'symsync':>8s} {'osc':>8s} {'eqlms':>8s} {'modem':>8s} {'sum':>9s} {'ratio':>7s}")
for C, nsym in ((64, 4096), (1024, 4096), (16384, 1024)):
    row(C, nsym)
