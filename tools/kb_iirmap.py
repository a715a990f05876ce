#!/usr/bin/env python3
"""IirDecimationFilter, IirInterpolationFilter and IirHilbertFilter block calls (GPU box): for each mode the fused
execute_block_dev and, in the same process, the composed path a caller had before -- zero-stuff or sign-map into a
temporary with torch ops, IirFilter.execute_block_dev over the virtual stream, a strided copy out.  The two are
alternated call by call (10 warm-up rounds, 40 timed rounds, HIP events around every call); the table gives the median,
the interquartile range and the full range (max - min) of each in microseconds and the fused / composed ratio of the
medians.
Cases: 2^20 and 2^24 filter steps; crcf with 4 sections at M = 2 and 8; the four Hilbert modes at order 5.
Usage: python tools/kb_iirmap.py
       python tools/kb_iirmap.py trace MODE LG    50 fused Hilbert calls of one mode at 2^LG steps and nothing else,
                                                  to run under `rocprofv3 --kernel-trace --stats`"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def ab(fused, composed):
    tf, tc = [], []
    for r in range(50):
        a, b = once(fused), once(composed)
        if r >= 10:
            tf.append(a)
            tc.append(b)
    return np.array(tf), np.array(tc)


def report(case, steps, tf, tc, tmp_bytes):
    iqr = lambda t: np.percentile(t, 75) - np.percentile(t, 25)
    print(f"{case:22s} {steps:9d} {np.median(tf):10.1f} {iqr(tf):6.1f} {tf.max() - tf.min():7.1f} {np.median(tc):10.1f} "
          f"{iqr(tc):6.1f} {tc.max() - tc.min():7.1f} {np.median(tf) / np.median(tc):7.3f} {tmp_bytes / 2**20:12.1f}")


SB = np.tile([0.1, 0.2, 0.1], 4).astype(np.float32)
SA = np.tile([1.0, -1.2, 0.5], 4).astype(np.float32)
HB, HA = ya.iir_design_lowpass_sos(ya.IirFilterShape.Butter, 5, 0.25)
SGN_R = torch.tensor([1, -1j, -1, 1j], dtype=torch.complex64, device=dev)     # r2c / decim input map: x -> u
ROT = torch.tensor([1, 1j, -1, -1j], dtype=torch.complex64, device=dev)       # r2c output map: v -> y / 2

if sys.argv[1:2] == ["trace"]:
    mode, N = sys.argv[2], 1 << int(sys.argv[3])
    h = ya.IirHilbertFilter.new_default(5)
    h.set_stream(st.cuda_stream)
    real_in, real_out, per = mode in ("r2c", "decim"), mode in ("c2r", "interp"), 2 if mode in ("decim", "interp") else 1
    x = torch.randn(N, dtype=torch.float32 if real_in else torch.complex64, device=dev)
    y = torch.empty(N, dtype=torch.float32 if real_out else torch.complex64, device=dev)
    for _ in range(50):
        getattr(h, mode + "_execute_block_dev")(x, N // per, y)
    torch.cuda.synchronize()
    sys.exit(0)

print(f"{'case':22s} {'steps':>9s} {'fused us':>10s} {'iqr':>6s} {'range':>7s} {'composed':>10s} {'iqr':>6s} {'range':>7s} {'ratio':>7s} {'composed MiB':>12s}")
for lg in (20, 24):
    N = 1 << lg
    for M in (2, 8):
        n = N // M
        # decim
        q, f = ya.IirDecimationFilter.new_sos("crcf", M, SB, SA, 4), ya.IirFilter.new_sos("crcf", SB, SA, 4)
        q.set_stream(st.cuda_stream); f.set_stream(st.cuda_stream)
        x = torch.randn(N, dtype=torch.complex64, device=dev)
        y, t = torch.empty(n, dtype=torch.complex64, device=dev), torch.empty(N, dtype=torch.complex64, device=dev)

        def comp_decim():
            f.execute_block_dev(x, N, t)
            y.copy_(t[::M])
        tf, tc = ab(lambda: q.execute_block_dev(x, n, y), comp_decim)
        report(f"decim crcf sos4 M={M}", N, tf, tc, t.numel() * 8)
        # interp
        q = ya.IirInterpolationFilter.new_sos("crcf", M, SB, SA, 4)
        q.set_stream(st.cuda_stream)
        xi, yi = x[:n].contiguous(), torch.empty(N, dtype=torch.complex64, device=dev)

        def comp_interp():
            t.zero_()
            t[::M] = xi
            f.execute_block_dev(t, N, yi)
        tf, tc = ab(lambda: q.execute_block_dev(xi, n, yi), comp_interp)
        report(f"interp crcf sos4 M={M}", N, tf, tc, t.numel() * 8)
        del x, y, t, xi, yi
    # Hilbert, order 5 (3 sections)
    h, f = ya.IirHilbertFilter.new_default(5), ya.IirFilter.new_sos("crcf", HB, HA, 3)
    h.set_stream(st.cuda_stream); f.set_stream(st.cuda_stream)
    xr, xc = torch.randn(N, dtype=torch.float32, device=dev), torch.randn(N, dtype=torch.complex64, device=dev)
    u, v = torch.empty(N, dtype=torch.complex64, device=dev), torch.empty(N, dtype=torch.complex64, device=dev)
    yc, yr = torch.empty(N, dtype=torch.complex64, device=dev), torch.empty(N, dtype=torch.float32, device=dev)
    sg, rt = SGN_R.repeat(N // 4), ROT.repeat(N // 4)

    def comp_r2c():
        torch.mul(xr, sg, out=u)
        f.execute_block_dev(u, N, v)
        torch.mul(v, rt, out=yc)
        yc.mul_(2.0)

    def comp_c2r():
        torch.mul(xc, rt.conj(), out=u)
        f.execute_block_dev(u, N, v)
        v.mul_(rt)
        yr.copy_(v.real)

    def comp_decim():
        torch.mul(xr, sg, out=u)
        f.execute_block_dev(u, N, v)
        torch.mul(v[::2], 2.0, out=yc[:N // 2])

    def comp_interp():
        u.zero_()
        u[::2] = xc[:N // 2]
        f.execute_block_dev(u, N, v)
        v.mul_(rt)
        torch.mul(v.real, 2.0, out=yr)

    for name, fused, comp in (("r2c", lambda: h.r2c_execute_block_dev(xr, N, yc), comp_r2c),
                              ("c2r", lambda: h.c2r_execute_block_dev(xc, N, yr), comp_c2r),
                              ("decim", lambda: h.decim_execute_block_dev(xr, N // 2, yc), comp_decim),
                              ("interp", lambda: h.interp_execute_block_dev(xc, N // 2, yr), comp_interp)):
        h.reset()
        tf, tc = ab(fused, comp)
        report(f"hilbert {name} order 5", N, tf, tc, (u.numel() + v.numel() + sg.numel()) * 8)
    del xr, xc, u, v, yc, yr, sg, rt
