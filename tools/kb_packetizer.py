#!/usr/bin/env python3
"""Packetizer block forms (GPU box) beside what they replace, modelled on tools/kb_convcode.py: v27, v29 and v27p34 at n in
{32, 128, 1024} payload bytes (where the code's limit allows) and F in {64, 4096, 65536} frames, CRC_32, C = floor(sqrt N)
columns, scrambler on, on random soft bytes (no codewords: every survivor decision is data dependent) and random payloads.
Per shape, on the same bank:
  fused    Packetizer.decode_block_devptr
  conv     ConvCode.decode_block_devptr over the same 8 (n + w) message bits (the kernel the fusion is built around)
  copy     one device-to-device copy of the soft plane: the floor of any separate deinterleave / descramble pass
  bar      fused must not exceed conv + copy by more than the larger of the spreads of the fused and the conv rows:
           ratio = fused / (conv + copy) against that spread; `ok` or `MISS`
  enc      Packetizer.encode_block_devptr (bps = 1) beside ConvCode.encode_block_devptr on the same bits, no bar
Three rounds; a round is HIP events around ITERS calls after WARM warm-up calls; ms is the fastest round, spread the slowest
over it.  The three decode rows of a shape are timed in turn within each of two passes and the faster pass kept, so a
drift of the machine does not fall on one of them alone.
Usage: python tools/kb_packetizer.py [--quick]"""
import math
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
QUICK = "--quick" in sys.argv
ROUNDS, WARM, ITERS = 3, 1, 3
CODES = (("v27", ya.Packetizer.v27, ya.ConvCode.v27), ("v29", ya.Packetizer.v29, ya.ConvCode.v29),
         ("v27p34", ya.Packetizer.v27p34, ya.ConvCode.v27p34))
NS = (32,) if QUICK else (32, 128, 1024)
FS = (64,) if QUICK else (64, 4096, 65536)
W = 4                                                     # CRC_32


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


def best_of(passes):
    return min(passes, key=lambda r: r[0])


print(f"# ms is the fastest of {ROUNDS} rounds of {ITERS} calls, spread the slowest over it; ratio = fused / (conv + copy); the bar "
      f"is the larger spread of the fused and conv rows")
print(f"{'code':>7s} {'n':>5s} {'F':>6s} {'N':>6s} {'C':>4s} {'fpw':>4s} {'waves':>5s} {'LDS':>7s} | {'fused ms':>10s} {'spread':>6s} | "
      f"{'conv ms':>10s} {'spread':>6s} | {'copy ms':>9s} {'spread':>6s} | {'ratio':>6s} {'bar':>6s} {'':>4s} | {'enc ms':>9s} {'spread':>6s} "
      f"{'conv enc':>9s} {'spread':>6s}")
missed = []
for name, make, make_conv in CODES:
    for n in NS:
        bits = 8 * (n + W)
        if bits > make_conv().nmax():
            continue
        N = make_conv().ncoded(bits)
        C = int(math.isqrt(N))
        for F in FS:
            q, c = make(n, columns=C), make_conv()
            q.set_stream(st.cuda_stream)
            c.set_stream(st.cuda_stream)
            assert q.enc_len() == N
            soft = torch.randint(0, 256, (F * N,), dtype=torch.uint8, device=dev)
            soft2 = torch.empty_like(soft)
            payload = torch.randint(0, 256, (F * n,), dtype=torch.uint8, device=dev)
            msg = torch.randint(0, 256, (F * (n + W),), dtype=torch.uint8, device=dev)
            out = torch.empty(F * (n + W), dtype=torch.uint8, device=dev)
            tx = torch.empty(F * N, dtype=torch.uint8, device=dev)
            valid = torch.empty(F, dtype=torch.uint8, device=dev)
            crc = torch.empty(F, dtype=torch.int32, device=dev)
            metric = torch.empty(F, dtype=torch.int32, device=dev)
            rows = {"fused": lambda: q.decode_block_devptr(soft, N, F, out, n, valid, crc, metric),
                    "conv": lambda: c.decode_block_devptr(soft, N, bits, F, out, n + W, metric),
                    "copy": lambda: soft2.copy_(soft)}
            passes = {k: [] for k in rows}
            for _ in range(2):
                for k, fn in rows.items():
                    passes[k].append(timed(fn))
            fused, conv, copy = (best_of(passes[k]) for k in ("fused", "conv", "copy"))
            enc = timed(lambda: q.encode_block_devptr(payload, n, F, 1, tx, N))
            cenc = timed(lambda: c.encode_block_devptr(msg, n + W, bits, F, tx, N))
            ratio, bar = fused[0] / (conv[0] + copy[0]), max(fused[1], conv[1])
            s = q.get_shape(F)
            verdict = "ok" if ratio <= bar else "MISS"
            if verdict == "MISS":
                missed.append((name, n, F, ratio, bar))
            print(f"{name:>7s} {n:5d} {F:6d} {N:6d} {C:4d} {s['frames_per_wave']:4d} {s['waves']:5d} {s['lds_bytes']:7d} | "
                  f"{fused[0]:10.4f} {fused[1]:6.3f} | {conv[0]:10.4f} {conv[1]:6.3f} | {copy[0]:9.4f} {copy[1]:6.3f} | "
                  f"{ratio:6.3f} {bar:6.3f} {verdict:>4s} | {enc[0]:9.4f} {enc[1]:6.3f} {cenc[0]:9.4f} {cenc[1]:6.3f}", flush=True)
            del q, c, soft, soft2, payload, msg, out, tx
print(f"# the bar is missed at {len(missed)} shapes" + "".join(f"; {m[0]} n={m[1]} F={m[2]}: x{m[3]:.3f} (bar {m[4]:.3f})" for m in missed))
