#!/usr/bin/env python3
"""EqRls block form (GPU box): step_block_devptr in TRAIN mode at k = 1 for p in {4, 8, 16, 32}, C in {64, 1024, 16384,
262144} (where channels p p is within EQRLS_MATRIX_MAX) and every admissible number L of lanes per channel (set_lanes);
`plan` marks the planner's own choice for that (C, p).  The input is QPSK symbols in a little noise and TRAIN's symbols
are those symbols, so the recursion stays well conditioned; `finite` says P0 and the weights stayed finite.  Three
rounds; a round is HIP events around ITERS calls after WARM warm-up calls (the state is carried from call to call, as in
a stream); the table gives the fastest round and the slowest / fastest spread, in millions of channel-steps per second
(one step = one symbol of one channel: execute and the O(p^3) update).
Usage: python tools/kb_eqrls.py"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import yagi_amd as ya

dev = torch.device("cuda")
st = torch.cuda.current_stream()
ROUNDS, WARM, ITERS = 3, 1, 3
ORDERS, BANKS = (4, 8, 16, 32), (64, 1024, 16384, 262144)
U = ya.EqRlsUpdate


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


def row(p, C, L, planned):
    nsym = max(16, min(1024, (1 << 24) // (C * p * p)))
    q = ya.EqRls(C, p)
    q.set_stream(st.cuda_stream)
    q.set_lanes(L)
    pts = torch.tensor([1 + 1j, -1 + 1j, 1 - 1j, -1 - 1j], dtype=torch.complex64, device=dev) * np.sqrt(0.5)
    d = pts[torch.randint(0, 4, (nsym, C), device=dev)].contiguous()
    x = (d + 0.05 * torch.randn(nsym, C, dtype=torch.complex64, device=dev)).contiguous()
    y = torch.empty(nsym * C, dtype=torch.complex64, device=dev)

    def call():
        q.step_block_devptr(1, U.TRAIN, x, C, nsym, d, C, y, C)

    t = [timed(call, WARM, ITERS) for _ in range(ROUNDS)]
    best = min(t)
    rate = nsym * C / (best * 1e-3)                                  # channel-steps per second
    finite = bool(np.isfinite(q.get_matrix()).all() and np.isfinite(q.get_coefficients()).all())
    lds = ya.eqrls_plan(C, p)[1] if planned else 0
    print(f"{p:3d} {C:6d} {L:3d} {'plan' if planned else '':>5s} {nsym:6d} {best:10.3f} {max(t) / best:7.3f} {rate / 1e6:11.3f} "
          f"{str(finite):>7s} {lds if planned else '':>8}", flush=True)


print(f"# step_block TRAIN, k = 1; ms is the fastest of {ROUNDS} rounds of {ITERS} calls, spread the slowest over it; "
      f"Mstep/s counts channel-steps; LDS bytes of the planned shape")
print(f"{'p':>3s} {'C':>6s} {'L':>3s} {'':>5s} {'nsym':>6s} {'ms':>10s} {'spread':>7s} {'Mstep/s':>11s} {'finite':>7s} {'LDS':>8s}")
for p in ORDERS:
    for C in BANKS:
        if C * p * p > ya.EQRLS_MATRIX_MAX:
            continue
        planned, _, adm = ya.eqrls_plan(C, p)
        for L in adm:
            row(p, C, L, L == planned)
