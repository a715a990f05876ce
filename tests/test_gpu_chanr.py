"""FirPfbChr on the GPU, every step of every call against the complex128 reference (tests/chanr_ref.py) computed on the
device: ||y_s - r_s|| <= TAU ||r_s|| + TAU rho, rho = rms step norm of the block.  A single step off by 1 % fails
(tests/test_chanr_ref_cpu.py).

General analyzer kernel and the synthesizer (transform + combine launches): the shapes of the CPU tests plus M 512 with
P 384, m 6 and P 1, m 1; per shape 8m ceil(M/P) + 13 steps, then 67, then 1.

Column analyzer kernel, pinned with set_kernel(2) and asserted through get_last_kernel().  launch_firpfbchr_col cuts the
block into runs of Q `run` steps (Q = M / gcd(M, P) phase classes of `run` class steps each), one work unit per class
of a run and G = 256 / M units per workgroup; `run` = 16 below 32 * 1024 * G steps, i.e. at every size here.  A launch
holds full workgroups only when the steps are a multiple of 16 Q and the units a multiple of G.  Per shape (M, P, 2m),
first call -> runs, units, grid:

  64, 48, 8    Q 4, G 4   64 steps: 1 run, 4 units, grid 1, all full      65: 2 runs, grid 2, one unit with 1 class step
  64, 48, 6    the same on the 8-tap kernel, two zero taps
  64, 16, 8    Q 4, G 4, P/g 1   64: grid 1      65: grid 2
  128, 80, 4   Q 8, G 2, P/g 5 > 2m (the whole window is replaced)   128: 1 run, 8 units, grid 4     129: grid 8
  256, 192, 16 Q 4, G 1   64: 1 run, 4 units, grid 4      65: grid 8
  64, 32, 8    Q 2, G 4   64: 2 runs, 4 units, grid 1     65: 3 runs, grid 2     also against ya.FirPfbCh2
  64, 64, 16   Q 1, G 4   64: 4 runs, 4 units, grid 1     65: 5 runs, grid 2     also against ya.FirPfbCh times M e^{+j 2 pi k / M}
  64, 48, 8    43 690 steps (2^21 samples): 683 runs, 2732 units, grid 683
  256, 192, 16 10 922 steps (2^21 samples): 171 runs, 684 units, grid 684

Every first call is followed by two calls of 67 steps.  After a count of full workgroups (a multiple of Q) the first of
them starts in class 0 and the second in class 67 mod Q = 3 (Q 4, 8) or 1 (Q 2); after that count plus one the first
starts in class 1.  So for Q > 1 every case has a 67-step call that starts in a class q != 0.

Per kernel the long call equals, bit for bit, the same stream cut into three calls on that kernel; reset() followed by
a block equals a fresh object's output; and the column analyzer followed by the synthesizer reconstructs the input to
within 0.1 dB of the complex128 chain on the same samples.

Worst per-step ratio measured on the MI355X over every case of this file: 2.17e-7 (synthesizer M 512, P 1, m 1);
CHANR_FRAME_TAU in tests/chanr_ref.py is three times that."""
import math

import numpy as np
import pytest
import torch

from chan_ref import GPU_FRAME_TAU, FirPfbCh2Ref, FirPfbChRef, FrameCheck
from chanr_ref import CHANR_FRAME_TAU as TAU
from chanr_ref import FirPfbChrRef, auto_takes_column
from gpu_util import SEED
from test_chanr_ref_cpu import SHAPES, reconstruction_db

pytestmark = pytest.mark.gpu

SEAM = 67
GENERAL = SHAPES + [(512, 384, 6), (512, 1, 1)]
# (M, P, 2m, steps of the first call)
COLUMN = [(64, 48, 8, 64), (64, 48, 8, 65), (64, 48, 6, 64), (64, 48, 6, 65), (64, 16, 8, 64), (64, 16, 8, 65),
          (128, 80, 4, 128), (128, 80, 4, 129), (256, 192, 16, 64), (256, 192, 16, 65), (64, 32, 8, 64), (64, 32, 8, 65),
          (64, 64, 16, 64), (64, 64, 16, 65), (64, 48, 8, 43690), (256, 192, 16, 10922)]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


def _proto(ya, M, m, fc):
    h = ya.fir_design_kaiser(2 * M * m + 1, fc, 60.0)
    return (h * M / h.sum()).astype(np.float32)


def _gen(ya, seed, n):
    torch.cuda.synchronize()                                  # the allocator may hand back memory torch just used
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    ya.gen_complex_dev(seed, n, out=x)
    ya.synchronize()
    return x


def _run_calls(ya, run, x, calls, ui, uo, after=None):
    """the stream x through run() in calls of `calls` steps; [sum(calls), uo] on the device"""
    n = sum(calls)
    y = torch.empty(n * uo, dtype=torch.complex64, device="cuda")
    a = 0
    for c in calls:
        run(x[a * ui: (a + c) * ui], c, y[a * uo: (a + c) * uo])
        if after:
            after()
        a += c
    ya.synchronize()
    return y.view(n, uo)


def _check(chunks, x, y, what, tau=TAU):
    fc = FrameCheck(y.shape[0], device="cuda")
    for s0, r in chunks(x):
        fc.add(s0, r, y[s0: s0 + r.shape[0]])
    worst, s, rel = fc.worst()
    print(f"{what}: worst step ratio {worst:.3e} at step {s}, rel L2 {rel:.3e}")
    assert worst <= tau, f"{what}: step {s} off by {worst:.3e} (||e_s|| / (||r_s|| + rho)), bound {tau:.1e}"


def _three(n, Q):
    """n steps as three calls whose boundaries are off the multiples of Q"""
    a, b = n // 3 + 1, (2 * n) // 3 + 2
    a += 1 if Q > 1 and a % Q == 0 else 0
    b += 1 if Q > 1 and b % Q == 0 else 0
    assert 0 < a < b < n
    return [a, b - a, n - b]


@pytest.mark.parametrize("M,P,m", GENERAL, ids=[f"M{M}-P{P}-m{m}" for M, P, m in GENERAL])
def test_general_kernels_every_step(ya, M, P, m):
    calls = [8 * m * -(-M // P) + 13, SEAM, 1]
    n, Q = sum(calls), M // math.gcd(M, P)
    ha, hs = _proto(ya, M, m, 0.5 / P), _proto(ya, M, m, 0.5 / M)
    x = _gen(ya, SEED + 70 + M + P, n * P)
    q = ya.FirPfbChr(M, P, m, ha)
    q.set_kernel(1)
    y = _run_calls(ya, q.analyzer_execute_devptr, x, calls, P, M, after=lambda: q.get_last_kernel() == 1 or pytest.fail("kernel"))
    _check(FirPfbChrRef(M, P, m, ha, device="cuda").analyzer_chunks, x, y, f"analyzer M {M} P {P} m {m}")
    q2 = ya.FirPfbChr(M, P, m, ha)
    q2.set_kernel(1)
    assert torch.equal(_run_calls(ya, q2.analyzer_execute_devptr, x, _three(n, Q), P, M), y), "cut stream differs (analyzer)"
    q.reset()
    q3 = ya.FirPfbChr(M, P, m, ha)
    q3.set_kernel(1)
    assert torch.equal(_run_calls(ya, q.analyzer_execute_devptr, x, [calls[0]], P, M),
                       _run_calls(ya, q3.analyzer_execute_devptr, x, [calls[0]], P, M)), "reset() != fresh (analyzer)"
    X = _gen(ya, SEED + 71 + M + P, n * M)
    s = ya.FirPfbChr(M, P, m, hs)
    ys = _run_calls(ya, s.synthesizer_execute_devptr, X, calls, M, P)
    _check(FirPfbChrRef(M, P, m, hs, device="cuda").synthesizer_chunks, X, ys, f"synthesizer M {M} P {P} m {m}")
    s2 = ya.FirPfbChr(M, P, m, hs)
    assert torch.equal(_run_calls(ya, s2.synthesizer_execute_devptr, X, _three(n, Q), M, P), ys), "cut stream differs (synthesizer)"
    s.reset()
    assert torch.equal(_run_calls(ya, s.synthesizer_execute_devptr, X, [calls[0]], M, P), ys[: calls[0]]), "reset() != fresh (synthesizer)"


@pytest.mark.parametrize("M,P,p,n1", COLUMN, ids=[f"M{M}-P{P}-2m{p}-{n}" for M, P, p, n in COLUMN])
def test_column_kernel_every_step(ya, M, P, p, n1):
    m, Q = p // 2, M // math.gcd(M, P)
    calls = [n1, SEAM, SEAM]
    n = sum(calls)
    assert Q == 1 or n1 % Q != 0 or (n1 + SEAM) % Q != 0       # a 67-step call starts in a class q != 0
    fc = {M: 0.5 / M, M // 2: 1.0 / M}.get(P, 0.5 / P)         # FirPfbCh's and FirPfbCh2's prototypes at their rates
    h = _proto(ya, M, m, fc)
    x = _gen(ya, SEED + 72 + M + P + p, n * P)
    q = ya.FirPfbChr(M, P, m, h)
    q.set_kernel(2)
    y = _run_calls(ya, q.analyzer_execute_devptr, x, calls, P, M, after=lambda: q.get_last_kernel() == 2 or pytest.fail("kernel"))
    _check(FirPfbChrRef(M, P, m, h, device="cuda").analyzer_chunks, x, y, f"column M {M} P {P} 2m {p}, {n1} + 67 + 67")
    q2 = ya.FirPfbChr(M, P, m, h)
    q2.set_kernel(2)
    assert torch.equal(_run_calls(ya, q2.analyzer_execute_devptr, x, _three(n, Q), P, M), y), "cut stream differs"
    assert q2.get_last_kernel() == 2
    q.reset()
    q3 = ya.FirPfbChr(M, P, m, h)
    q3.set_kernel(2)
    assert torch.equal(_run_calls(ya, q.analyzer_execute_devptr, x, [n1], P, M),
                       _run_calls(ya, q3.analyzer_execute_devptr, x, [n1], P, M)), "reset() != fresh"
    if 2 * P == M:
        # the same FIR sums in the same order, another transform: FirPfbCh2 at its own bound
        y2 = _run_calls(ya, ya.FirPfbCh2(M, m, h).analyzer_execute_dev, x, calls, P, M)
        fcmp = FrameCheck(n, device="cuda")
        fcmp.add(0, y2.to(torch.complex128), y)
        worst, s, _ = fcmp.worst()
        print(f"against FirPfbCh2: worst step ratio {worst:.3e} at step {s}")
        assert worst <= GPU_FRAME_TAU
        _check(FirPfbCh2Ref(M, m, h, device="cuda").analyzer_chunks, x, y, "against FirPfbCh2Ref", GPU_FRAME_TAU)
    if P == M:
        y1 = _run_calls(ya, ya.FirPfbCh(M, p, h).analyzer_execute_dev, x, calls, M, M)
        rot = M * torch.exp(2j * math.pi * torch.arange(M, dtype=torch.float64, device="cuda") / M)
        fcmp = FrameCheck(n, device="cuda")
        fcmp.add(0, y1.to(torch.complex128), y.to(torch.complex128) * rot)
        worst, s, _ = fcmp.worst()
        print(f"against FirPfbCh: worst frame ratio {worst:.3e} at frame {s}")
        assert worst <= GPU_FRAME_TAU
        _check(FirPfbChRef(M, p, h, device="cuda").analyzer_chunks, x, y.to(torch.complex128) * rot, "against FirPfbChRef",
               GPU_FRAME_TAU)


def test_column_kernel_is_refused_where_it_does_not_serve(ya):
    for M, P, m in [(32, 24, 4), (64, 47, 4), (64, 48, 9), (512, 384, 4)]:
        q = ya.FirPfbChr(M, P, m, np.ones(2 * M * m, np.float32))
        with pytest.raises(ya.ConfigError):
            q.set_kernel(2)
    with pytest.raises(ya.ConfigError):
        ya.FirPfbChr(64, 48, 4, np.ones(512, np.float32)).set_kernel(3)


def test_reconstruction_through_the_column_analyzer_and_the_synthesizer(ya):
    """M 64, P 48, m 8, As 60: f32 rounding sits about 60 dB below the design error of -63 dB, so the GPU chain's figure is
    the complex128 chain's on the same input to within 0.1 dB"""
    M, P, m, ns = 64, 48, 8, 300
    ha, hs = _proto(ya, M, m, 0.5 / P), _proto(ya, M, m, 0.5 / M)
    x = _gen(ya, SEED + 73, ns * P)
    a, s = ya.FirPfbChr(M, P, m, ha), ya.FirPfbChr(M, P, m, hs)
    a.set_kernel(2)
    Y = torch.empty(ns * M, dtype=torch.complex64, device="cuda")
    y = torch.empty(ns * P, dtype=torch.complex64, device="cuda")
    a.analyzer_execute_devptr(x, ns, Y)
    s.synthesizer_execute_devptr(Y, ns, y)
    ya.synchronize()
    assert a.get_last_kernel() == 2
    Y64 = FirPfbChrRef(M, P, m, ha, device="cuda").analyzer_execute(x)
    y64 = FirPfbChrRef(M, P, m, hs, device="cuda").synthesizer_execute(Y64).reshape(-1)
    delay = 2 * M * m - P + 1
    xh = x.cpu().numpy()
    got, want = reconstruction_db(xh, y.cpu().numpy(), delay), reconstruction_db(xh, y64.cpu().numpy(), delay)
    print(f"reconstruction M {M} P {P} m {m}: GPU f32 chain {got:.3f} dB, complex128 chain {want:.3f} dB")
    assert want < -60.0
    assert abs(got - want) <= 0.1


# (M, P, m, input samples) -> the kernel choice auto takes: the column kernel only where profiles/r13_kbench_chanr.txt has
# it ahead of the general one at both measured block lengths, and never below floor(2^20 / P) steps (not measured)
AUTO = [((64, 64, 4, 1 << 20), 2), ((64, 64, 4, (1 << 20) - 64), 1), ((64, 16, 3, 1 << 20), 2), ((64, 16, 1, 1 << 20), 1),
        ((64, 48, 4, 1 << 20), 2), ((128, 96, 4, 1 << 20), 2), ((256, 192, 4, 1 << 20), 1), ((256, 192, 8, 1 << 20), 2),
        ((64, 48, 2, 1 << 20), 1), ((64, 48, 3, 1 << 20), 1), ((64, 40, 8, 1 << 20), 2), ((64, 40, 4, 1 << 20), 1),
        ((64, 56, 8, 1 << 20), 2), ((128, 112, 8, 1 << 20), 1), ((100, 75, 5, 1 << 20), 1)]


@pytest.mark.parametrize("shape,want", AUTO, ids=[str(s) for s, _ in AUTO])
def test_auto_follows_the_measured_table(ya, shape, want):
    M, P, m, n = shape
    ns = -(-n // P)
    x = _gen(ya, SEED + 74, ns * P)
    y = torch.empty(ns * M, dtype=torch.complex64, device="cuda")
    q = ya.FirPfbChr(M, P, m, _proto(ya, M, m, 0.5 / P))
    assert q.get_last_kernel() == 0
    run = ns - 1 if n < (1 << 20) else ns
    assert want == (2 if auto_takes_column(M, P, m, run) else 1)      # the rule tests/test_chanr_table_cpu.py holds to the table
    q.analyzer_execute_devptr(x[: run * P], run, y)
    ya.synchronize()
    assert q.get_last_kernel() == want


def test_a_synthesizer_history_too_large_is_refused_by_the_synthesizer_only(ya):
    """M 4096, P 1, m 1: the synthesizer would carry 8191 steps of 4096 values (2^25 > the limit of 2^23), which its first
    call refuses; the analyzer of the same object, whose history is 8191 samples, runs"""
    M, P, m, ns = 4096, 1, 1, 300
    h = _proto(ya, M, m, 0.5 / M)
    x = _gen(ya, SEED + 75, ns)
    q = ya.FirPfbChr(M, P, m, h)
    y = _run_calls(ya, q.analyzer_execute_devptr, x, [200, 100], P, M)
    _check(FirPfbChrRef(M, P, m, h, device="cuda").analyzer_chunks, x, y, f"analyzer M {M} P {P} m {m}")
    X = torch.zeros(M, dtype=torch.complex64, device="cuda")
    out = torch.empty(P, dtype=torch.complex64, device="cuda")
    with pytest.raises(ya.ConfigError, match="synthesizer history"):
        q.synthesizer_execute_devptr(X, 1, out)
    q.reset()
