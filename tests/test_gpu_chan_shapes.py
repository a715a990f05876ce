"""Channelizers at the launch shapes of the column-sliding kernels, every output frame against the complex128 reference
(tests/chan_ref.py) computed on the device.

The column kernels pick their workgroup count `wgs` and run length `run` from the block length (chan_kernels.hip:
launch_firpfbch_col, launch_firpfbch_wide, launch_firpfbch_syn_col, launch_firpfbch2_col, launch_firpfbch2_wide,
launch_firpfbch2_syn_col); a block that does not split into whole column groups runs the checked (FULL = false) kernel
for the whole launch.  What each case reaches with its first, long call (G = 256 / M column groups per workgroup;
`grid` = workgroups launched; frames for firpfbch, steps for firpfbch2):

  firpfbch analyzer (column)       M 64, p 16, 393 216 frames     wgs 1536 (middle), run 64, full
                                   M 64, p 16, 393 253 frames     wgs 1536, run 64, checked (grid 1537, last partial)
                                   M 64, p 16, 2^22 frames        wgs 4096 (upper clamp), run 256 (clamp), full; 2^28 samples
                                   M 64, p 8, 786 437 frames      wgs 1536 of cap 2048, run 128, checked
                                   M 64, p 6, 786 437 frames      the same on the P = 8 kernel, two zero taps
                                   M 8, p 8, 2^23 frames          wgs 1024, run 256 (clamp), full, G = 32
                                   M 256, p 16, 2^18 frames       wgs 1024, run 256 (clamp), full, G = 1
  firpfbch analyzer (wide)         M 512, p 8, 2^17 + 3 frames    run 128, checked (grid 1025)
                                   M 1024, p 4, 2^16 frames       run 64, full (grid 1024)
  firpfbch2 analyzer (column)      M 256, m 4, 196 608 steps      wgs 1536, run 128, full
                                   M 256, m 4, 196 714 steps      wgs 1536, run 128, checked
                                   M 256, m 4, 2^18 + 2 steps     wgs 2048, run 128, checked
                                   M 256, m 3, 196 714 steps      wgs 1536, run 128, checked, 2m = 6 on the P = 8 kernel
                                   M 8, m 4, 2^24 steps           wgs 1024, run 512 (clamp), full, G = 32
  firpfbch2 analyzer (wide)        M 512, m 2, 2^19 steps         run 512 (clamp), full (grid 1024)
  firpfbch2 shard kernel           M 256, m 4, 2^19 steps, R 2 and 8, every r: nranks > 1 column path, wgs 4096, run 128,
                                   full (config C5's size)
  firpfbch synthesizer (column)    M 64, p 16, 2^20 frames        run 256 (clamp), full (grid 1024)
                                   M 256, p 8, 2^18 + 7 frames    run 256, checked (grid 1025)
                                   M 16, p 5, 2^22 frames         run 256, full, P = 8 kernel, three zero taps
  firpfbch2 synthesizer (column)   M 256, m 4, 2^19 steps         run 256 (clamp), full, ring 16 (grid 2048)
                                   M 64, m 2, 2^18 + 5 steps      run 64, checked, ring 8 (grid 1025); odd step0 on the
                                                                  second call
                                   M 64, m 3, 2^20 steps          run 256, full, ring 16 with 4 zero lags

Every case then continues the stream with a second call of 67 frames / steps (odd: firpfbch2 runs it on the column
kernel, with the step parity the first call left), and every frame of both calls is checked:
||y_f - r_f|| <= TAU ||r_f|| + TAU rho, rho = rms frame norm of the block, plus the global relative L2 bounds of
test_gpu_chan.py.  A single frame off by 1 % fails (test_chan_ref_cpu.py).

The long call also equals, bit for bit, the same stream cut into calls of 2^22 input samples (the last one takes the
remainder): a frame's arithmetic -- the per-column FIR in tap order, the transform -- does not depend on `wgs` or `run`,
and every such call is >= 64 frames (an even number of steps for firpfbch2) so that it stays on the same kernel."""
import numpy as np
import pytest
import torch

from chan_ref import GPU_FRAME_TAU as TAU
from chan_ref import FirPfbCh2Ref, FirPfbChRef, FrameCheck, shard_columns
from gpu_util import SEED

pytestmark = pytest.mark.gpu

SEAM = 67                 # frames / steps of the second call
CUT = 1 << 22             # input samples per call of the cut stream


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


# (op, M, p for firpfbch / m for firpfbch2, frames or steps of the first call)
CASES = [
    ("ana", 64, 16, 393216), ("ana", 64, 16, 393253), ("ana", 64, 16, 1 << 22), ("ana", 64, 8, 786437),
    ("ana", 64, 6, 786437), ("ana", 8, 8, 1 << 23), ("ana", 256, 16, 1 << 18),
    ("ana", 512, 8, (1 << 17) + 3), ("ana", 1024, 4, 1 << 16),
    ("ana2", 256, 4, 196608), ("ana2", 256, 4, 196714), ("ana2", 256, 4, (1 << 18) + 2), ("ana2", 256, 3, 196714),
    ("ana2", 8, 4, 1 << 24), ("ana2", 512, 2, 1 << 19),
    ("syn", 64, 16, 1 << 20), ("syn", 256, 8, (1 << 18) + 7), ("syn", 16, 5, 1 << 22),
    ("syn2", 256, 4, 1 << 19), ("syn2", 64, 2, (1 << 18) + 5), ("syn2", 64, 3, 1 << 20),
]


def _taps(ya, op, M, k):
    if op == "ana" or op == "syn":
        return ya.fir_design_kaiser(M * k + 1, 0.5 / M, 60.0)
    h = ya.fir_design_kaiser(2 * M * k + 1, (1.0 if op == "ana2" else 0.5) / M, 60.0)
    return (h * M / h.sum()).astype(np.float32)


def _units(op, M):
    """(input samples, output samples) per frame / step"""
    return {"ana": (M, M), "syn": (M, M), "ana2": (M // 2, M), "syn2": (M, M // 2)}[op]


def _objects(ya, op, M, k, h):
    if op in ("ana", "syn"):
        q, ref = ya.FirPfbCh(M, k, h), FirPfbChRef(M, k, h, device="cuda")
    else:
        q, ref = ya.FirPfbCh2(M, k, h), FirPfbCh2Ref(M, k, h, device="cuda")
    run = q.analyzer_execute_dev if op.startswith("ana") else q.synthesizer_execute_dev
    chunks = ref.analyzer_chunks if op.startswith("ana") else ref.synthesizer_chunks
    return q, run, chunks


def _gen(ya, seed, n, first=0):
    torch.cuda.synchronize()                                  # the allocator may hand back memory torch just used
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    ya.gen_complex_dev(seed, n, out=x, first=first)
    ya.synchronize()
    return x


def _pieces(n, per_call, even):
    """the cut stream: calls of per_call frames / steps, the remainder joined to the last call when shorter than 64"""
    cuts = list(range(0, n, per_call)) + [n]
    if len(cuts) > 2 and cuts[-1] - cuts[-2] < 64:
        del cuts[-2]
    assert all(b - a >= 64 for a, b in zip(cuts, cuts[1:]))
    assert not even or all((b - a) % 2 == 0 for a, b in zip(cuts[:-2], cuts[1:-1]))
    return list(zip(cuts, cuts[1:]))


def _check(fc, what, rel_bound):
    worst, f, rel = fc.worst()
    print(f"{what}: worst frame ratio {worst:.3e} at frame {f}, rel L2 {rel:.3e}")
    assert worst <= TAU, f"{what}: frame {f} off by {worst:.3e} (||e_f|| / (||r_f|| + rho)), bound {TAU:.1e}"
    assert rel <= rel_bound, (what, rel)


@pytest.mark.parametrize("op,M,k,n", CASES, ids=[f"{o}-M{M}-{k}-{n}" for o, M, k, n in CASES])
def test_chan_every_frame_at_launch_shape(ya, op, M, k, n):
    seed = SEED + 30 + M + k
    ui, uo = _units(op, M)
    h = _taps(ya, op, M, k)
    q, run, chunks = _objects(ya, op, M, k, h)
    x = _gen(ya, seed, (n + SEAM) * ui)
    y = torch.empty((n + SEAM) * uo, dtype=torch.complex64, device="cuda")
    run(x[: n * ui], n, y[: n * uo])                          # the long call at the target shape
    run(x[n * ui:], SEAM, y[n * uo:])                         # continues the stream across the seam
    ya.synchronize()
    y2 = y.view(n + SEAM, uo)
    fc = FrameCheck(n + SEAM, device="cuda")
    for f0, r in chunks(x):
        fc.add(f0, r, y2[f0: f0 + r.shape[0]])
        del r
    _check(fc, f"{op} M {M} {'p' if op in ('ana', 'syn') else 'm'} {k}, {n} + {SEAM}",
           2e-6 if op.startswith("ana") else 3e-6)
    del fc
    # the same stream cut into calls of 2^22 input samples: bit for bit
    q2, run2, _ = _objects(ya, op, M, k, h)
    yc = torch.empty(n * uo, dtype=torch.complex64, device="cuda")
    for a, b in _pieces(n, CUT // ui, op == "ana2"):
        run2(x[a * ui: b * ui], b - a, yc[a * uo: b * uo])
    ya.synchronize()
    same = torch.equal(yc, y[: n * uo])
    if not same:
        bad = torch.nonzero((yc != y[: n * uo]).view(n, uo).any(dim=1)).flatten()
        pytest.fail(f"cut stream differs from the long call in {bad.numel()} frames, first {bad[:8].tolist()}")
    del x, y, y2, yc, q, q2
    torch.cuda.empty_cache()


def test_firpfbch2_shards_every_frame_c5_size(ya):
    """the sharded analyzer (nranks > 1 column path of firpfbch2_col_kernel, SHARDED = true) at config C5's size: M 256,
    m 4, 2^19 steps (wgs 4096, run 128, full), every rank r of R = 2 and R = 8, then 67 steps across the seam; every
    step of every shard against the reference's channels k = r + R q"""
    M, m, n = 256, 4, 1 << 19
    M2 = M // 2
    h = _taps(ya, "ana2", M, m)
    x = _gen(ya, SEED + 5, (n + SEAM) * M2)
    shards = []
    for R in (2, 8):
        for r in range(R):
            q = ya.FirPfbCh2(M, m, h)
            ys = torch.empty((n + SEAM) * (M // R), dtype=torch.complex64, device="cuda")
            q.analyzer_execute_shard_dev(x[: n * M2], n, r, R, ys[: n * (M // R)])
            q.analyzer_execute_shard_dev(x[n * M2:], SEAM, r, R, ys[n * (M // R):])
            shards.append((r, R, ys.view(n + SEAM, M // R), FrameCheck(n + SEAM, device="cuda"), q))
    ya.synchronize()
    for f0, ref in FirPfbCh2Ref(M, m, h, device="cuda").analyzer_chunks(x):
        for r, R, ys, fc, _ in shards:
            fc.add(f0, shard_columns(ref, r, R), ys[f0: f0 + ref.shape[0]])
    for r, R, _, fc, _ in shards:
        _check(fc, f"shard r {r} of R {R}", 3e-6)
    del x, shards
    torch.cuda.empty_cache()
