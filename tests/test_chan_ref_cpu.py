"""tests/chan_ref.py (the complex128 channelizer reference of the GPU shape tests) pinned to the oracle on small blocks:
firpfbch / firpfbch2 analyzers and synthesizers, every frame, power-of-two and other channel counts, branch lengths
1 .. 16 (the zero-padded sizes included), blocks cut into two or three calls (odd step counts for firpfbch2), and
sub-band shard columns.  The oracle computes in f32, hence the 1e-6 per-frame bound."""
import numpy as np
import pytest
import torch

from chan_ref import GPU_FRAME_TAU, FirPfbCh2Ref, FirPfbChRef, FrameCheck, shard_columns
from gpu_util import SEED

TAU = 1e-6


def _check_frames(ref, want, tau=TAU):
    """ref: the complex128 reference's frames, want: the oracle's"""
    want = torch.as_tensor(np.ascontiguousarray(want))
    assert ref.shape == want.shape, (ref.shape, want.shape)
    fc = FrameCheck(ref.shape[0])
    fc.add(0, ref, want)
    worst, f, rel = fc.worst()
    assert worst <= tau, f"worst frame {f}: ratio {worst:.3e} (rel L2 {rel:.3e})"


def _cuts(n, ncalls):
    cuts = [0, n // 3 + 1, (2 * n) // 3 + 2, n][: ncalls] + [n]
    return sorted(set(min(c, n) for c in cuts))


M_P = [(2, 1), (4, 2), (6, 3), (8, 4), (10, 5), (48, 6), (64, 16), (100, 10), (256, 12), (512, 14), (64, 8), (8, 16),
       (6, 2), (2, 3), (4, 1), (16, 5)]


@pytest.mark.parametrize("M,p", M_P)
@pytest.mark.parametrize("ncalls", [1, 2, 3])
def test_firpfbch_analyzer_ref_vs_oracle(oracle, M, p, ncalls):
    h = oracle.fir_design_kaiser(M * p + 1, 0.5 / M, 60.0)         # the last tap must be ignored
    nfr = 3 * p + 11
    x = oracle.gen_complex(SEED + 20 + M, nfr * M)
    want = oracle.FirPfbCh(M, p, h).analyzer_execute(x)
    ref = FirPfbChRef(M, p, h)
    c = _cuts(nfr, ncalls)
    got = torch.cat([ref.analyzer_execute(torch.from_numpy(x[a * M: b * M]), chunk=5 * M) for a, b in zip(c, c[1:])])
    _check_frames(got, want)


@pytest.mark.parametrize("M,p", M_P)
@pytest.mark.parametrize("ncalls", [1, 3])
def test_firpfbch_synthesizer_ref_vs_oracle(oracle, M, p, ncalls):
    h = oracle.fir_design_kaiser(M * p + 1, 0.5 / M, 60.0)
    nfr = 2 * p + 9
    X = oracle.gen_complex(SEED + 21 + M, nfr * M)
    want = oracle.FirPfbCh(M, p, h).synthesizer_execute(X).reshape(nfr, M)
    ref = FirPfbChRef(M, p, h)
    c = _cuts(nfr, ncalls)
    got = torch.cat([ref.synthesizer_execute(torch.from_numpy(X[a * M: b * M]), chunk=3 * M) for a, b in zip(c, c[1:])])
    _check_frames(got, want)


M_m = [(2, 1), (4, 2), (6, 3), (8, 4), (10, 1), (48, 3), (64, 8), (100, 5), (256, 4), (512, 6), (64, 7), (8, 2),
       (256, 3), (6, 5)]


@pytest.mark.parametrize("M,m", M_m)
@pytest.mark.parametrize("ncalls", [1, 2, 3])
def test_firpfbch2_analyzer_ref_vs_oracle(oracle, M, m, ncalls):
    h = oracle.fir_design_kaiser(2 * M * m + 1, 1.0 / M, 60.0)
    h = (h * M / h.sum()).astype(np.float32)
    M2 = M // 2
    ns = 8 * m + 13                                                 # odd: the cuts fall on odd steps
    x = oracle.gen_complex(SEED + 22 + M, ns * M2)
    want = oracle.FirPfbCh2(M, m, h).analyzer_execute(x)
    ref = FirPfbCh2Ref(M, m, h)
    c = _cuts(ns, ncalls)
    got = torch.cat([ref.analyzer_execute(torch.from_numpy(x[a * M2: b * M2]), chunk=7 * M2) for a, b in zip(c, c[1:])])
    _check_frames(got, want)
    for R in (r for r in (2, 3, 8) if M % r == 0):
        for r in sorted({0, 1, R - 1}):
            _check_frames(shard_columns(got, r, R), want[:, r::R])


@pytest.mark.parametrize("M,m", M_m)
@pytest.mark.parametrize("ncalls", [1, 3])
def test_firpfbch2_synthesizer_ref_vs_oracle(oracle, M, m, ncalls):
    h = oracle.fir_design_kaiser(2 * M * m + 1, 0.5 / M, 60.0)
    h = (h * M / h.sum()).astype(np.float32)
    ns = 4 * m + 9
    X = oracle.gen_complex(SEED + 23 + M, ns * M)
    want = oracle.FirPfbCh2(M, m, h).synthesizer_execute(X).reshape(ns, M // 2)
    ref = FirPfbCh2Ref(M, m, h)
    c = _cuts(ns, ncalls)
    got = torch.cat([ref.synthesizer_execute(torch.from_numpy(X[a * M: b * M]), chunk=3 * M) for a, b in zip(c, c[1:])])
    _check_frames(got, want)


def test_frame_check_catches_one_frame_off_by_one_percent(oracle):
    """the per-frame bound of the GPU shape tests (tau = 4e-7) fails a single frame that is 1 % off"""
    M, p = 64, 16
    h = oracle.fir_design_kaiser(M * p + 1, 0.5 / M, 60.0)
    nfr = 4096
    x = torch.from_numpy(oracle.gen_complex(SEED + 24, nfr * M))
    want = FirPfbChRef(M, p, h).analyzer_execute(x)
    bad = want.clone()
    bad[1234] *= 1.01
    fc = FrameCheck(nfr)
    fc.add(0, want, bad)
    worst, f, _ = fc.worst()
    assert f == 1234 and worst > 1e-3 > 100 * GPU_FRAME_TAU
