"""The frequency-domain stream kernel (variant 4) reads its per-lane constants from tables laid out in pairs for 16-byte
loads: the six row entries of a main-wave lane, wave 0's six transform twiddles, the scaled conj(DFT_512{g}) / 512 of
the fast correction sum and the scaled FFT{h} (yagi_amd/csrc/stream_tables.hpp).  Small shapes at which a wrong slot shows: every tap count at which
the correction operands' mask 64 a + l < L - 1 changes (both ends and each 64-boundary), one to three frames per call
with a second call that takes its window from the object, the table rebuilt after a scale change on the plain and on
the pipelined entry path, pipelined against plain calls bit for bit, and an integer impulse across a frame boundary.

The stream object has no set_coefficients entry point (include/yagi_hip.h): its taps are fixed at creation, so the
table rebuild after a change of taps is reached through a new object only -- which every case here does."""
import numpy as np
import pytest

from gpu_util import SEED, rel_l2

pytestmark = pytest.mark.gpu

NFFT = 4096
LENGTHS = [1, 2, 64, 65, 128, 129, 192, 193, 255, 256, 257]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


@pytest.fixture(scope="module")
def stream(oracle):
    """six frames of the C2 stream, shared and never written"""
    x = oracle.gen_complex(SEED + 2, 6 * NFFT)
    x.setflags(write=False)
    return x


def spectra_truth(oracle, h, scale, x):
    y = oracle.fir_block_f64("crcf", h, x, scale=scale)
    return np.array([np.fft.fft(y[f * NFFT:(f + 1) * NFFT]) for f in range(len(x) // NFFT)])


def run_dev(ya, q, x, sizes):
    """x through q.execute_dev in calls of `sizes` frames; returns [frames, 4096] after join + synchronize"""
    nf = sum(sizes)
    dx = ya.DeviceArray.from_numpy(np.ascontiguousarray(x[: nf * NFFT]))
    dy = ya.DeviceArray(nf * NFFT, np.complex64)
    f0 = 0
    for s in sizes:
        q.execute_dev(dx.ptr + 8 * NFFT * f0, s, dy.ptr + 8 * NFFT * f0)
        f0 += s
    q.join()
    ya.synchronize()
    got = dy.to_numpy().reshape(nf, NFFT)
    dx.free()
    dy.free()
    return got


@pytest.mark.parametrize("L", LENGTHS)
def test_small_shapes_vs_f64_oracle(ya, oracle, stream, L):
    rng = np.random.default_rng(1400 + L)
    h = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
    truth = spectra_truth(oracle, h, 0.4, stream)                  # causal: a prefix of the stream has a prefix of it
    want32 = oracle.stream_fir_fft(h, 0.4, stream, NFFT).reshape(6, NFFT)
    for nframes in (1, 2, 3):
        q = ya.FirFftStream(h)
        q.set_scale(0.4)
        q.set_variant(4)
        got = run_dev(ya, q, stream, [nframes, nframes])           # frame 0 of call 2: window from the object
        nf = 2 * nframes
        errs = [rel_l2(got[f], truth[f]) for f in range(nf)]
        e_all, e32 = rel_l2(got, truth[:nf]), rel_l2(want32[:nf], truth[:nf])
        print(f"L={L} nframes={nframes}: worst frame {max(errs):.3e}, all {e_all:.3e}, oracle f32 {e32:.3e}")
        for f in range(nf):
            assert errs[f] <= 1e-5, (nframes, f)
        assert e_all <= 3 * e32 + 1e-7, nframes


@pytest.mark.parametrize("piped", [False, True])
def test_scale_change_rebuilds_the_paired_tables(ya, oracle, stream, piped):
    """set_scale between two calls: the scaled tables (FFT{h} and the correction sum's, both in pairs) are rebuilt on the next
    call, on either entry path; the spectra after the change are those of the new scale, carried state included"""
    h = oracle.fir_design_kaiser(256, 0.2, 60.0)
    unit = spectra_truth(oracle, h, 1.0, stream)
    q = ya.FirFftStream(h)
    q.set_scale(0.4)
    q.set_variant(4)
    q.set_pipeline(piped)
    dx = ya.DeviceArray.from_numpy(np.ascontiguousarray(stream))
    dy = ya.DeviceArray(6 * NFFT, np.complex64)
    scales = [0.4, 0.4, 0.4, 0.25, 0.25, 0.25]
    for f in range(6):                                             # one frame per call; with set_pipeline the calls after
        if f == 3:                                                 # the first of each scale take the pipelined path
            q.set_scale(0.25)
        q.execute_dev(dx.ptr + 8 * NFFT * f, 1, dy.ptr + 8 * NFFT * f)
    q.join()
    ya.synchronize()
    got = dy.to_numpy().reshape(6, NFFT)
    for f in range(6):
        assert rel_l2(got[f], scales[f] * unit[f]) <= 1e-5, f
    dx.free()
    dy.free()


def test_pipelined_equals_plain_bit_for_bit(ya, oracle, stream):
    h = oracle.fir_design_kaiser(256, 0.2, 60.0)
    out = []
    for piped in (False, True):
        q = ya.FirFftStream(h)
        q.set_scale(0.4)
        q.set_variant(4)
        q.set_pipeline(piped)
        out.append(run_dev(ya, q, stream, [2, 2, 2]))
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
    truth = spectra_truth(oracle, h, 0.4, stream)
    for f in range(6):
        assert rel_l2(out[1][f], truth[f]) <= 1e-5, f


@pytest.mark.parametrize("L", [256, 257])
def test_integer_impulse_across_a_frame_boundary(ya, L):
    """all-ones taps, an impulse whose response straddles frames 0 and 1: the correction's slots are all in play"""
    h = np.ones(L, np.float32)
    x = np.zeros(3 * NFFT, np.complex64)
    x[NFFT - 100] = 1.0
    y = np.zeros(3 * NFFT)
    y[NFFT - 100: NFFT - 100 + L] = 1.0
    for sizes in ([3], [1, 2]):
        q = ya.FirFftStream(h)
        q.set_variant(4)
        got = run_dev(ya, q, x, sizes)
        for f in range(3):
            truth = np.fft.fft(y[f * NFFT:(f + 1) * NFFT])
            assert np.max(np.abs(got[f] - truth)) <= 2e-3, (sizes, f)
        assert np.max(np.abs(got[2])) == 0.0
