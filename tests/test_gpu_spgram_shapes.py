"""Spgram on the GPU, frame by frame against f64, at every launch shape of tests/spgram_shapes.py.

A case is a row of the table, a sample type and a mode (accumulate, or recursive with the alpha of spgram_shapes).  It
first asserts that the library's plan query reports the row's key for the row's largest call, so the branch the case is
about is the branch that runs; then it drives a device object through the row's calls (write, write_dev on one device
copy of the stream, push, clear, reset, set_alpha) and compares get_psd_mag() with tests/spgram_ref.py.  The stream is
zero except for a burst that ends on each frame of interest (frame 0, the first frame since a clear, both frames at every
seam the row is about, the last full group, the last frame of every call), so one frame that is displaced by a sample,
dropped, counted twice or weighted as its neighbour moves the estimate by at least 10 TOL (test_spgram_ref_cpu.py
proves that for every case), and the all-zero frames in between cost the reference nothing.

Criteria per case
  per bin   max |gpu - truth| <= TOL max(truth)
  rel-L2    rel_l2(gpu, truth) <= RATIO rel_l2(model_f32, truth), and never above TOL; model_f32 is the pipeline rounded to
            f32 stage by stage in the reference's order
  counters  get_num_transforms / _total, get_num_samples / _total are the reference's
Each case prints one line: plan key, the GPU error, the model error, the ratio, the seconds it took.

The GPU adds in another association than the model (slab partials, the 32-to-1 fold, four partial sums, exp2f weights
against a running product), so the ratio had to be measured.  Worst per family on an MI355X: see WORST below; RATIO is
the next power of two at or above twice the worst.  Slowest case: see SLOWEST."""
import time

import numpy as np
import pytest

import spgram_ref as sr
import spgram_shapes as ss
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu

# Worst measured ratio per family (MI355X, 280 cases); the assertion is <= RATIO whatever these say.  The median ratio
# is 1.35 and nine cases in ten are below 2.3; the GPU's rel-L2 error is 5e-8 .. 2.2e-7 on the fused rows and up to
# 6.9e-7 on the unfused ones (64-cut+33 recursive), its worst bin 7.2e-7 of the largest: thirty times below TOL.
#   fused    7.422  512-wlen1 float32 accumulate: with one tap a frame is one sample, its transform is exact and the
#                   model errs by 1.7e-8 only; the GPU by 1.3e-7 like everywhere else
#   unfused  4.981  2-2acc+1 complex recursive: a 2-point transform, the model errs by 1.6e-8, the GPU by 7.8e-8
# The recursive 2^20-transform row has ratio 0.001: the model rounds psd 2^20 times in a row and drifts to 1.4e-4, the
# closed-form weights of the fused kernel stay at 9.1e-8.
WORST = {"fused": 7.422, "unfused": 4.981}
RATIO = 16.0
# Slowest case measured, reference and model included: 256-cut+37 complex recursive, 0.62 s (accumulate: 0.21 s); every
# other case takes at most 0.17 s.
SLOWEST = ("256-cut+37-cf-rec", 0.62)
TOL = ss.TOL


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


def make(ya, g, dt):
    return ya.Spgram(g.nfft, ya.WindowType(g.wtype), g.wlen, g.delay, dtype=dt)


def drive(ya, q, x, ops):
    """returns the device copy of the stream: the caller keeps it until the object has been read"""
    dx = ya.DeviceArray.from_numpy(x)
    pos = 0
    for op in ops:
        if op[0] in sr.WRITES:
            n = int(op[1])
            if op[0] == "write":
                q.write(x[pos:pos + n])
            elif op[0] == "write_dev":
                q.write_dev(dx.ptr + pos * x.itemsize, n)
            else:
                for v in x[pos:pos + n]:
                    q.push(v)
            pos += n
        elif op[0] == "set_alpha":
            q.set_alpha(op[1])
        else:
            getattr(q, op[0])()
    assert pos == len(x)
    return dx


def counters(q):
    return (q.get_num_samples(), q.get_num_samples_total(), q.get_num_transforms(), q.get_num_transforms_total())


CASES = ss.cases()


@pytest.mark.parametrize("row,dt,mode", CASES, ids=[ss.case_id(*c) for c in CASES])
def test_spgram_shape(ya, oracle, row, dt, mode):
    t0 = time.perf_counter()
    c = ss.build_case(ya, row, dt, mode)
    key = ss.key_of(ya.plan_spgram(row.nfft, c.main), c.main)
    assert key == row.key, (key, row)
    q = make(ya, c.g, dt)
    dx = drive(ya, q, c.x, c.ops)
    got = q.get_psd_mag()
    cnt = counters(q)
    dx.free()
    del q                                                # the 2^20-transform row holds about 512 MiB of scratch

    w = sr.taper(oracle, c.g)
    truth, s = sr.spgram_ref(c.g, w, c.x, c.ops, sched=c.sched)
    model = sr.model_f32(c.g, w, c.x, c.ops)
    e_gpu, e_model = rel_l2(got, truth), rel_l2(model, truth)
    e_bin = float(np.max(np.abs(got - truth)) / np.max(truth))
    ratio = e_gpu / e_model if e_model > 0 else (1.0 if e_gpu == 0 else np.inf)
    print(f"{ss.case_id(row, dt, mode)}: key {key} transforms {len(s.end)} alpha {c.alpha} rel-L2 vs f64 {e_gpu:.3e}, "
          f"model f32 {e_model:.3e}, ratio {ratio:.3f}, worst bin {e_bin:.3e}, {time.perf_counter() - t0:.2f} s")
    assert cnt == (s.num_samples, s.num_samples_total, s.num_transforms, s.num_transforms_total)
    assert np.max(truth) > 1e6 * float(sr.PSD_MIN) / max(1, s.num_transforms)        # far above the floor of get_psd_mag
    assert e_bin <= TOL
    assert e_gpu <= TOL
    assert e_gpu <= RATIO * e_model, (e_gpu, e_model)


@pytest.mark.parametrize("nfft", [512, 100])
@pytest.mark.parametrize("dt", [np.complex64, np.float32], ids=["cf", "f"])
def test_reset_replays_to_the_bits_of_a_fresh_object(ya, nfft, dt):
    g = sr.Geometry(nfft, 60, 7, ss.HAMMING)
    ops = [("write", 3), ("write_dev", 2 * nfft + 150), ("push", 2), ("write_dev", 333)]
    n = sum(op[1] for op in ops)
    x = sr.sparse_stream(dt, g, [0, 5, 40, n // 7 - 1], 77, n=n)
    y = sr.sparse_stream(dt, g, [1, 9, 30], 78, n=n)
    fresh, used = make(ya, g, dt), make(ya, g, dt)
    used.set_alpha(0.2)
    keep = [drive(ya, used, y, ops)]
    used.set_alpha(-1.0)                                   # reset keeps alpha; both objects replay in accumulate mode
    used.reset()
    assert counters(used) == (0, 0, 0, 0)
    keep += [drive(ya, used, x, ops), drive(ya, fresh, x, ops)]
    a, b = used.get_psd_mag(), fresh.get_psd_mag()
    assert counters(used) == counters(fresh) == (n, n, n // 7, n // 7)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.max(b) > 1e-6


@pytest.mark.parametrize("nfft", [512, 100])
def test_all_zero_stream_is_the_floor(ya, nfft):
    """every bin is f32(1e-12) * scale exactly, and get_psd its 10 log10 (to two units in the last place of f32 at 140:
    log10f is the device's)"""
    g = sr.Geometry(nfft, 60, 7, ss.HAMMING)
    n = 2 * nfft + 100
    q = make(ya, g, np.complex64)
    dx = drive(ya, q, np.zeros(n, np.complex64), [("write", 10), ("write_dev", n - 10)])
    nt = n // 7
    assert q.get_num_transforms() == nt
    want = sr.PSD_MIN * (np.float32(1.0) / np.float32(nt))
    mag = q.get_psd_mag()
    assert mag.dtype == np.float32 and np.all(mag == want), (mag[:4], want)
    assert np.max(np.abs(q.get_psd() - 10.0 * np.log10(np.float64(want)))) <= 3.1e-5
    q.set_alpha(0.5)                                       # while averaging the linear scale is 0
    assert np.all(q.get_psd_mag() == 0)
    dx.free()
