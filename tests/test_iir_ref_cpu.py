"""CPU checks of the IirFilter references (tests/iir_ref.py) and of the IirFilter boundary without a GPU.

(a) the f32 restatement reproduces the reference's nine golden sets (iirfilt.rs:806-986, tolerance 1e-3); (b) the
chunk-vectorised f64 reference equals (c) the plain f64 loop; (b) agrees with scipy where it is installed."""
from pathlib import Path

import numpy as np
import pytest

from conftest import has_gpu
from iir_ref import Seq32, iir64, iir64_loop

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "iirfilt.npz")
KINDS = ["rrrf", "crcf", "cccf"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h", [3, 5, 7])
def test_restatement_matches_golden(kind, h):
    b, a, x, y = (GOLD[f"{kind}_h{h}_{p}"] for p in "baxy")
    got = Seq32(kind, b, a).execute_block(x)
    np.testing.assert_allclose(got, y, rtol=1e-3, atol=1e-3)


def test_restatement_sos_impulse_step():
    for t in ("impulse", "step"):
        b, a, want = GOLD[f"sos_{t}_b"], GOLD[f"sos_{t}_a"], GOLD[f"sos_{t}_y"]
        x = np.zeros(15, np.float32)
        x[: 1 if t == "impulse" else 15] = 1.0
        np.testing.assert_allclose(Seq32("rrrf", b, a, nsos=1).execute_block(x), want, atol=1e-4)


def test_restatement_head_split_and_clone():
    """n = 3: the deque's head walks 0, 2, 1, 0, ...; a clone restarts at head 0 with the same logical state"""
    b, a = GOLD["rrrf_h3_b"], GOLD["rrrf_h3_a"]
    q = Seq32("rrrf", b, a)
    heads = []
    for v in GOLD["rrrf_h3_x"][:6]:
        q.execute(v)
        heads.append(q.head)
    assert heads == [2, 1, 0, 2, 1, 0]
    c = q.clone()
    q.execute(1.0)
    assert c.head == 0
    y0 = [q.execute(v) for v in GOLD["rrrf_h3_x"]]
    y1 = [c.execute(v) for v in np.concatenate([[1.0], GOLD["rrrf_h3_x"]])][1:]
    np.testing.assert_allclose(y0, y1, rtol=1e-5)


def _rand(rng, kind, n):
    if kind == "rrrf":
        return rng.standard_normal(n)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", list(range(0, 33)))
def test_f64_chunked_equals_loop_tf(kind, S):
    rng = np.random.default_rng(S)
    n = S + 1
    # sum |a[1:]| = 0.9 < 1: stable whatever the f32 rounding of the normalised coefficients (Rouche)
    a = np.concatenate([[1.0], _rand(rng, "cccf" if kind == "cccf" else "rrrf", S)])
    if S:
        a[1:] *= 0.9 / np.sum(np.abs(a[1:]))
    b = _rand(rng, "cccf" if kind == "cccf" else "rrrf", n) * 0.1
    x = _rand(rng, kind, 997)
    y_loop = iir64_loop(kind, b, a, x)
    for chunk in (1, 7, 64, 997, 2000):
        y = iir64(kind, b, a, x, chunk=chunk)
        assert np.linalg.norm(y - y_loop) <= 1e-12 * np.linalg.norm(y_loop), chunk


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nsos", [1, 2, 5, 16])
def test_f64_chunked_equals_loop_sos(kind, nsos):
    rng = np.random.default_rng(nsos)
    b = _rand(rng, "cccf" if kind == "cccf" else "rrrf", 3 * nsos) * 0.3
    a = np.tile([1.0, -0.5, 0.3], nsos) + 0.05 * _rand(rng, "cccf" if kind == "cccf" else "rrrf", 3 * nsos)
    a[::3] = 1.0
    x = _rand(rng, kind, 1001)
    y_loop = iir64_loop(kind, b, a, x, nsos=nsos)
    for chunk in (3, 64, 1001):
        y = iir64(kind, b, a, x, nsos=nsos, chunk=chunk)
        assert np.linalg.norm(y - y_loop) <= 1e-12 * np.linalg.norm(y_loop)


def test_f64_against_scipy():
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(3)
    b, a = GOLD["rrrf_h7_b"], GOLD["rrrf_h7_a"]
    x = rng.standard_normal(5000)
    bn, an = (np.float32(b) / np.float32(a[0])).astype(np.float64), (np.float32(a) / np.float32(a[0])).astype(np.float64)
    np.testing.assert_allclose(iir64("rrrf", b, a, x, chunk=128), sig.lfilter(bn, an, x), rtol=1e-9, atol=1e-12)
    sb = np.array([0.2, 0.4, 0.2, 1.0, -0.3, 0.5], np.float32)
    sa = np.array([1.0, -0.6, 0.2, 1.0, 0.1, 0.4], np.float32)
    sos = np.concatenate([sb.reshape(2, 3), sa.reshape(2, 3)], axis=1).astype(np.float64)
    np.testing.assert_allclose(iir64("rrrf", sb, sa, x, nsos=2, chunk=100), sig.sosfilt(sos, x), rtol=1e-9, atol=1e-12)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_iirfilter_without_gpu_is_a_device_error():
    import yagi_amd as ya
    b, a = GOLD["crcf_h3_b"], GOLD["crcf_h3_a"]
    for make in (lambda k: ya.IirFilter(k, b, a),
                 lambda k: ya.IirFilter.new_sos(k, np.ones(3), np.ones(3), 1),
                 lambda k: ya.IirFilter.new_dc_blocker(k, 0.2),
                 lambda k: ya.IirFilter.new_integrator(k),
                 lambda k: ya.IirFilter.new_differentiator(k),
                 lambda k: ya.IirFilter.new_pll(k, 0.1, 0.7, 1000.0)):
        for kind in KINDS:
            with pytest.raises(ya.DeviceError):
                make(kind)
