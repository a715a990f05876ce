"""The prototype constructors (firinterp.rs:105-124, firdecim.rs:102-121, firfilt.rs:112-116) are the design followed by
the plain constructor: an object made by new_prototype / new_rnyquist and one made from fir_design_prototype's taps by
hand give the same bytes.  For the interpolator an impulse shows the taps themselves: output n k + i of a unit sample is
h[i + n k] exactly, and against the same object made by hand the outputs are equal byte for byte."""
import numpy as np
import pytest

from gpu_util import rand_samples

pytestmark = pytest.mark.gpu
CASES = [("Rrcos", 2, 3, 0.3, 0.0), ("Arkaiser", 5, 7, 0.25, 0.25), ("Rcos", 8, 4, 1.0, 0.0), ("Kaiser", 3, 12, 0.2, -0.25)]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


@pytest.mark.parametrize("shape,k,m,beta,dt", CASES)
def test_firinterp_new_prototype_taps_are_the_design_s_bytes(ya, shape, k, m, beta, dt):
    F = ya.FirFilterShape[shape]
    h = ya.fir_design_prototype(F, k, m, beta, dt)
    for kind in ("rrrf", "crcf", "cccf"):
        q = ya.FirInterpolationFilter.new_prototype(kind, F, k, m, beta, dt)
        assert q.get_interp_rate() == k and q.get_sub_len() == 2 * m + 1
        x = np.zeros(2 * m + 1, q.T)
        x[0] = 1
        y = q.execute_block(x)
        assert np.array_equal(np.real(y[:h.size]).astype(np.float32), h), kind      # == : a tap of -0.0 comes out as +0.0
        assert not np.any(np.imag(y)) and not np.any(y[h.size:])
        x = rand_samples(np.random.default_rng(k + m), kind, 300)
        q.reset()
        assert q.execute_block(x).tobytes() == ya.FirInterpolationFilter(kind, k, h.astype(q.Cdt)).execute_block(x).tobytes()


@pytest.mark.parametrize("shape,k,m,beta,dt", CASES)
def test_firdecim_new_prototype_and_firfilt_new_rnyquist(ya, shape, k, m, beta, dt):
    F = ya.FirFilterShape[shape]
    h = ya.fir_design_prototype(F, k, m, beta, dt)
    for kind in ("rrrf", "crcf", "cccf"):
        x = rand_samples(np.random.default_rng(k + m), kind, 600 * k)
        q = ya.FirDecimationFilter.new_prototype(kind, F, k, m, beta, dt)
        ref = ya.FirDecimationFilter(kind, k, h.astype(q.Cdt))
        assert q.get_decim_rate() == k
        assert q.execute_block(x, 600).tobytes() == ref.execute_block(x, 600).tobytes(), kind
        f = ya.FirFilter.new_rnyquist(kind, F, k, m, beta, dt)
        assert f.get_length() == h.size
        assert np.real(f.get_coefficients()).astype(np.float32).tobytes() == h.tobytes(), kind
