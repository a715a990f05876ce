"""Every FFT plan that serves a batch in passes over a fixed scratch buffer, driven across its pass seams, its consumers
at multi-pass batches, and the plan rule at its size limits and switch points.

The path and the chunk of every case are asserted through Fft.describe(), which reports what launch_fft_batch's own
dispatch and loops use: a tuning change that moves a size to another path or another chunk fails here instead of
silently emptying the case.  The batch arithmetic below takes the chunk from describe(), never from the table.

Truth is numpy's f64 FFT of the same f32 samples; rel_l2 <= 1e-5 is the project's FFT tolerance (test_gpu_fft.py).
The per-transform Parseval bound 2.1e-5 is what that tolerance implies for the energy: |y| within (1 +- 1e-5) |Y|
gives |y|^2 / |Y|^2 within 1 +- 2e-5 (+ 1e-10), and |Y|^2 = n |x|^2 exactly.  Random transforms differ in energy by
about 1 / sqrt(n) >= 1e-3 at every size here, so a misplaced, duplicated or unwritten transform fails it."""
import numpy as np
import pytest

from gpu_util import SEED, rand_taps, rel_l2

pytestmark = pytest.mark.gpu

SENTINEL = 0xFFFFFFFF               # memset 0xFF: a NaN bit pattern no transform of finite samples produces
PARSEVAL = 2.1e-5
FFT_TOL = 1e-5


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


# n, path, batch_chunk, (n1, n2) or None, bluestein m, nested (path, chunk) or None: the plan rule as it stands
PLANS = [
    (97, "bluestein", 32768, None, 256, ("one_kernel", 0)),
    (509, "bluestein", 8192, None, 1024, ("one_kernel", 0)),
    (1021, "bluestein", 4096, None, 2048, ("one_kernel", 0)),
    (8191, "bluestein", 512, None, 16384, ("two_pass", 1024)),
    (12289, "bluestein", 256, None, 32768, ("two_pass", 512)),
    (100003, "bluestein", 32, None, 1 << 18, ("tile256", 32)),
    (1 << 14, "two_pass", 1024, None, 0, None),
    (1 << 15, "two_pass", 512, None, 0, None),
    (1 << 16, "tile256", 128, (256, 256), 0, None),
    (1 << 17, "tile256", 64, (256, 512), 0, ("one_kernel", 0)),
    (1 << 20, "tile256", 8, (256, 4096), 0, ("one_kernel", 0)),
    (1 << 22, "tile256", 2, (256, 16384), 0, ("two_pass", 1024)),
    (10000, "mixed_two_pass", 1676, (100, 100), 0, None),
    (130321, "mixed_two_pass", 128, (361, 361), 0, None),
    (1000000, "mixed_two_pass", 16, (1000, 1000), 0, None),
    (1049600, "four_step", 7, (1024, 1025), 0, ("one_kernel", 0)),
    (3000000, "four_step", 2, None, 0, ("one_kernel", 0)),
]
PLAN_IDS = [str(p[0]) for p in PLANS]
ODD_OFFSET_SIZES = {97, 1 << 14, 1 << 16, 1 << 20, 10000, 1049600}      # one size per path (tile256: both row forms)


def check_plan(ya, info, n, path, chunk, split, m, nested):
    assert info.path == ya.FftPath[path], info
    assert info.batch_chunk == chunk, info
    assert info.bluestein_m == m, info
    if split is not None:
        assert (info.n1, info.n2) == split, info
    elif path in ("one_kernel", "bluestein_fused", "bluestein"):
        assert (info.n1, info.n2) == (0, 0), info             # no n1 x n2 split on these paths
    else:
        assert info.n1 * info.n2 == n, info
    if nested is None:
        assert info.nested is None, info
    else:
        assert info.nested is not None, info
        assert (info.nested.path, info.nested.batch_chunk) == (ya.FftPath[nested[0]], nested[1]), info
        assert info.nested.n == (m if m else info.n2), info


def memset_ff(ya, ptr, count):
    rc = ya.lib.yagi_hip_memset_dev(ptr, 0xFF, count * 8)
    assert rc == 0


def energies(a, batch, n):
    """sum |a|^2 of each of the batch transforms, accumulated in f64"""
    v = a.view(np.float32).reshape(batch, 2 * n)
    out = np.empty(batch)
    rows = max(1, (1 << 22) // (2 * n))
    for r0 in range(0, batch, rows):
        out[r0:r0 + rows] = np.square(v[r0:r0 + rows], dtype=np.float64).sum(axis=1)
    return out


def truth_f64(x, backward):
    x = x.astype(np.complex128)
    return np.fft.ifft(x) * len(x) if backward else np.fft.fft(x)


def bits(a):
    return a.view(np.uint64)


class Buffers:
    """buffers of `batch` transforms that start `off` elements into their allocations and have a guard of at least n
    points behind them, prefilled with the sentinel; with a seed, the input dx (device) / x (host) as well"""

    def __init__(self, ya, n, batch, off, seed=None):
        self.ya, self.n, self.batch, self.off = ya, n, batch, off
        self.total = batch * n
        self.size = off + self.total + n + 5
        if seed is not None:
            self.dx = self.out()
            ya.gen_complex_dev(seed, self.total, out=self.at(self.dx))
            self.x = self.dx.to_numpy(self.total, offset=off)

    def out(self):
        dy = self.ya.DeviceArray(self.size, np.complex64)
        memset_ff(self.ya, dy.ptr, self.size)
        return dy

    def at(self, d, transform=0):
        return d.ptr + 8 * (self.off + transform * self.n)

    def fetch(self, d):
        """the transforms of a buffer, after checking that nothing outside them was written and every point inside was"""
        self.ya.synchronize()
        a = d.to_numpy()
        u = a.view(np.uint32)
        lo, hi = 2 * self.off, 2 * (self.off + self.total)
        assert np.all(u[:lo] == SENTINEL), "wrote in front of the first transform"
        assert np.all(u[hi:] == SENTINEL), "wrote into the guard behind the last transform"
        y = a[self.off:self.off + self.total]
        assert not np.any(u[lo:hi] == SENTINEL), "a sentinel survived inside the output"
        assert np.all(np.isfinite(y.view(np.float32)))
        return y

    def free(self, *arrays):
        for d in arrays:
            d.free()


def run_seams(ya, n, direction, chunk, batch, off):
    """the checks of one (size, direction, batch): returns nothing, asserts everything"""
    backward = direction == "Backward"
    plan = ya.Fft(n, ya.Direction[direction])
    assert plan.describe().batch_chunk == chunk
    buf = Buffers(ya, n, batch, off, SEED + 40 + n % 97)
    dy = buf.out()
    plan.run_batch_dev(buf.at(buf.dx), buf.at(dy), batch)
    y = buf.fetch(dy)
    x = buf.x

    # per-transform Parseval, every transform
    e_in, e_out = energies(x, batch, n), energies(y, batch, n)
    ratio = np.abs(e_out / (n * e_in) - 1.0)
    worst = int(np.argmax(ratio))
    print(f"n={n} {direction} B={batch} chunk={chunk} off={off}: Parseval worst {ratio[worst]:.3e} at transform {worst}")
    assert ratio[worst] <= PARSEVAL, (worst, ratio[worst])

    # f64 truth on the transforms around every seam
    seams = sorted({b for b in (0, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, batch - 2, batch - 1)
                    if 0 <= b < batch})
    for b in seams:
        err = rel_l2(y[b * n:(b + 1) * n], truth_f64(x[b * n:(b + 1) * n], backward))
        assert err <= FFT_TOL, (b, err)

    if batch > chunk:
        # the same buffer by separate calls of at most one pass each
        dz = buf.out()
        calls = 0
        for b0 in range(0, batch, chunk):
            plan.run_batch_dev(buf.at(buf.dx, b0), buf.at(dz, b0), min(chunk, batch - b0))
            calls += 1
        assert calls == -(-batch // chunk)
        z = buf.fetch(dz)
        assert np.array_equal(bits(z), bits(y)), "multi-pass output differs from single-pass calls"
        buf.free(dz)
        del z

    if batch >= chunk + 2 and chunk >= 2:
        # four transforms across the first seam as a call of their own: another position in the batch, in the grid and
        # in the scratch.  Every path computes a transform with the same instruction sequence wherever it falls (no
        # kernel here has a separately compiled partial-workgroup variant), so the results are bit-identical.
        sub = Buffers(ya, n, 4, off)
        dw = sub.out()
        plan.run_batch_dev(buf.at(buf.dx, chunk - 2), sub.at(dw), 4)
        w = sub.fetch(dw)
        assert np.array_equal(bits(w), bits(y[(chunk - 2) * n:(chunk + 2) * n])), "result depends on the batch position"
        sub.free(dw)

    if batch == 2 * chunk + 3:
        # in place (the input buffer has the same guard)
        plan.run_batch_dev(buf.at(buf.dx), buf.at(buf.dx), batch)
        z = buf.fetch(buf.dx)
        assert np.array_equal(bits(z), bits(y)), "in-place output differs"
    buf.free(buf.dx, dy)


# ---- part A -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,path,chunk,split,m,nested", PLANS, ids=PLAN_IDS)
def test_plan_table(ya, n, path, chunk, split, m, nested):
    """the plan rule as the cases below rely on it, forward and backward"""
    for d in (ya.Direction.Forward, ya.Direction.Backward):
        check_plan(ya, ya.Fft(n, d).describe(), n, path, chunk, split, m, nested)


@pytest.mark.parametrize("passes", ["one", "one_plus_1", "two_plus_3"])
@pytest.mark.parametrize("direction", ["Forward", "Backward"])
@pytest.mark.parametrize("n,path,chunk,split,m,nested", PLANS, ids=PLAN_IDS)
def test_fft_batch_across_passes(ya, n, path, chunk, split, m, nested, direction, passes):
    """batches of chunk (the last transform of a full pass), chunk + 1 (a second pass of one transform) and
    2 chunk + 3 (two full passes and a ragged third): sentinel and guard, Parseval on every transform, f64 truth at the
    seams, bit-identity with single-pass calls, with a call at another batch position, and with the in-place run"""
    info = ya.Fft(n, ya.Direction[direction]).describe()
    check_plan(ya, info, n, path, chunk, split, m, nested)
    c = info.batch_chunk
    batch = {"one": c, "one_plus_1": c + 1, "two_plus_3": 2 * c + 3}[passes]
    if passes == "one":
        assert batch == c
    else:
        assert batch > c and batch % c != 0
    assert batch * n <= 36 << 20
    run_seams(ya, n, direction, c, batch, 0)


@pytest.mark.parametrize("direction", ["Forward", "Backward"])
@pytest.mark.parametrize("n,path,chunk,split,m,nested", [p for p in PLANS if p[0] in ODD_OFFSET_SIZES],
                         ids=[str(p[0]) for p in PLANS if p[0] in ODD_OFFSET_SIZES])
def test_fft_batch_across_passes_odd_offset(ya, n, path, chunk, split, m, nested, direction):
    """input and output three elements into their allocations: every transform starts on an 8-byte boundary only"""
    info = ya.Fft(n, ya.Direction[direction]).describe()
    check_plan(ya, info, n, path, chunk, split, m, nested)
    c = info.batch_chunk
    batch = 2 * c + 3
    assert batch > c and batch % c != 0
    run_seams(ya, n, direction, c, batch, 3)


# ---- part B: the consumers -----------------------------------------------------------------------------------------
def fftfilt_blocks(ya, oracle, n, L, nblocks, seam_blocks):
    """FftFilt.execute_blocks_dev over nblocks blocks: sampled blocks against the f64 direct form (tolerances of
    test_fftfilt_equals_direct_form), every block against FirFilter.execute_block_dev (test_fftfilt_large_batch_dev)"""
    rng = np.random.default_rng(n + L)
    h = rand_taps(rng, "crcf", L)
    total = n * nblocks
    dx = ya.gen_complex_dev(SEED + 41, total)
    dy = ya.DeviceArray(total, np.complex64)
    dz = ya.DeviceArray(total, np.complex64)
    q = ya.FftFilt("crcf", h, n)
    q.set_scale(0.5)
    q.execute_blocks_dev(dx, nblocks, dy)
    fir = ya.FirFilter("crcf", h)
    fir.set_scale(0.5)
    fir.execute_block_dev(dx, total, dz)
    ya.synchronize()
    x, y, z = dx.to_numpy(), dy.to_numpy(), dz.to_numpy()
    assert np.all(np.isfinite(y.view(np.float32)))
    for b in sorted(set(seam_blocks)):
        lo = max(0, b * n - (L - 1))                    # the block and the history its outputs reach into
        truth = oracle.fir_block_f64("crcf", h, x[lo:(b + 1) * n], scale=0.5)[b * n - lo:]
        got = y[b * n:(b + 1) * n]
        assert rel_l2(got, truth) <= 2e-6, b
        assert np.max(np.abs(got - truth)) <= 1e-5 * max(1.0, float(np.max(np.abs(truth)))), b
    d = (y.astype(np.complex128) - z).reshape(nblocks, n)
    err = np.linalg.norm(d, axis=1) / np.linalg.norm(z.reshape(nblocks, n).astype(np.complex128), axis=1)
    worst = int(np.argmax(err))
    print(f"fftfilt n={n} L={L} blocks={nblocks}: worst block {worst} rel_l2 {err[worst]:.3e}")
    assert err[worst] <= 2e-6, (worst, err[worst])
    for d_ in (dx, dy, dz):
        d_.free()


def test_fftfilt_blocks_across_two_pass_chunks(ya, oracle):
    """n = 8192 with 2050 taps (> 2049: the five-stage overlap-add form around the 2n-point plans): 2n = 2^14 is the
    two-launch form with 1024 transforms per pass; 2051 blocks = two full passes and a ragged third, forward and
    backward"""
    n, L = 8192, 2050
    for d in (ya.Direction.Forward, ya.Direction.Backward):
        info = ya.Fft(2 * n, d).describe()
        assert info.path == ya.FftPath.two_pass and info.batch_chunk == 1024, info
    c = info.batch_chunk
    nblocks = 2 * c + 3
    assert nblocks > 2048 and nblocks % c != 0
    fftfilt_blocks(ya, oracle, n, L, nblocks, (0, 1, c - 1, c, c + 1, 2 * c - 1, 2 * c, nblocks - 2, nblocks - 1))


def test_fftfilt_blocks_n509(ya, oracle):
    """n = 509, more than 8192 blocks.  A 2n = 1018-point plan would be Bluestein over m = 2048 with 4096 transforms per
    pass (asserted), but FftFilt never builds it at this block length: the filter is at most n + 1 = 510 taps, and up
    to 2049 taps the call goes to the one-launch overlap-save kernel (firfilt_fftconv_kernel), which has no batch
    loop.  The case stays as the check of that kernel at a block length that is no multiple of its 4096-point frames."""
    n, L = 509, 510
    info = ya.Fft(2 * n, ya.Direction.Forward).describe()
    assert info.path == ya.FftPath.bluestein and info.bluestein_m == 2048 and info.batch_chunk == 4096, info
    c = info.batch_chunk
    nblocks = 2 * c + 3
    assert nblocks > 8192 and nblocks % c != 0
    fftfilt_blocks(ya, oracle, n, L, nblocks, (0, 1, c - 1, c, c + 1, 2 * c - 1, 2 * c, nblocks - 2, nblocks - 1))


def test_spgram_16384_across_both_chunks(ya, oracle):
    """nfft = 16384 in one write_dev of 2100 transforms: run_frames cuts them at 2048 (2^25 / nfft), the plan serves
    those 2048 in two passes of 1024 and then the ragged 52"""
    nfft, wlen, delay = 16384, 16384, 1000
    info = ya.Fft(nfft, ya.Direction.Forward).describe()
    assert info.path == ya.FftPath.two_pass and info.batch_chunk == 1024, info
    frames_per_call = (1 << 25) // nfft
    assert frames_per_call == 2 * info.batch_chunk
    ntr = frames_per_call + 52
    n = ntr * delay + 77
    dx = ya.gen_complex_dev(SEED + 9, n)
    x = dx.to_numpy()
    q = ya.Spgram(nfft, ya.WindowType.Hann, wlen, delay)
    q.write_dev(dx, n)
    assert q.get_num_transforms() == ntr
    ref = oracle.Spgram(nfft, 2, wlen, delay)
    ref.write(x)
    assert ref.num_transforms == ntr
    a, b = q.get_psd_mag(), ref.get_psd_mag()
    err = np.linalg.norm(a - b) / np.linalg.norm(b)
    print(f"spgram nfft={nfft} transforms={ntr}: rel_l2 {err:.3e}")
    assert err <= 5e-5


def test_stream_8192_has_no_batch_loop(ya):
    """FirFftStream with nfft = 8192 hands its frames to the 8192-point plan, which is one launch whatever the batch:
    there is no pass seam to drive (the stream's own frame handling is test_gpu_stream.py's)"""
    info = ya.Fft(8192, ya.Direction.Forward).describe()
    assert info.path == ya.FftPath.one_kernel and info.batch_chunk == 0 and info.nested is None, info


# ---- part C: size limits and path switch points --------------------------------------------------------------------
def is_prime(v):
    if v < 2 or v % 2 == 0:
        return v == 2
    f = 3
    while f * f <= v:
        if v % f == 0:
            return False
        f += 2
    return True


def vs_f64(ya, n, batch):
    rng = np.random.default_rng(n)
    x = ((rng.standard_normal(batch * n) + 1j * rng.standard_normal(batch * n)) * np.sqrt(0.5)).astype(np.complex64)
    for direction in ("Forward", "Backward"):
        got = ya.Fft(n, ya.Direction[direction]).run_batch(x)
        for b in range(batch):
            err = rel_l2(got[b], truth_f64(x[b * n:(b + 1) * n], direction == "Backward"))
            print(f"n={n} {direction} transform {b}: rel_l2 {err:.3e}")
            assert err <= FFT_TOL, (direction, b, err)


LARGEST_PRIME = 8388593


@pytest.mark.parametrize("n,path,chunk,m,nested", [
    (1 << 23, "tile256", 1, 0, ("two_pass", 512)),
    (LARGEST_PRIME, "bluestein", 1, 1 << 24, ("tile256", 1)),
    ((1 << 23) - 1, "bluestein", 1, 1 << 24, ("tile256", 1)),                 # 47 x 178 481
], ids=["2^23", "largest_prime", "2^23-1"])
def test_fft_largest_sizes(ya, n, path, chunk, m, nested):
    """the largest sizes the plan rule accepts, at batch 2 (two passes of one transform; Bluestein over m = 2^24 runs
    its m-point transforms through nested tile256 passes)"""
    if n == LARGEST_PRIME:
        assert is_prime(n) and not any(is_prime(v) for v in range(n + 1, (1 << 23) + 1))
    for d in (ya.Direction.Forward, ya.Direction.Backward):
        check_plan(ya, ya.Fft(n, d).describe(), n, path, chunk, None, m, nested)
    vs_f64(ya, n, 2)


def test_fft_sizes_past_the_limit(ya):
    above = (1 << 23) + 1
    while not is_prime(above):
        above += 2
    for n in ((1 << 23) + 1, above):
        for d in (ya.Direction.Forward, ya.Direction.Backward):
            with pytest.raises(ya.ConfigError):
                ya.Fft(n, d)


SWITCHES = [
    (7921, "one_kernel", 0, None, 0, None),                                   # 89^2: the last direct-sum prime, twice
    (8188, "one_kernel", 0, None, 0, None),                                   # 4 x 23 x 89
    (8186, "bluestein", 512, None, 16384, ("two_pass", 1024)),                # 2 x 4093: the prime goes to Bluestein
    (8191, "bluestein", 512, None, 16384, ("two_pass", 1024)),
    (8192, "one_kernel", 0, None, 0, None),
    (8193, "bluestein", 256, None, 32768, ("two_pass", 512)),                 # 3 x 2731, and 2n - 1 > 16384
    (1024 * 1023, "mixed_two_pass", 16, (1023, 1024), 0, None),               # the factor limit of the two-launch form
    (1048575, "four_step", 8, (1025, 1023), 0, ("one_kernel", 0)),            # 1025 x 1023: just past it
    (1049600, "four_step", 7, (1024, 1025), 0, ("one_kernel", 0)),
    (1024 * 1024, "tile256", 8, (256, 4096), 0, ("one_kernel", 0)),
]


@pytest.mark.parametrize("n,path,chunk,split,m,nested", SWITCHES, ids=[str(p[0]) for p in SWITCHES])
def test_fft_path_switch_points(ya, n, path, chunk, split, m, nested):
    """the sizes on either side of each switch of the plan rule, forward and backward against f64"""
    for d in (ya.Direction.Forward, ya.Direction.Backward):
        check_plan(ya, ya.Fft(n, d).describe(), n, path, chunk, split, m, nested)
    vs_f64(ya, n, 2)
