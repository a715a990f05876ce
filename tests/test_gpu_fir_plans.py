"""Every launch plan of the FIR family on the GPU against a reference, at the shapes of tests/fir_shapes.py.

A case is a row of the table and a sample type.  It first asserts that the library's plan query reports the row's key on
this machine, so the kernel the case is about is the kernel that runs, then:

  fir      FirFilter (kernel 1) for M = 1, FirDecimationFilter for M >= 2: one stream at scale 0.5 cut into calls of 512,
           T + 1, (ceil((L - 1) / (T M)) + 3) T + 7, 511 and T outputs (T = the plan's outputs per workgroup), through the
           host call and the _dev call.  Every element within gpu_util.fir_bound of oracle.fir_block_f64; rel-L2 error
           against f64 at most twice that of the oracle's sequential f32 object on the same data (the register-window
           decimators add phase by phase, the same products in another order); integer data equal to the oracle bit for
           bit; the long call again on guarded, poisoned arenas at element offsets 0 and 1.  Complex rows with M >= 2
           whose plan stages a span also run Ddc's fused kernel (NCO and VCO) word for word against Osc +
           FirDecimationFilter, which the checks before it pin to f64.
  pfb      FirPfbFilter.execute_all, FirInterpolationFilter (host and _dev call) and, for complex samples, Duc: calls of
           1, 63, 64, 65, 255, 256, 257 and 773 inputs on one stream, the same two criteria per branch against
           oracle.FirPfbFilter and the f64 sum.
  rresamp  integer data, calls of 1, tb - 1, tb + 1 and 3 tb + 2 blocks, bit for bit against oracle.Rresamp.
  resamp   integer data, calls worth 1, tile - 1, tile + 1 and 3 tile + 2 outputs, bit for bit against
           resamp_util.RefResamp.
  none     the call raises ConfigError and leaves the object as it was: its next valid call gives a twin's bits.  A
           Resamp of such a shape is refused when it is created, and a FirInterpolationFilter or Rresamp of one has no
           valid block call at all: there the refused call is repeated and the object's host calls still work.

Each case prints one line with its plan key and the measured ratio (rel-L2 error of the GPU over that of the oracle's f32
object).  Worst ratio measured on an MI355X: see WORST below."""
import numpy as np
import pytest

import fir_shapes as fs
from dev_arena import GUARD_MIN, Arena
from gpu_util import fir_bound, int_samples, int_taps, rand_samples, rand_taps, rel_l2
from resamp_util import RefResamp

pytestmark = pytest.mark.gpu

# Worst measured ratio per family (MI355X, 168 cases with a ratio); the assertion is <= RATIO whatever these say.
#   fir  1.695  cccf consec (M 1, L 3405); complex taps are near 1.4 .. 1.7 wherever an output sums more than a few
#               taps: mac(cf32, cf32, cf32) rounds the accumulator twice per tap, the oracle adds a finished product
#               once.  Real taps 0.84 .. 1.20, but 1.435 (rrrf) / 1.400 (crcf) at staged (M 2, L 15)
#   pfb  1.447  cccf taps_global (nf 2, Ls 5890); real taps 0.80 .. 1.02
WORST = {"fir": 1.695, "pfb": 1.447}
RATIO = 2.0
SCALE = 0.5
PFB_CALLS = [1, 63, 64, 65, 255, 256, 257, 3 * 256 + 5]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


def params(family):
    cs = fs.cases(family)
    return pytest.mark.parametrize("row,kind", cs, ids=[fs.case_id(r, k) for r, k in cs])


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_key(ya, row, kind):
    key, plan = fs.query(ya, row, kind)
    assert key == row.key, (key, row)
    return plan


def accuracy(tag, got, ref32, truth, bound):
    """the two criteria of the module docstring; returns the ratio"""
    assert np.all(np.abs(got - truth) <= bound), (tag, float(np.max(np.abs(got - truth))), float(np.max(bound)))
    e_gpu, e_ref = rel_l2(got, truth), rel_l2(ref32, truth)
    ratio = e_gpu / e_ref if e_ref > 0 else (1.0 if e_gpu == 0 else np.inf)
    print(f"{tag}: rel-L2 vs f64 {e_gpu:.3e}, oracle f32 {e_ref:.3e}, ratio {ratio:.3f}")
    assert e_gpu <= RATIO * e_ref, (tag, e_gpu, e_ref)
    return ratio


# ---- launch_fir_block ------------------------------------------------------------------------------------------------
def make_fir(mod, kind, M, h):
    if M == 1:
        q = mod.FirFilter(kind, h)
        if hasattr(q, "set_kernel"):
            q.set_kernel(1)                          # the general direct forms: launch_fir_block
    else:
        q = mod.FirDecimationFilter(kind, M, h)
    q.set_scale(SCALE)
    return q


def run_fir(q, M, x, n):
    return q.execute_block(x) if M == 1 else q.execute_block(x, n)


def fir_cuts(T, L, M):
    long = (-(-(L - 1) // (T * M)) + 3) * T + 7
    return np.cumsum([0, 512, T + 1, long, 511, T])


def run_fir_dev(ya, q, M, x, cuts):
    dx, dy = ya.DeviceArray.from_numpy(x), ya.DeviceArray(int(cuts[-1]), x.dtype)
    for a, b in zip(cuts[:-1], cuts[1:]):
        q.execute_block_dev(dx.ptr + int(a) * M * x.itemsize, int(b - a), dy.ptr + int(a) * x.itemsize)
    ya.synchronize()
    return dy.to_numpy()


@params("fir")
def test_fir_block_plan(ya, oracle, row, kind):
    M, L, ny = row.shape
    plan = check_key(ya, row, kind)
    elem = fs.ELEM[kind][0]
    T = plan.tile
    cuts = fir_cuts(T, L, M)
    n = int(cuts[-1])
    # what each call of the stream runs: the 512-output call and the long one run the row's plan, the 511-output call a
    # general kernel (the window passes from one kernel to the other)
    ran = [fs.fir_key(ya.plan_fir_block(elem, L, M, int(b - a))) for a, b in zip(cuts[:-1], cuts[1:])]
    assert ran[0] == row.key and ran[2] == row.key and ran[3][0] in ("staged", "unstaged"), ran
    tag = fs.case_id(row, kind)
    rng = np.random.default_rng(7000 + 131 * M + L)
    h, x = rand_taps(rng, kind, L), rand_samples(rng, kind, n * M)

    q = make_fir(ya, kind, M, h)
    got = np.concatenate([run_fir(q, M, x[a * M:b * M], int(b - a)) for a, b in zip(cuts[:-1], cuts[1:])])
    truth = oracle.fir_block_f64(kind, h, x, M=M, n=n, scale=SCALE)
    ref32 = run_fir(make_fir(oracle, kind, M, h), M, x, n)
    accuracy(f"{tag} key {row.key} T {T} n {n}", got, ref32, truth, fir_bound(kind, h, x))
    got_dev = run_fir_dev(ya, make_fir(ya, kind, M, h), M, x, cuts)
    assert np.array_equal(words(got_dev), words(got)), int(np.flatnonzero(words(got_dev) != words(got))[0])

    # integers: every product and partial sum is exact, so the cuts, the tiles and the window hand-over show bit for bit
    hi, xi = int_taps(rng, kind, L), int_samples(rng, kind, n * M)
    qi = make_fir(ya, kind, M, hi)
    goti = np.concatenate([run_fir(qi, M, xi[a * M:b * M], int(b - a)) for a, b in zip(cuts[:-1], cuts[1:])])
    wanti = run_fir(make_fir(oracle, kind, M, hi), M, xi, n)
    assert np.array_equal(goti, wanti), int(np.flatnonzero(goti != wanti)[0])

    # the long call on arenas: its first tile reads the carried window, its last is ragged
    a, b = int(cuts[2]), int(cuts[3])
    qa = make_fir(ya, kind, M, h)
    run_fir(qa, M, x[:cuts[1] * M], int(cuts[1]))
    run_fir(qa, M, x[cuts[1] * M:a * M], a - int(cuts[1]))
    guard = GUARD_MIN + L + T * M
    for off in (0, 1):
        c = qa.clone()
        xa = Arena(ya, x.dtype, (b - a) * M, off, guard).load(x[a * M:b * M])
        yb = Arena(ya, x.dtype, b - a, off, guard)
        c.execute_block_dev(xa.ptr, b - a, yb.ptr)
        y = yb.fetch_output()
        xa.assert_input_intact(x[a * M:b * M])
        assert np.array_equal(words(y), words(got[a:b])), (off, int(np.flatnonzero(words(y) != words(got[a:b]))[0]))
        xa.free()
        yb.free()

    # Ddc: the same bodies with the oscillator mixed in on the way into LDS
    if kind != "rrrf" and M >= 2 and row.key[0] in ("decim", "staged"):
        for scheme in (0, 1):
            d, osc, fir = ya.Ddc(kind, scheme, M, h), ya.Osc(scheme), ya.FirDecimationFilter(kind, M, h)
            d.set_scale(SCALE)
            fir.set_scale(SCALE)
            d.set_kernel(2)
            for o in (d, osc):
                o.set_phase(6.2831)
                o.set_frequency(0.3713)
            for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                seg = x[a * M:b * M]
                y = d.execute_block(seg, int(b - a))
                want = fir.execute_block(osc.mix_block_down(seg), int(b - a))
                assert d.get_last_kernel() == (1 if ran[i][0] == "unstaged" else 2), (scheme, i, ran[i])
                assert np.array_equal(words(y), words(want)), (scheme, i, int(np.flatnonzero(words(y) != words(want))[0]))
            assert d.get_state() == osc.get_state()


# ---- launch_firpfb_all -----------------------------------------------------------------------------------------------
def duc_pair(ya, kind, scheme, nf, h):
    d, osc, fir = ya.Duc(kind, scheme, nf, h), ya.Osc(scheme), ya.FirInterpolationFilter(kind, nf, h)
    d.set_scale(SCALE)
    fir.set_scale(SCALE)
    d.set_kernel(2)
    for o in (d, osc):
        o.set_phase(6.2831)
        o.set_frequency(0.3713)
    return d, osc, fir


@params("pfb")
def test_firpfb_all_plan(ya, oracle, row, kind):
    nf, Ls = row.shape
    check_key(ya, row, kind)
    tag = fs.case_id(row, kind)
    cuts = np.cumsum([0] + PFB_CALLS)
    n = int(cuts[-1])
    rng = np.random.default_rng(7100 + 131 * nf + Ls)
    h, x = rand_taps(rng, kind, nf * Ls), rand_samples(rng, kind, n)
    pfb = ya.FirPfbFilter(kind, nf, h)
    pfb.set_scale(SCALE)
    interp = ya.FirInterpolationFilter(kind, nf, h)
    interp.set_scale(SCALE)

    if row.key[1] == "none":
        twin = ya.FirPfbFilter(kind, nf, h)
        twin.set_scale(SCALE)
        first = [o.execute_block(0, x[:700]) for o in (pfb, twin)]
        assert np.array_equal(words(first[0]), words(first[1]))
        with pytest.raises(ya.ConfigError, match="too long"):
            pfb.execute_all(x[700:900])
        a, b = pfb.execute_block(1, x[700:1500]), twin.execute_block(1, x[700:1500])
        assert np.array_equal(words(a), words(b))
        truth = oracle.fir_block_f64(kind, h[1::nf], x[:1500], scale=SCALE)[700:]
        assert np.all(np.abs(a - truth) <= fir_bound(kind, h[1::nf], x))
        for _ in range(2):                           # no block call of the interpolator fits: refused, and again
            with pytest.raises(ya.ConfigError, match="too long"):
                interp.execute_block(x[:64])
        interp.reset()
        if kind != "rrrf":
            d, _, _ = duc_pair(ya, kind, 0, nf, h)
            before = d.get_state()
            with pytest.raises(ya.ConfigError, match="too long"):
                d.execute_block(x[:64])
            assert d.get_state() == before
        print(f"{tag}: key {row.key} refused, the object's next call equals its twin's")
        return

    got = np.concatenate([pfb.execute_all(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])          # [n, nf]
    goti = np.concatenate([interp.execute_block(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]).reshape(n, nf)
    assert np.array_equal(words(goti), words(got))
    idev = ya.FirInterpolationFilter(kind, nf, h)
    idev.set_scale(SCALE)
    dx, dy = ya.DeviceArray.from_numpy(x), ya.DeviceArray(n * nf, x.dtype)
    for a, b in zip(cuts[:-1], cuts[1:]):
        idev.execute_block_dev(dx.ptr + int(a) * x.itemsize, int(b - a), dy.ptr + int(a) * nf * x.itemsize)
    ya.synchronize()
    assert np.array_equal(words(dy.to_numpy().reshape(n, nf)), words(got))

    ref = oracle.FirPfbFilter(kind, nf, h, nf * Ls)
    ref.set_scale(SCALE)
    ref32, truth, bound = np.empty_like(got), np.empty(got.shape, np.result_type(x.dtype, np.float64)), np.empty(nf)
    for i in range(nf):
        ref.reset()
        ref32[:, i] = ref.execute_block(i, x)
        truth[:, i] = oracle.fir_block_f64(kind, h[i::nf], x, scale=SCALE)
        bound[i] = fir_bound(kind, h[i::nf], x)
    accuracy(f"{tag} key {row.key}", got, ref32, truth, bound[None, :])

    if kind != "rrrf":
        for scheme in (0, 1):
            d, osc, fir = duc_pair(ya, kind, scheme, nf, h)
            for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                y = d.execute_block(x[a:b])
                want = osc.mix_block_up(fir.execute_block(x[a:b]))
                assert d.get_last_kernel() == 2, (scheme, i)
                assert np.array_equal(words(y), words(want)), (scheme, i, int(np.flatnonzero(words(y) != words(want))[0]))
            assert d.get_state() == osc.get_state()


# ---- launch_rresamp --------------------------------------------------------------------------------------------------
@params("rresamp")
def test_rresamp_plan(ya, oracle, row, kind):
    P, Q, Ls = row.shape
    plan = check_key(ya, row, kind)
    tag = fs.case_id(row, kind)
    m = Ls // 2
    rng = np.random.default_rng(7200 + 131 * P + 17 * Q + Ls)
    h = int_taps(rng, kind, 2 * P * m)
    q = ya.Rresamp(kind, P, Q, m, h)
    if row.key[1] == "none":
        x = int_samples(rng, kind, 2 * Q)
        for _ in range(2):                           # no block call of this object fits: refused, and again
            with pytest.raises(ya.ConfigError, match="do not fit"):
                q.execute_block(x, 2)
        q.write(x[:Q])
        q.reset()
        print(f"{tag}: key {row.key} refused")
        return
    tb = plan.tile
    cuts = np.cumsum([0] + [c for c in (1, tb - 1, tb + 1, 3 * tb + 2) if c > 0])
    nb = int(cuts[-1])
    x = int_samples(rng, kind, nb * Q)
    got = np.concatenate([q.execute_block(x[a * Q:b * Q], int(b - a)) for a, b in zip(cuts[:-1], cuts[1:])])
    want = oracle.Rresamp(kind, P, Q, m, h).execute_block(x, nb)
    assert got.shape == want.shape and np.array_equal(got, want), int(np.flatnonzero(got != want)[0])
    print(f"{tag}: key {row.key} tb {tb}, {nb} blocks equal the oracle bit for bit")


# ---- launch_resamp ---------------------------------------------------------------------------------------------------
def resamp_dev(ya, q, x):
    """through the kernel whatever the length (the host call runs up to 32 inputs on the host mirror)"""
    ny = q.get_num_output(len(x))
    dx, dy = ya.DeviceArray.from_numpy(x), ya.DeviceArray(max(ny, 1), x.dtype)
    nw = q.execute_block_dev(dx, len(x), dy, max(ny, 1))
    ya.synchronize()
    assert nw == ny
    return dy.to_numpy(ny)


@params("resamp")
def test_resamp_plan(ya, oracle, row, kind):
    rate, Ls = row.shape
    plan = check_key(ya, row, kind)
    tag = fs.case_id(row, kind)
    m, npfb = Ls // 2, 4
    rng = np.random.default_rng(7300 + Ls + int(1000 * rate))
    h = int_taps(rng, kind, 2 * m * npfb)
    if row.key[1] == "none":
        # Resamp checks the same bound when it is created (2 m + 1 samples in 48 KiB), so the launch never sees the shape
        with pytest.raises(ya.ConfigError, match="too large"):
            ya.Resamp.from_taps(kind, rate, m, npfb, h)
        print(f"{tag}: key {row.key} refused at creation")
        return
    tile = plan.tile
    q = ya.Resamp.from_taps(kind, rate, m, npfb, h)
    assert q.get_delay() == m
    nxs = [max(1, int(np.ceil(t / rate))) for t in (1, tile - 1, tile + 1, 3 * tile + 2) if t > 0]
    cuts = np.cumsum([0] + nxs)
    x = int_samples(rng, kind, int(cuts[-1]))
    got = np.concatenate([resamp_dev(ya, q, x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    want = RefResamp(oracle, kind, rate, m, npfb, h).execute_block(x)
    assert got.shape == want.shape and np.array_equal(got, want), int(np.flatnonzero(got != want)[0])
    assert len(got) > 3 * tile
    print(f"{tag}: key {row.key} tile {tile}, {len(got)} outputs equal the reference loop bit for bit")
