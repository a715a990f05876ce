"""Every device-pointer (`_dev`) entry point on offset, guarded, poisoned buffers (tests/dev_arena.py).

One registry, ROWS; one procedure for every row and every offset pair (ox, oy), in elements of each operand's type:

  * every operand lives in an Arena: an allocation filled with 0xFF bytes, the operand `guard + off` elements in;
  * a fresh object runs three calls that continue one stream: the row's long call (at least two of the kernel's tiles
    and a ragged tail of 1, 2 or 3 mod 4 elements wherever the entry point's units allow one), then 1 unit, then 5 --
    so the carried window / state is read back in through offset pointers too;
  * 1. each output arena passes fetch_output(): guards intact, no sentinel left inside, everything finite;
    2. each input arena passes assert_input_intact();
    3. the concatenated output meets the reference of the object's own test file at that file's tolerance;
    4. the output is bit-identical to the (0, 0) run of the same row.

What this does not catch: an out-of-range READ whose value is discarded (a masked lane, a halo fetched and never
used).  Such a read leaves nothing in memory to read back, and the buffers are deliberately placed in the middle of
their allocations so that it cannot fault either.  A read that is USED shows up as a NaN (points 1 and 3).

Entry points without a row are listed in EXCLUDED with the reason; tests/test_dev_arena_cpu.py checks, without a GPU,
that ROWS and EXCLUDED together cover every `_dev` method of the package."""
import numpy as np
import pytest

from dev_arena import GUARD_MIN, Arena
from gpu_util import SEED, int_samples, int_taps, rand_samples, rand_taps, rel_l2

pytestmark = pytest.mark.gpu

KINDS = ["rrrf", "crcf", "cccf"]
FFT_TOL = 1e-5                       # test_gpu_fft.py / test_gpu_fft_batches.py
F32, C64, U32 = np.dtype(np.float32), np.dtype(np.complex64), np.dtype(np.uint32)

EXCLUDED = {
    "FirPfbCh2.analyzer_execute_sharded_dev": "needs RCCL peers (a communicator); covered by test_gpu_chan.py / test_gpu_dist2.py",
}


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


def T(kind):
    return F32 if kind == "rrrf" else C64


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def check_equal(got, want):
    """every element equal to the reference's (numpy.array_equal, as the objects' own integer-data tests compare)"""
    want = np.ascontiguousarray(want).astype(got.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} elements differ from the reference, first at {int(bad[0])}"


class Row:
    """id            test id;  entry  'Class.method' (or the module function) the row drives
    make(ya, oracle) a fresh object (None for the plain functions)
    ins              [(dtype, elements per unit)] of the inputs;  out  (dtype, elements per unit) or None
    gen(oracle, units) the host inputs of the whole stream, one array per input
    call(q, in_ptrs, n, out_ptr, cap) one device call of n units; returns the count written for counted rows
    want(ya, oracle, xs, calls) the reference output of the whole stream
    check(got, want) point 3;  big  units of the long call;  cite  where the tile size was read
    cap(q, n)        elements of capacity of the output of a call of n units (default n * out per unit)
    counted          the call reports how many elements it wrote (Resamp, MsResamp): the rest must stay sentinel
    result(q)        rows with no output operand: what to compare instead (Spgram: the PSD)"""

    def __init__(self, id, entry, make, ins, out, gen, call, want, big, cite, check=check_equal, cap=None,
                 counted=False, result=None, pairs=None, guard=GUARD_MIN, tail=(1, 5)):
        self.id, self.entry, self.make, self.ins, self.out = id, entry, make, ins, out
        self.gen, self.call, self.want, self.big, self.cite, self.check = gen, call, want, big, cite, check
        self.cap, self.counted, self.result, self.pairs, self.guard = cap, counted, result, pairs, guard
        self.calls = (big,) + tuple(tail)

    def offset_pairs(self):
        if self.pairs is not None:
            return self.pairs
        if self.out is None:                                 # no output operand: the output offset moves nothing
            return [(0, 0), (1, 0)]
        if not self.ins:                                     # no input operand: every output offset of the type
            return [(0, 0), (0, 1)] + ([(0, 2), (0, 3)] if self.out[0] == F32 else [])
        p = [(0, 0), (1, 0), (0, 1), (1, 1)]
        dts = [d for d, _ in self.ins] + ([self.out[0]] if self.out else [])
        return p + ([(3, 2)] if F32 in dts else [])


_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def run_row(ya, oracle, row, ox, oy):
    """the three calls of one row at one offset pair: points 1 and 2 asserted here, the whole output returned"""
    q = row.make(ya, oracle)
    xs = cached((row.id, "x"), lambda: row.gen(oracle, sum(row.calls)))
    outs, pos = [], 0
    for n in row.calls:
        ins = []
        for (dt, per), x in zip(row.ins, xs):
            seg = np.ascontiguousarray(x[pos * per:(pos + n) * per], dt)
            ins.append((Arena(ya, dt, seg.size, ox, row.guard).load(seg), seg))
        yo = cap = None
        if row.out is not None:
            cap = row.cap(q, n) if row.cap else n * row.out[1]
            yo = Arena(ya, row.out[0], cap, oy, row.guard)
        nw = row.call(q, [a.ptr for a, _ in ins], n, yo.ptr if yo else None, cap)
        if yo is not None:
            if row.counted:
                assert nw == cap - 7, (nw, cap)             # capacity is get_num_output(n) + 7: exactly that many
            outs.append(yo.fetch_output(nw if row.counted else None))                   # point 1
            yo.free()
        for a, seg in ins:
            a.assert_input_intact(seg)                                                  # point 2
            a.free()
        pos += n
    return np.concatenate(outs) if row.out is not None else row.result(q)


# ---- FIR family: integer taps and samples, bit for bit against the oracle ----------------------------------------
ROWS = []


def fir_rows():
    rows = []
    for kind in KINDS:
        dt = T(kind)
        h63 = int_taps(np.random.default_rng(63), kind, 63)
        # fir_kernels.hip:331-340 (launch_fir_consec: 256 lanes x 8 outputs = 2048 per workgroup) and, for crcf,
        # stream_kernels.hip:371 (TILE 2048 unfused); 2 x 4096 + 3 covers two tiles of either
        rows.append(Row(f"firfilt-{kind}", "FirFilter.execute_block_dev",
                        lambda ya, o, kind=kind, h=h63: ya.FirFilter(kind, h), [(dt, 1)], (dt, 1),
                        lambda o, u, kind=kind: [int_samples(np.random.default_rng(1), kind, u)],
                        lambda q, xp, n, yp, cap: q.execute_block_dev(xp[0], n, yp),
                        lambda ya, o, xs, calls, kind=kind, h=h63: o.FirFilter(kind, h).execute_block(xs[0]),
                        2 * 4096 + 3, "fir_kernels.hip:331-340, stream_kernels.hip:371"))
        h129 = int_taps(np.random.default_rng(129), kind, 129)
        # fir_kernels.hip:494 (TILE = NT * R = 256 * 8 outputs at 32 taps per phase, :529)
        rows.append(Row(f"firdecim-{kind}", "FirDecimationFilter.execute_block_dev",
                        lambda ya, o, kind=kind, h=h129: ya.FirDecimationFilter(kind, 4, h), [(dt, 4)], (dt, 1),
                        lambda o, u, kind=kind: [int_samples(np.random.default_rng(2), kind, 4 * u)],
                        lambda q, xp, n, yp, cap: q.execute_block_dev(xp[0], n, yp),
                        lambda ya, o, xs, calls, kind=kind, h=h129:
                            o.FirDecimationFilter(kind, 4, h).execute_block(xs[0], len(xs[0]) // 4),
                        2 * 2048 + 3, "fir_kernels.hip:494,529"))
        nf, hlen = 13, 13 * 14 + 1
        hp = int_taps(np.random.default_rng(13), kind, hlen)
        # launch_fir_block with M = 1 and ny >= 512 goes to launch_fir_consec (fir_kernels.hip:512-513): kConsecTile =
        # 256 * 8 = 2048 outputs per workgroup (:224, :338-340); the 1- and 5-sample calls take fir_block_kernel with
        # tile = kFirR * kFirBlock = 1024 (:542, :552)
        rows.append(Row(f"firpfb-block-{kind}", "FirPfbFilter.execute_block_dev",
                        lambda ya, o, kind=kind, h=hp: ya.FirPfbFilter(kind, nf, h, hlen), [(dt, 1)], (dt, 1),
                        lambda o, u, kind=kind: [int_samples(np.random.default_rng(3), kind, u)],
                        lambda q, xp, n, yp, cap: q.execute_block_dev(5, xp[0], n, yp),
                        lambda ya, o, xs, calls, kind=kind, h=hp:
                            o.FirPfbFilter(kind, nf, h, hlen).execute_block(5, xs[0]),
                        2 * 4096 + 2, "fir_kernels.hip:224,512-513,542"))

        def pfb_all(ya, o, xs, calls, kind=kind, h=hp):
            ref = o.FirPfbFilter(kind, nf, h, hlen)
            out = np.empty((len(xs[0]), nf), T(kind))
            for k, v in enumerate(xs[0]):
                ref.push(v)
                out[k] = [ref.execute(i) for i in range(nf)]
            return out.ravel()

        def pfb_sel(ya, o, xs, calls, kind=kind, h=hp):
            ref = o.FirPfbFilter(kind, nf, h, hlen)
            out = np.empty(len(xs[1]), T(kind))
            for k, v in enumerate(xs[1]):
                ref.push(v)
                out[k] = ref.execute(int(xs[0][k]))
            return out

        # fir_kernels.hip:659-682: 256-lane workgroups, one pushed sample per lane in the few-branch form (:668)
        rows.append(Row(f"firpfb-all-{kind}", "FirPfbFilter.execute_all_dev",
                        lambda ya, o, kind=kind, h=hp: ya.FirPfbFilter(kind, nf, h, hlen), [(dt, 1)], (dt, nf),
                        lambda o, u, kind=kind: [int_samples(np.random.default_rng(4), kind, u)],
                        lambda q, xp, n, yp, cap: q.execute_all_dev(xp[0], n, yp), pfb_all,
                        2 * 256 + 3, "fir_kernels.hip:659-682"))
        rows.append(Row(f"firpfb-select-{kind}", "FirPfbFilter.execute_select_dev",
                        lambda ya, o, kind=kind, h=hp: ya.FirPfbFilter(kind, nf, h, hlen), [(U32, 1), (dt, 1)], (dt, 1),
                        lambda o, u, kind=kind: [np.random.default_rng(5).integers(0, nf, u).astype(np.uint32),
                                                 int_samples(np.random.default_rng(6), kind, u)],
                        lambda q, xp, n, yp, cap: q.execute_select_dev(xp[0], xp[1], n, yp), pfb_sel,
                        2 * 1024 + 3, "fir_kernels.hip:695,729 (kSelTile = 1024 outputs per workgroup)"))
        hi = int_taps(np.random.default_rng(48), kind, 48)
        rows.append(Row(f"firinterp-{kind}", "FirInterpolationFilter.execute_block_dev",
                        lambda ya, o, kind=kind, h=hi: ya.FirInterpolationFilter(kind, 4, h), [(dt, 1)], (dt, 4),
                        lambda o, u, kind=kind: [int_samples(np.random.default_rng(7), kind, u)],
                        lambda q, xp, n, yp, cap: q.execute_block_dev(xp[0], n, yp),
                        lambda ya, o, xs, calls, kind=kind, h=hi:
                            o.FirInterpolationFilter(kind, 4, h).execute_block(xs[0]),
                        2 * 1024 + 3, "fir_kernels.hip:659-682 (the all-branch kernel, 256 inputs per workgroup)"))
        P, Q, m = 3, 5, 15
        hr = int_taps(np.random.default_rng(35), kind, 2 * P * m)
        # fir_kernels.hip:791-797: tb = 1024 / max(P, Q) = 204 blocks per workgroup; 843 blocks = 4 tiles and 27
        rows.append(Row(f"rresamp-{kind}", "Rresamp.execute_block_dev",
                        lambda ya, o, kind=kind, h=hr: ya.Rresamp(kind, P, Q, m, h), [(dt, Q)], (dt, P),
                        lambda o, u, kind=kind: [int_samples(np.random.default_rng(8), kind, Q * u)],
                        lambda q, xp, n, yp, cap: q.execute_block_dev(xp[0], n, yp),
                        lambda ya, o, xs, calls, kind=kind, h=hr:
                            o.Rresamp(kind, P, Q, m, h).execute_block(xs[0], len(xs[0]) // Q),
                        3 * 256 + 75, "fir_kernels.hip:791-797"))
    return rows


ROWS += fir_rows()


def persistent_row():
    """the persistent stream form of the MFMA Toeplitz FIR: taken for ny >= 2^21 on a 16-byte aligned y, the tiled form
    otherwise (stream_kernels.hip:533); 2^21 + 777 is the smallest size class that selects it, output offset 0 and 1"""
    h = int_taps(np.random.default_rng(256), "crcf", 256)

    def make(ya, o):
        q = ya.FirFilter("crcf", h)
        q.set_kernel(3)
        return q
    return Row("firfilt-crcf-persistent", "FirFilter.execute_block_dev", make, [(C64, 1)], (C64, 1),
               lambda o, u: [int_samples(np.random.default_rng(9), "crcf", u)],
               lambda q, xp, n, yp, cap: q.execute_block_dev(xp[0], n, yp),
               lambda ya, o, xs, calls: o.FirFilter("crcf", h).execute_block(xs[0]),
               (1 << 21) + 777, "stream_kernels.hip:26 (kTile 4096), :533", pairs=[(0, 0), (0, 1)])


ROWS.append(persistent_row())


# ---- Resamp2 / MsResamp2 ------------------------------------------------------------------------------------------
R2_MODES = ["filter", "analyzer", "synthesizer", "decim", "interp"]
R2_UNITS = {"filter": (1, 2), "analyzer": (2, 2), "synthesizer": (2, 2), "decim": (2, 1), "interp": (1, 2)}


def resamp2_rows():
    rows = []
    m = 5
    hf = np.random.default_rng(7).integers(-3, 4, 4 * m + 1).astype(np.float32)       # test_gpu_resamp2.int_halfband
    for kind in KINDS:
        dt = T(kind)
        for mode in R2_MODES:
            pin, pout = R2_UNITS[mode]
            mi = R2_MODES.index(mode)
            # resamp2_kernels.hip:24 (kR2Tile = 256 lanes x 4 units = 1024 units per workgroup), launch at :150
            rows.append(Row(f"resamp2-{mode}-{kind}", "Resamp2.execute_block_dev",
                            lambda ya, o, kind=kind: ya.Resamp2(kind, hf, m, 0.0), [(dt, pin)], (dt, pout),
                            lambda o, u, kind=kind, pin=pin, mode=mode:
                                [int_samples(np.random.default_rng(10), kind, pin * u) * (2 if mode == "analyzer" else 1)],
                            lambda q, xp, n, yp, cap, mi=mi, pin=pin: q.execute_block_dev(mi, xp[0], n * pin, yp, cap),
                            lambda ya, o, xs, calls, kind=kind, mode=mode:
                                o.Resamp2(kind, hf, m, 0.0).execute_block(mode, xs[0]),
                            2 * 4096 + 3, "resamp2_kernels.hip:24,150"))
    return rows


ROWS += resamp2_rows()


def check_rel(tol):
    def check(got, want):
        assert got.shape == np.shape(want)
        assert rel_l2(got, want) <= tol, rel_l2(got, want)
    return check


def msresamp2_rows():
    """designed Kaiser stages (the oracle has no external-tap constructor): rel L2 <= 3e-6, test_msresamp2_vs_oracle"""
    rows = []
    ns, fc = 3, 0.45
    for kind in KINDS:
        dt = T(kind)
        for interp in (False, True):
            pin, pout = (1, 1 << ns) if interp else (1 << ns, 1)
            rows.append(Row(f"msresamp2-{'interp' if interp else 'decim'}-{kind}", "MsResamp2.execute_block_dev",
                            lambda ya, o, kind=kind, interp=interp:
                                ya.MsResamp2(kind, ya.MsResamp2.INTERP if interp else ya.MsResamp2.DECIM, ns, fc, 0.0, 60.0),
                            [(dt, pin)], (dt, pout),
                            lambda o, u, kind=kind, pin=pin: [rand_samples(np.random.default_rng(11), kind, pin * u)],
                            lambda q, xp, n, yp, cap: q.execute_block_dev(xp[0], n, yp),
                            lambda ya, o, xs, calls, kind=kind, interp=interp:
                                o.MsResamp2(kind, interp, ns, fc, 0.0, 60.0).execute_block(xs[0]),
                            2 * 1024 + 3, "resamp2_kernels.hip:529-608 (decimator), :741-762 (interpolator)",
                            check=check_rel(3e-6)))
    return rows


ROWS += msresamp2_rows()


# ---- Resamp / MsResamp: counted outputs, capacity get_num_output + 7 ----------------------------------------------
def resamp_rows():
    from resamp_util import RefResamp
    rows = []
    rate, m, npfb = float(np.float32(0.7123921)), 7, 256
    for kind in KINDS:
        dt = T(kind)
        h = int_taps(np.random.default_rng(77), kind, 2 * m * npfb)

        def want(ya, o, xs, calls, kind=kind, h=h):
            ref = RefResamp(o, kind, rate, m, npfb, h)
            out, pos = [], 0
            for n in calls:
                out.append(ref.execute_block(xs[0][pos:pos + n]))
                pos += n
            return np.concatenate(out)

        def call(q, xp, n, yp, cap):
            return q.execute_block_dev(xp[0], n, yp, cap)

        # fir_kernels.hip:890-895: at most 1024 outputs per workgroup
        rows.append(Row(f"resamp-{kind}", "Resamp.execute_block_dev",
                        lambda ya, o, kind=kind, h=h: ya.Resamp.from_taps(kind, rate, m, npfb, h), [(dt, 1)], (dt, 1),
                        lambda o, u, kind=kind: [int_samples(np.random.default_rng(12), kind, u)], call, want,
                        3 * 4096 + 3, "fir_kernels.hip:890-895", cap=lambda q, n: q.get_num_output(n) + 7, counted=True))
    return rows


def msresamp_rows():
    """the reference of test_gpu_msresamp.py::test_composition: the separately built parts chained by hand"""
    rows = []
    for kind, rate in (("crcf", 0.127115323), ("rrrf", 1.3)):
        dt = T(kind)
        rate = float(np.float32(rate))

        def want(ya, o, xs, calls, kind=kind, rate=rate):
            from test_gpu_msresamp import HandChain
            hand = HandChain(ya, kind, rate, 60.0)
            out, pos = [], 0
            for n in calls:
                out.append(hand.execute(xs[0][pos:pos + n]))
                pos += n
            return np.concatenate(out)

        rows.append(Row(f"msresamp-{kind}", "MsResamp.execute_dev",
                        lambda ya, o, kind=kind, rate=rate: ya.MsResamp(kind, rate, 60.0), [(dt, 1)], (dt, 1),
                        lambda o, u, kind=kind: [rand_samples(np.random.default_rng(13), kind, u)],
                        lambda q, xp, n, yp, cap: q.execute_dev(xp[0], n, yp, cap), want,
                        20003, "resamp2_kernels.hip:529-608 and fir_kernels.hip:881-898 (the two stages' launches)",
                        cap=lambda q, n: q.get_num_output(n) + 7, counted=True))
    return rows


ROWS += resamp_rows() + msresamp_rows()


# ---- FirHilbertFilter, Fdelay ------------------------------------------------------------------------------------
def firhilb_rows():
    from firhilb_ref import C2R, DECIM, INTERP, R2C, FirHilbRef, block, same_bits
    from test_firhilb_ref_cpu import rand_input
    shapes = {R2C: (F32, 1, C64, 1), C2R: (C64, 1, F32, 2), DECIM: (F32, 2, C64, 1), INTERP: (C64, 1, F32, 2)}
    rows = []
    m = 12

    def check(got, want):
        assert same_bits(got, want)

    for mode, (xdt, pin, ydt, pout) in shapes.items():
        def want(ya, o, xs, calls, mode=mode):
            hq = ya.firhilb_design(m, 60.0)
            y, _ = block(mode, hq, FirHilbRef(hq).state(), xs[0])
            return y

        # firhilb_kernels.hip:37 (kTile = kFirhilbTile pairs per workgroup), launch at :316
        rows.append(Row(f"firhilb-{mode}", f"FirHilbertFilter.{mode}_execute_block_dev",
                        lambda ya, o: ya.FirHilbertFilter(m, 60.0), [(xdt, pin)], (ydt, pout),
                        lambda o, u, mode=mode: [rand_input(np.random.default_rng(14), mode, u)],
                        lambda q, xp, n, yp, cap, mode=mode: getattr(q, mode + "_execute_block_dev")(xp[0], n, yp),
                        want, 2 * 4096 + 3, "firhilb_kernels.hip:37,316", check=check))
    return rows


def fdelay_rows():
    from fdelay_ref import Design, block, f32, lag, reset_state, same_bits
    from test_fdelay_ref_cpu import rand_input
    shape = (200, 8, 64)                                     # nmax, m, npfb
    rows = []

    def check(got, want):
        assert same_bits(got, want)

    for kind in KINDS:
        dt = T(kind)
        dl = f32(shape[0]) * f32(0.37)

        def make(ya, o, kind=kind):
            q = ya.Fdelay(kind, *shape)
            q.set_delay(dl)
            return q

        def want(ya, o, xs, calls, kind=kind):
            d = cached(("fdelay-design", kind), lambda: Design(o, kind, *shape))
            st = reset_state(d)
            st = st[:2] + (dl,) + lag(dl, d.nmax, d.npfb)
            y, _ = block(d, st, xs[-1], xs[0] if len(xs) == 2 else None)
            return y

        # fdelay_kernels.hip:284-323: `tiles` workgroups of kWg lanes
        rows.append(Row(f"fdelay-block-{kind}", "Fdelay.execute_block_dev", make, [(dt, 1)], (dt, 1),
                        lambda o, u, kind=kind: [rand_input(np.random.default_rng(15), kind, u)],
                        lambda q, xp, n, yp, cap: q.execute_block_dev(xp[0], n, yp), want,
                        2 * 4096 + 3, "fdelay_kernels.hip:284-312", check=check))
        rows.append(Row(f"fdelay-track-{kind}", "Fdelay.execute_track_dev", make, [(F32, 1), (dt, 1)], (dt, 1),
                        lambda o, u, kind=kind: [
                            (np.random.default_rng(16).random(u) * shape[0]).astype(np.float32),
                            rand_input(np.random.default_rng(17), kind, u)],
                        lambda q, xp, n, yp, cap: q.execute_track_dev(xp[0], xp[1], n, yp), want,
                        2 * 4096 + 3, "fdelay_kernels.hip:314-323", check=check))
    return rows


ROWS += firhilb_rows() + fdelay_rows()


# ---- IIR ---------------------------------------------------------------------------------------------------------
def iir_rows():
    from iir_ref import iir64
    from iirmap_ref import IirDecimRef, IirHilbRef, IirInterpRef
    from test_gpu_iir import int_signal, sos_int
    cdt = {"rrrf": np.float32, "crcf": np.float32, "cccf": np.complex64}
    rows = []
    for kind in KINDS:
        dt = T(kind)
        b4, a4 = sos_int(4)
        # iir_kernels.hip:526-533: G workgroups of kIirWg = 64 lanes (kernels.hpp:238), one chunk of T steps per lane,
        # T = 64 for the 8 state entries of 4 sections (test_gpu_iir.chunk_len): 4096 steps per workgroup, 8 tiles and 3
        rows.append(Row(f"iirfilt-{kind}", "IirFilter.execute_block_dev",
                        lambda ya, o, kind=kind: ya.IirFilter.new_sos(kind, b4.astype(cdt[kind]), a4.astype(cdt[kind]), 4),
                        [(dt, 1)], (dt, 1),
                        lambda o, u, kind=kind: [int_signal(np.random.default_rng(18), kind, u)],
                        lambda q, xp, n, yp, cap: q.execute_block_dev(xp[0], n, yp),
                        lambda ya, o, xs, calls, kind=kind: iir64(kind, b4, a4, xs[0], nsos=4, chunk=4096),
                        2 * 256 * 64 + 3, "iir_kernels.hip:526-533, kernels.hpp:238"))
        b2, a2 = sos_int(2)
        M = 5
        for interp, W, Ref in ((False, "IirDecimationFilter", IirDecimRef), (True, "IirInterpolationFilter", IirInterpRef)):
            pin, pout = (1, M) if interp else (M, 1)
            rows.append(Row(f"{'iirinterp' if interp else 'iirdecim'}-{kind}", f"{W}.execute_block_dev",
                            lambda ya, o, kind=kind, W=W: getattr(ya, W).new_sos(kind, M, b2.astype(cdt[kind]),
                                                                                  a2.astype(cdt[kind]), 2),
                            [(dt, pin)], (dt, pout),
                            lambda o, u, kind=kind, pin=pin: [int_signal(np.random.default_rng(19), kind, pin * u)],
                            lambda q, xp, n, yp, cap: q.execute_block_dev(xp[0], n, yp),
                            lambda ya, o, xs, calls, kind=kind, Ref=Ref: Ref(kind, M, b2, a2, nsos=2).execute_block(xs[0]),
                            2 * 256 * 16 + 3, "iir_kernels.hip:526,535 (iirmap_kernel: 64 lanes x 64 steps = 4096 steps per workgroup)"))
    b3, a3 = sos_int(3)
    hin = {"r2c": ("rrrf", 1, C64, 1), "c2r": ("crcf", 1, F32, 1), "decim": ("rrrf", 2, C64, 1), "interp": ("crcf", 1, F32, 2)}
    for mode, (kind, pin, ydt, pout) in hin.items():
        def want(ya, o, xs, calls, mode=mode):
            w = getattr(IirHilbRef(b3, a3, 3), mode + "_execute_block")(xs[0])
            return w

        def check(got, want):
            check_equal(got, np.asarray(want))

        rows.append(Row(f"iirhilb-{mode}", f"IirHilbertFilter.{mode}_execute_block_dev",
                        lambda ya, o: ya.IirHilbertFilter.new_sos(b3, a3, 3), [(T(kind), pin)], (ydt, pout),
                        lambda o, u, kind=kind, pin=pin: [int_signal(np.random.default_rng(20), kind, pin * u)],
                        lambda q, xp, n, yp, cap, mode=mode: getattr(q, mode + "_execute_block_dev")(xp[0], n, yp),
                        want, 2 * 256 * 16 + 3, "iir_kernels.hip:526,535 (iirmap_kernel: 64 lanes x 64 steps = 4096 steps per workgroup)", check=check))
    return rows


ROWS += iir_rows()


# ---- Osc ---------------------------------------------------------------------------------------------------------
def osc_rows():
    from osc_ref import OscRef
    rows = []
    for scheme in (0, 1):
        for down in (False, True):
            def make(ya, o, scheme=scheme):
                q = ya.Osc(ya.OscScheme(scheme))
                q.set_phase(1.234)
                q.set_frequency(0.1234 * 2 * np.pi)
                return q

            def want(ya, o, xs, calls, scheme=scheme, down=down):
                r = OscRef(scheme)
                r.set_phase(1.234)
                r.set_frequency(0.1234 * 2 * np.pi)
                return r.mix_block(xs[0], down)

            name = "mix_block_down_dev" if down else "mix_block_up_dev"
            # osc_kernels.hip:126 (G workgroups of kOscWg lanes), :137 (16-byte accesses only when x and y allow)
            rows.append(Row(f"osc-{'vco' if scheme else 'nco'}-{'down' if down else 'up'}", f"Osc.{name}", make,
                            [(C64, 1)], (C64, 1),
                            lambda o, u: [rand_samples(np.random.default_rng(21), "crcf", u)],
                            lambda q, xp, n, yp, cap, name=name: getattr(q, name)(xp[0], n, yp), want,
                            2 * 4096 + 3, "osc_kernels.hip:126,137"))
    return rows


ROWS += osc_rows()


# ---- FFT and its consumers ---------------------------------------------------------------------------------------
def fft_rows():
    rows = []
    # (n, transforms per workgroup): fft_kernels.hip:51 (B = 16 / M transforms per workgroup at N = 256 M),
    # :102 and :141 (nfr = 2048 / N transforms per workgroup), 4096 and 8192: one transform per workgroup (:78)
    for n, per_wg, direction in ((64, 32, "Forward"), (256, 16, "Forward"), (1024, 4, "Backward"), (4096, 1, "Forward"),
                                 (8192, 1, "Forward"), (8192, 1, "Backward"), (1000, 2, "Forward")):
        back = direction == "Backward"

        def want(ya, o, xs, calls, n=n, back=back):
            x = xs[0].astype(np.complex128).reshape(-1, n)
            return (np.fft.ifft(x, axis=1) * n if back else np.fft.fft(x, axis=1)).ravel()

        def check(got, want, n=n):
            g, w = got.reshape(-1, n), want.reshape(-1, n)
            for b in range(len(w)):
                assert rel_l2(g[b], w[b]) <= FFT_TOL, (b, rel_l2(g[b], w[b]))

        rows.append(Row(f"fft-{n}-{direction}", "Fft.run_batch_dev",
                        lambda ya, o, n=n, direction=direction: ya.Fft(n, ya.Direction[direction]), [(C64, n)], (C64, n),
                        lambda o, u, n=n: [o.gen_complex(SEED + 40 + n % 97, u * n)],
                        lambda q, xp, nb, yp, cap: q.run_batch_dev(xp[0], yp, nb), want,
                        2 * per_wg + 3, "fft_kernels.hip:51,78,102,141", check=check, guard=max(GUARD_MIN, n)))
    return rows


def fftfilt_rows():
    """tolerances of test_fftfilt_equals_direct_form; n = 4096 with more than 2049 taps runs the 8192-point plan"""
    rows = []
    for n, L in ((4096, 2050), (509, 510)):
        h = rand_taps(np.random.default_rng(n + L), "crcf", L)

        def make(ya, o, n=n, h=h):
            q = ya.FftFilt("crcf", h, n)
            q.set_scale(0.5)
            return q

        def check(got, want):
            assert rel_l2(got, want) <= 2e-6, rel_l2(got, want)
            assert np.max(np.abs(got - want)) <= 1e-5 * max(1.0, float(np.max(np.abs(want))))

        rows.append(Row(f"fftfilt-n{n}-L{L}", "FftFilt.execute_blocks_dev", make, [(C64, n)], (C64, n),
                        lambda o, u, n=n: [o.gen_complex(SEED + 41, u * n)],
                        lambda q, xp, nb, yp, cap: q.execute_blocks_dev(xp[0], nb, yp),
                        lambda ya, o, xs, calls, h=h: o.fir_block_f64("crcf", h, xs[0], scale=0.5),
                        3, "fft_kernels.hip:78 (one 2n-point transform per workgroup), stream_kernels.hip:546 (4096-point frames)",
                        check=check, guard=max(GUARD_MIN, 2 * n)))
    return rows


def stream_rows():
    rows = []
    for nfft in (4096, 8192):
        def make(ya, o, nfft=nfft):
            q = ya.FirFftStream(o.fir_design_kaiser(256, 0.2, 60.0), nfft)
            q.set_scale(0.4)
            return q

        def want(ya, o, xs, calls, nfft=nfft):                  # test_gpu_stream.spectra_truth
            y = o.fir_block_f64("crcf", o.fir_design_kaiser(256, 0.2, 60.0), xs[0], scale=0.4)
            return np.fft.fft(y.reshape(-1, nfft), axis=1).ravel()

        def check(got, want, nfft=nfft):
            g, w = got.reshape(-1, nfft), want.reshape(-1, nfft)
            for f in range(len(w)):
                assert rel_l2(g[f], w[f]) <= 1e-5, (f, rel_l2(g[f], w[f]))

        rows.append(Row(f"firfft-{nfft}", "FirFftStream.execute_dev", make, [(C64, nfft)], (C64, nfft),
                        lambda o, u, nfft=nfft: [o.gen_complex(SEED + 2, u * nfft)],
                        lambda q, xp, nf, yp, cap: q.execute_dev(xp[0], nf, yp), want,
                        3, "stream_kernels.hip:26 (kTile 4096 = one frame per workgroup)", check=check,
                        guard=max(GUARD_MIN, nfft)))
    return rows


def spgram_rows():
    """an input arena only; the PSD against oracle.Spgram at the tolerances of test_spgram_fused_vs_oracle"""
    rows = []
    for nfft, big in ((256, 12 * 4096 + 321), (4096, 40 * 4096 + 321), (800, 12 * 4096 + 321)):
        wlen = int(0.73 * nfft)
        wlen += wlen % 2
        delay = int(0.19 * nfft) | 1

        def want(ya, o, xs, calls, nfft=nfft, wlen=wlen, delay=delay):
            ref = o.Spgram(nfft, 2, wlen, delay)
            ref.write(xs[0])
            return ref.get_psd_mag()

        def check(got, want):
            assert np.max(np.abs(got - want) / want) <= 1e-3
            assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 2e-5

        rows.append(Row(f"spgram-{nfft}", "Spgram.write_dev",
                        lambda ya, o, nfft=nfft, wlen=wlen, delay=delay: ya.Spgram(nfft, ya.WindowType.Hann, wlen, delay),
                        [(C64, 1)], None,
                        lambda o, u: [o.gen_complex(SEED + 9, u) * np.float32(3e-2)],
                        lambda q, xp, n, yp, cap: q.write_dev(xp[0], n), want,
                        big, "spgram_kernels.hip:298-313 (one frame per workgroup), :257-259 (unfused)", check=check,
                        result=lambda q: q.get_psd_mag(), guard=max(GUARD_MIN, nfft)))
    return rows


ROWS += fft_rows() + fftfilt_rows() + stream_rows() + spgram_rows()


# ---- channelizers --------------------------------------------------------------------------------------------------
def chan_rows():
    """every frame against tests/chan_ref.py in complex128 (per-frame TAU, global bounds of test_gpu_chan_shapes.py)"""
    import torch
    from chan_ref import GPU_FRAME_TAU, FirPfbCh2Ref, FirPfbChRef, FrameCheck, shard_columns
    rows = []

    def frame_check(width, rel_bound):
        def check(got, want):
            w = torch.as_tensor(want).reshape(-1, width)
            fc = FrameCheck(w.shape[0])
            fc.add(0, w, torch.from_numpy(np.ascontiguousarray(got)).reshape(-1, width))
            worst, f, rel = fc.worst()
            assert worst <= GPU_FRAME_TAU, (f, worst)
            assert rel <= rel_bound, rel
        return check

    def taps(ya, op, M, k):                                  # test_gpu_chan_shapes._taps
        if op in ("ana", "syn"):
            return ya.fir_design_kaiser(M * k + 1, 0.5 / M, 60.0)
        h = ya.fir_design_kaiser(2 * M * k + 1, (1.0 if op == "ana2" else 0.5) / M, 60.0)
        return (h * M / h.sum()).astype(np.float32)

    M, k = 64, 4
    specs = [("ana", "FirPfbCh.analyzer_execute_dev", M, M, 2e-6), ("syn", "FirPfbCh.synthesizer_execute_dev", M, M, 3e-6),
             ("ana2", "FirPfbCh2.analyzer_execute_dev", M // 2, M, 2e-6),
             ("syn2", "FirPfbCh2.synthesizer_execute_dev", M, M // 2, 3e-6)]
    for op, entry, ui, uo, bound in specs:
        def make(ya, o, op=op):
            h = taps(ya, op, M, k)
            return ya.FirPfbCh(M, k, h) if op in ("ana", "syn") else ya.FirPfbCh2(M, k, h)

        def want(ya, o, xs, calls, op=op):
            h = taps(ya, op, M, k)
            ref = FirPfbChRef(M, k, h) if op in ("ana", "syn") else FirPfbCh2Ref(M, k, h)
            return (ref.analyzer_execute if op.startswith("ana") else ref.synthesizer_execute)(torch.from_numpy(xs[0])).numpy()

        name = entry.split(".")[1]
        # chan_kernels.hip launch_firpfbch_col / _syn_col / launch_firpfbch2_col / _syn_col: G = 256 / M column groups
        # per workgroup, runs of 64 .. 512 frames; 1027 frames is two runs of the longest and a ragged rest
        rows.append(Row(f"chan-{op}", entry, make, [(C64, ui)], (C64, uo),
                        lambda o, u, ui=ui: [o.gen_complex(SEED + 30, u * ui)],
                        lambda q, xp, n, yp, cap, name=name: getattr(q, name)(xp[0], n, yp), want,
                        1027, "chan_kernels.hip (launch_firpfbch_col, launch_firpfbch_syn_col, launch_firpfbch2_col, "
                        "launch_firpfbch2_syn_col)", check=frame_check(uo, bound), guard=max(GUARD_MIN, 8 * M)))
    R = 2
    for r in range(R):
        def want(ya, o, xs, calls, r=r):
            ref = FirPfbCh2Ref(M, k, taps(ya, "ana2", M, k))
            return shard_columns(ref.analyzer_execute(torch.from_numpy(xs[0])), r, R).contiguous().numpy()

        rows.append(Row(f"chan-ana2-shard-{r}of{R}", "FirPfbCh2.analyzer_execute_shard_dev",
                        lambda ya, o: ya.FirPfbCh2(M, k, taps(ya, "ana2", M, k)), [(C64, M // 2)], (C64, M // R),
                        lambda o, u: [o.gen_complex(SEED + 5, u * (M // 2))],
                        lambda q, xp, n, yp, cap, r=r: q.analyzer_execute_shard_dev(xp[0], n, r, R, yp), want,
                        1027, "chan_kernels.hip (launch_firpfbch2_col, SHARDED)", check=frame_check(M // R, 3e-6),
                        guard=max(GUARD_MIN, 8 * M)))

    # assemble_dev: gathered [rank][step][M / R] -> y [step][M] with channel k = r + R q; a pure permutation, bit for bit.
    # Its unit is one call's whole block (the layout depends on nsteps), so every call is a stream of its own.
    def assemble_want(ya, o, xs, calls):
        out, pos = [], 0
        for n in calls:
            g = xs[0][pos * M:(pos + n) * M].reshape(R, n, M // R)
            y = np.empty((n, M), np.complex64)
            for r in range(R):
                y[:, r::R] = g[r]
            out.append(y.ravel())
            pos += n
        return np.concatenate(out)

    rows.append(Row("chan-assemble", "FirPfbCh2.assemble_dev", lambda ya, o: ya.FirPfbCh2, [(C64, M)], (C64, M),
                    lambda o, u: [o.gen_complex(SEED + 6, u * M)],
                    lambda q, xp, n, yp, cap: q.assemble_dev(xp[0], n, M, R, yp), assemble_want,
                    1027, "chan_kernels.hip (firpfbch2 assemble kernel, 256 lanes per workgroup)"))
    return rows


ROWS += chan_rows()


# ---- the generators: an output arena only ------------------------------------------------------------------------
GEN_R_MAX = float(np.sqrt(-2.0 * np.log(2.0 ** -24)))        # the largest Box-Muller radius: u1 >= 2^-24
GEN_TOL = 8 * float(np.finfo(np.float32).eps) * GEN_R_MAX    # 5.5e-6


def check_gen(got, want):
    """The generator and the oracle's run the same f32 formula, r = sqrtf(-2 logf(u1)) times sinf / cosf of the same f32
    angle, on the same integers, but through two math libraries (the device's and the host's), so the words are not
    promised equal (yagi_hip.h: "in the shape of").  Each library's logf, sinf and cosf are within 2 ulp of the true
    value and sqrtf within 1: the two radii differ by at most (2 + 2) / 2 + 2 = 4 eps relative (the square root halves
    the logarithm's error), the two trigonometric factors by at most 4 eps absolute, so two samples differ by at most
    8 eps r <= 8 eps r_max.  Samples are O(1) apart from their neighbours, so a sample at the wrong index, or a second
    call that does not continue at `first`, is five orders of magnitude above this."""
    want = np.ascontiguousarray(want).astype(got.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = float(np.max(np.abs(got.view(np.float32).astype(np.float64) - want.view(np.float32))))
    print(f"generator: max |device - oracle| {err:.3e}, bound {GEN_TOL:.3e}")
    assert err <= GEN_TOL, err


def gen_rows():
    rows = []
    for name, dt, ref in (("gen_complex_dev", C64, "gen_complex"), ("gen_real_dev", F32, "gen_real")):
        state = {}

        def make(ya, o, name=name, state=state):
            state["first"] = 0
            return getattr(ya, name)

        def call(q, xp, n, yp, cap, state=state):
            q(SEED + 3, n, out=yp, first=state["first"])       # continues the sequence where the last call stopped
            state["first"] += n

        rows.append(Row(name.replace("_", "-"), name, make, [], (dt, 1), lambda o, u: [], call,
                        lambda ya, o, xs, calls, ref=ref: getattr(o, ref)(SEED + 3, sum(calls)),
                        2 * 4096 + 3, "misc_kernels.hip:44-52 (gen_grid, 256 lanes)", check=check_gen))
    return rows


ROWS += gen_rows()

CASES = [(row, ox, oy) for row in ROWS for ox, oy in row.offset_pairs()]


@pytest.mark.parametrize("row,ox,oy", CASES, ids=[f"{r.id}-x{ox}-y{oy}" for r, ox, oy in CASES])
def test_dev_entry_point_on_guarded_offset_buffers(ya, oracle, row, ox, oy):
    if _cache.get("device error"):
        pytest.fail(f"not run: {_cache['device error']} hit a device error, nothing more is started on the GPU")
    try:
        got = run_row(ya, oracle, row, ox, oy)                                      # points 1 and 2
    except ya.DeviceError:
        _cache["device error"] = f"{row.id} at ({ox}, {oy})"
        raise
    want = cached((row.id, "want"), lambda: row.want(ya, oracle, _cache[(row.id, "x")], row.calls))
    row.check(got, want)                                                            # point 3
    base = got if (ox, oy) == (0, 0) else cached((row.id, "base"), lambda: run_row(ya, oracle, row, 0, 0))
    if (ox, oy) == (0, 0):
        _cache.setdefault((row.id, "base"), got)
    assert got.shape == base.shape and np.array_equal(bits(got), bits(base)), \
        "the output depends on where the buffers start"                             # point 4
