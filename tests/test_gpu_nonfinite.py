"""The NaN / Inf footprint of every windowed block path, pinned to its reference model (tests/nonfinite_util.py).

One sample of a finite stream is made NaN, +Inf or -Inf (real part, imaginary part or both).  The object under test
and its existing reference model -- oracle.* in f32, tests/*_ref.py, chan_ref in complex128 -- run over the same
poisoned stream with the same call cuts.  The model's non-finite outputs are the reference's window; the library's must
be that set, or that set widened by a rule read off the kernel's code (a zero-padded tap or a transform block
multiplies what the reference never touches: 0 * NaN = NaN).  Set equality, not "at most"; every other output equals,
bit for bit, the run of a second object over the clean stream; and after reset() a clean block equals a fresh object's.

Placements, one at a time: (a) the first sample of the stream, (b) the last sample of one kernel tile and the first of
the next, (c) inside the last window - 1 samples of call 1 (the footprint continues into call 2 through the carried
state), (d) the very last sample of call 1 (poisons call 2 only), and for objects with per-sample host calls (e) the last
sample of call 2, followed by a few per-sample calls whose mask must be the model's (the mirror fetched the window).

Case -> kernel reached (the dispatch condition that sends it there):

FirFilter (capi.hip FirFilt::block_dev, fir_kernels.hip launch_fir_block)
  kernel 1, all kinds, n1 511            fir_block_kernel<STAGE> (M = 1 but ny < 512), one tile
  kernel 1, all kinds, n1 512            fir_consec_kernel (ny >= 512, span within 48 KiB), tile 2048, at its threshold
  kernel 1, all kinds, n1 2600           fir_consec_kernel, two tiles (seam 2047 | 2048); rrrf L >= 16 takes
                                         fir_consec_rrrf_body, L < 16 the generic body
  kernel 1, crcf L 3500, n1 1500         fir_block_kernel<STAGE = true>: the register-window span exceeds 48 KiB; tile 1024
  kernel 1, crcf L 6200, n1 700          fir_block_kernel<STAGE = false>: no tile of >= 64 outputs fits the LDS
  kernel 0, rrrf / cccf                  = kernel 1 (auto is the direct form for these kinds)
  kernel 0, crcf, n1 1000                launch_fir_block (n < 1024) -> fir_consec_kernel
  kernel 0, crcf, n1 1024 and 4700       firfilt_crcf_slide_kernel (n >= 1024, Lp <= 1024), tile 4096
  kernel 0, crcf, n1 2^16                fir_crcf_mfma_kernel<NS, false, 4, 2048> (n >= 2^16, L <= 256), tile 2048
  kernel 2, crcf                         firfilt_crcf_slide_kernel whatever the length (n1 600 and 4700)
  kernel 3, crcf, L <= 256               fir_crcf_mfma_kernel, Lm = 64 / 128 / 256 (L 257: no MFMA form, the general kernel)
  kernel 3, crcf, n1 3 * 2^20            fir_crcf_mfma_stream_kernel (ny >= 2^21, 16-byte aligned y): persistent form
  kernel 4, all kinds                    firfilt_fftconv_kernel: blocks of V outputs; rrrf: two blocks per workgroup
  pipelined, crcf kernel 0 and 1         the same kernels on the object's two lanes, window read from the previous
                                         call's input (DevWindow::begin_piped, calls of >= L samples)
  L in {1, 31, 32, 33, 65, 130, 256, 257} for every kernel that takes them.
FirDecimationFilter (launch_fir_block, M >= 2): one shape per launch_fir_decim_consec<NT, R> instantiation --
  <256,8>, <256,4>, <128,4>, <64,8>, <64,4> -- and fir_block_kernel (fewer than 8 taps per phase); decim_dispatch()
  below restates the choice and the tile, and test_nonfinite_util_cpu.py asserts that the cases reach all six.
FirPfbFilter: execute_block -> launch_fir_block on one branch (fir_consec_kernel); execute_all_dev with 4 branches ->
  firpfb_fewbranch_kernel (nf <= 16), with 32 -> firpfb_all_kernel<TAPS_LDS>; execute_select_dev -> firpfb_select_kernel.
FirInterpolationFilter, h_len 37 at rate 5 (sub-filters of 8 taps, three of them zero): firpfb_fewbranch_kernel on the
  padded bank.  The reference pads the same way (firinterp.rs:36-60), so its window already holds the zero taps.
Rresamp (3,5), (5,3), (160,147): rresamp_kernel, tiles of 204 / 204 / 6 blocks.
Resamp 0.3, 1.1, 3.7: resamp_kernel, tiles of 1024 outputs.
MsResamp 0.2 (two half-band decimator stages, then Resamp) and 5.3 (Resamp, then two interpolator stages).
Resamp2, five modes, m 5: resamp2_kernel<MODE>, tiles of 1024 units; the decimator block of 2^19 + 202 samples:
  launch_msresamp2_decim with one stage -- msresamp2_decim_kernel<1> for outputs [0, 256) and the tail,
  msresamp2_decim_fast_kernel<1> for the tiles of F = 1025 - 2m outputs in between (nx >= 2^19, m <= 64).
MsResamp2 decimator and interpolator, 1 to 4 stages: msresamp2_decim_kernel<S> / msresamp2_interp_kernel<S>; the
  decimator call of 2^21 + 1000 outputs (3 stages): msresamp2_decim_fast_kernel<3> in the middle (room >= 1024 * 231).
FirHilbertFilter, four modes, m 12: firhilb fast form (m <= 512), tiles of 2048 pairs; device entry points (host
  blocks of <= 4096 units would run on the host mirror).
Fdelay fixed delay: fdelay_block_kernel, tiles of 2048 (rrrf) / 1024 (complex); delay track: fdelay_track_kernel<XLDS>.
IirFilter TF and SOS, IirDecimationFilter, IirInterpolationFilter, IirHilbertFilter (four modes): iir_chunk_kernel /
  iirmap_kernel, chunks of 64 steps, workgroups of 64 chunks = 4096 steps: a full workgroup and a ragged second.
FirFftStream nfft 4096: variant 0 and 4 -> firfft_crcf_4096_freq_kernel (L <= 257); 1 -> firfft_crcf_4096_slide_kernel;
  2 -> fir_crcf_mfma_kernel<NS, true, 4, 4096>; 3 -> firfilt_fftconv_kernel + the batched transform; nfft 1000 ->
  firfilt_fftconv_kernel + the plan's transform.
FftFilt execute and execute_blocks, h_len <= 2049 -> FirFilter kernel 4 over the call; h_len 2100 -> the reference's
  five stages (pad, FFT, multiply, inverse, overlap-add).
Spgram 256, 1024 (spgram_fused_n256m_kernel<T, 1 / 4>), 4096 (spgram_fused4096_kernel), 1000 (launch_spgram_frames +
  batched transform + accumulate), wlen < nfft, delay > wlen so that some samples lie in no frame's window.
FirPfbCh analyzer / synthesizer, FirPfbCh2 analyzer / synthesizer:
  M 12 (not a power of two)              firpfbch_kernel<false>, firpfbch_syn_kernel<false>, firpfbch2_kernel,
                                         firpfbch2_syn_kernel: the generic kernels
  M 64, 40 frames / steps                the generic kernels (fewer than 64 frames)
  M 64 and M 16, 200 frames / steps      firpfbch_col_kernel<P, 6 / 4>, firpfbch_syn_col_kernel, firpfbch2_col_kernel,
                                         firpfbch2_syn_col_kernel (>= 64 frames, M in 8 .. 256), runs of 16
  M 512, 96 frames / steps               firpfbch_wide_kernel<P, 9>, firpfbch2_wide_kernel<P, 9> (p <= 8); the
                                         synthesizers have no wide kernel and take the generic one
  p in {4, 5, 6, 8, 16}, m in {2, 3, 4}: on and between the built branch lengths P.

Every listed path is reached at blocks of at most a few thousand samples except the four that need a long block by
their dispatch condition: FirFilter auto MFMA (2^16), the persistent MFMA form (3 * 2^20), the Resamp2 decimator's fast
middle (2^19) and the MsResamp2 decimator's fast middle (2^21 outputs).

Footprints that differ from the reference's window (rule and where it comes from; DESIGN.md section 6 has the table):
  sliding kernel          s .. s + Lp - 1, Lp = roundup(L, 32): fir_tile_slide multiplies taps_pad[L .. Lp) = 0.  Across a
                          call cut only while the sample is among the L the carried window holds.
  MFMA kernels            the same with Lm = 64 / 128 / 256.  The Toeplitz operand T[m][u] is zero, not absent, where a row's
                          window does not reach (the 16 outputs of a row tile share columns up to one sample past the
                          tile), which poisoned up to 16 outputs BEFORE the sample -- fused with the FFT (FirFftStream
                          variant 2) the whole previous frame -- until the kernels learnt to look for non-finite samples
                          (stream_kernels.hip mfma_task_poisoned, mfma_repair); mfma_rule asserts none is left.
  kernel 4 / FftFilt      whole overlap-save blocks of V outputs of the call (rrrf: pairs of blocks), see conv_rule.
  channelizer col / wide  frames f .. f + P - 1 (P the built branch length >= p), steps .. + 2P - 1 for firpfbch2;
                          firpfbch2 synthesizer: the ring of 8 / 16 lags in place of 4m.
  auto choice, call cuts  the padded forms carry the reference's window only, and the auto choice picks a kernel per call:
                          near a call cut the footprint depends on the length of the next call.
  Spgram                  the reference's set, but read through max(psd, 1e-12), which drops a NaN operand in the reference
                          and in the kernel alike: a NaN bin reads as the floor 1e-12 * scale, an infinite one as +Inf.
"""
import os

import numpy as np
import pytest

from gpu_util import rand_samples, rand_taps
from nonfinite_util import check_footprint, dilate, mask, poison

# the numpy models compute on the poisoned samples too: their "invalid value" warnings are the point, not noise
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")]
KINDS = ["rrrf", "crcf", "cccf"]
DT = {"rrrf": np.float32, "crcf": np.complex64, "cccf": np.complex64}


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


# ---- the sweep -------------------------------------------------------------------------------------------------------
def pairs(cuts):
    return list(zip(cuts[:-1], cuts[1:]))


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


class Obj:
    """an object under test or a model: block(x, a, b) runs one call over x[a:b] and returns its outputs, flat"""

    def __init__(self, q, fn, reset=None, single=None):
        self.q, self.fn, self._reset, self._single = q, fn, reset, single

    def block(self, x, a, b):
        return np.asarray(self.fn(self.q, x, a, b)).reshape(-1)

    def single(self, x, a, b):
        return np.asarray(self._single(self.q, x, a, b)).reshape(-1)

    def reset(self):
        (self._reset or self.q.reset)()


# (value, part) per placement; the first letter of the placement's name picks the list
COMBOS = {"a": [("nan", "re")], "b": [("nan", "im"), ("-inf", "both")], "c": [("nan", "re"), ("+inf", "im")],
          "d": [("nan", "both"), ("-inf", "re")], "e": [("nan", "re")], "m": [("nan", "re"), ("+inf", "both")]}


def spots(n1, tile=None, window=1, more=None):
    d = {"a first sample": 0}
    if tile and tile < n1:
        d["b- last sample of a tile"] = tile - 1
        d["b+ first sample of the next tile"] = tile
    if window >= 3:
        d["c in the carried window"] = n1 - 1 - min((window - 1) // 2, n1 // 2)
    d["d last sample of call 1"] = n1 - 1
    d.update(more or {})
    return d


def sweep(what, mk_gpu, mk_model, x, cuts, where, rule=None, control=None, tail=0, combos=None):
    """cuts: input indices of the call boundaries; x holds cuts[-1] + tail samples, the last `tail` of which go through
    per-sample calls; where: {placement name: input index}; rule(base, s, ocuts) widens the model's mask"""
    spans = pairs(cuts)
    g0 = mk_gpu()
    clean = [g0.block(x, a, b) for a, b in spans]
    if tail:
        clean.append(g0.single(x, cuts[-1], cuts[-1] + tail))
    ocuts = np.concatenate([[0], np.cumsum([len(c) for c in clean])])
    cleancat = np.concatenate(clean)
    assert not mask(cleancat).any(), what
    real = x.dtype.kind == "f"
    done = 0
    for name, s in where.items():
        for value, part in (combos or COMBOS)[name[0]]:
            tag = f"{what}: {name}, sample {s} {value} ({part})"
            xp = poison(x, s, value, "re" if real else part)
            g, m = mk_gpu(), mk_model()
            got = [g.block(xp, a, b) for a, b in spans]
            ref = [m.block(xp, a, b) for a, b in spans]
            if tail:
                got.append(g.single(xp, cuts[-1], cuts[-1] + tail))
                ref.append(m.block(xp, cuts[-1], cuts[-1] + tail))
            assert [len(v) for v in got] == [len(v) for v in ref] == [len(v) for v in clean], tag
            base = mask(np.concatenate(ref))
            want = rule(base, s, ocuts) if rule else base
            if tail:                                           # the per-sample calls are the reference's loop on the host
                want = want.copy()
                want[ocuts[-2]:] = base[ocuts[-2]:]
            gotcat = np.concatenate(got)
            check_footprint(gotcat, cleancat, want, tag)
            if control:
                control(gotcat, cleancat, base, want, tag)
            g.reset()
            again = g.block(x, *spans[0])
            assert np.array_equal(bits(again), bits(clean[0])), f"{tag}: after reset() a clean block differs from a fresh object's"
            done += 1
    return done


def dev_call(ya, call, x, ny, ydt):
    """one device-pointer call on fresh device arrays: call(x_dev, y_dev)"""
    xd = ya.DeviceArray.from_numpy(np.ascontiguousarray(x))
    yd = ya.DeviceArray(max(ny, 1), ydt)
    call(xd, yd)
    ya.synchronize()
    return yd.to_numpy(ny)


# ---- rules read off the kernels -----------------------------------------------------------------------------------------
def padded_rule(L, Lp, cuts, unit=1, hist=None, in_unit=1, padded=None):
    """a window of L units (samples, frames, steps) run as Lp >= L with zero taps behind the real ones: the model's mask
    widened to the right by Lp - L units of `unit` outputs.  The state carried across a call cut holds `hist` units
    (default L) of in_unit input samples each, so a later call sees the sample only while it is among them.  padded: per
    call, whether it runs the padded kernel (default: every call); the others keep the model's mask."""
    hist = L if hist is None else hist

    def rule(base, s, ocuts):
        w = dilate(base, (Lp - L) * unit)
        for i, ((a, b), oa, ob) in enumerate(zip(pairs(cuts), ocuts[:-1], ocuts[1:])):
            if s < a - hist * in_unit or (padded is not None and not padded[i]):
                w[oa:ob] = base[oa:ob]
        return w
    return rule


def mfma_rule(L, Lm, cuts, padded=None):
    """fir_crcf_mfma_kernel / fir_crcf_mfma_stream_kernel: the tap class Lm = 64 / 128 / 256 in place of L, like the sliding
    kernel with Lp = Lm.  The 16 outputs of a row tile share the Toeplitz operand's columns R - (Lm-1) .. R + 16, zeros
    where a row's own window does not reach; a wave whose span holds a non-finite sample runs the products with those
    samples zeroed and adds their terms to the outputs whose window holds them (mfma_repair), so nothing before s -- in
    the row tile, in the tile before or in the frame before -- is poisoned: asserted here on top of the exact set."""
    pad = padded_rule(L, Lm, cuts, padded=padded)

    def rule(base, s, ocuts):
        out = pad(base, s, ocuts)
        assert not out[:s].any() and not (base & ~out).any()
        return out
    return rule


def crcf_auto_form(L, n):
    """FirFilt<CRCF>::block_dev, kernel choice 0, for a call of n samples"""
    if L <= 256 and n >= 1 << 16:
        return "mfma"
    return "slide" if (L + 31) // 32 * 32 <= 1024 and n >= 1024 else "exact"


def conv_geometry(L, real):
    """launch_fir_fftconv_t: V outputs per 4096-point block, rounded down to whole 128-byte lines; P0 samples of history"""
    align = 32 if real else 16
    V = (4096 - (L - 1)) // align * align
    if V <= 0:
        V = 4096 - (L - 1)
    return V, 4096 - V


def conv_rule(L, cuts, real):
    """firfilt_fftconv_kernel: block k of a call makes outputs [kV, kV + V) from the 4096 samples [kV - P0, kV + V) of
    win ++ x (the window holds L samples, what lies past the call reads as zero); a non-finite sample makes the whole
    transform non-finite.  rrrf: blocks 2w and 2w + 1 share one complex transform, so they are poisoned together."""
    V, P0 = conv_geometry(L, real)
    G = 2 if real else 1

    def rule(base, s, ocuts):
        out = np.zeros_like(base)
        for a, b in pairs(cuts):
            n, r = b - a, s - a
            if r >= n or r < -min(L, P0):
                continue
            for k0 in range(0, -(-n // V), G):
                if k0 * V - P0 <= r < (k0 + G) * V:
                    out[a + k0 * V: min(a + (k0 + G) * V, b)] = True
        assert not (base & ~out).any()
        return out
    return rule


def frames_of(rule, nfft):
    """a sample-level rule -> whole frames of nfft outputs (a transform of a poisoned frame is poisoned everywhere)"""
    def frule(base, s, ocuts):
        w = rule(base, s, ocuts) if rule else base
        return np.repeat(w.reshape(-1, nfft).any(axis=1), nfft)
    return frule


# ---- FirFilter -----------------------------------------------------------------------------------------------------------
FIR_L = [1, 31, 32, 33, 65, 130, 256, 257]


def fir_objs(ya, oracle, kind, h, kernel, scale):
    def mk_gpu():
        q = ya.FirFilter(kind, h)
        q.set_scale(scale)
        q.set_kernel(kernel)

        def single(q, x, a, b):
            return np.array([q.execute_one(v) for v in x[a:b]], DT[kind])
        return Obj(q, lambda q, x, a, b: q.execute_block(x[a:b]), single=single)

    def mk_model():
        m = oracle.FirFilter(kind, h)
        m.set_scale(scale)
        return Obj(m, lambda m, x, a, b: m.execute_block(x[a:b]))
    return mk_gpu, mk_model


def fir_case(ya, oracle, kind, kernel, L, n1, n2, tile, rule=None, control=None, tail=0, seed=0, more=None, combos=None):
    rng = np.random.default_rng(4000 + 17 * L + n1 + seed)
    h, x = rand_taps(rng, kind, L), rand_samples(rng, kind, n1 + n2 + tail)
    scale = (0.5 + 0.25j) if kind == "cccf" else -0.5
    cuts = [0, n1, n1 + n2]
    mk_gpu, mk_model = fir_objs(ya, oracle, kind, h, kernel, scale)
    where = spots(n1, tile, L, more)
    if tail:
        where["e last sample of call 2"] = n1 + n2 - 1
    return sweep(f"FirFilter {kind} kernel {kernel} L {L} calls {n1} + {n2}", mk_gpu, mk_model, x, cuts, where,
                 rule(cuts) if rule else None, control, tail, combos)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L", FIR_L)
def test_firfilt_general_and_register_window_keep_the_reference_window(ya, oracle, kind, L):
    """kernel 1 (and, for rrrf / cccf, the auto choice): fir_block_kernel below 512 samples, fir_consec_kernel from 512 on
    (one tile at the threshold, two tiles at 2600).  The header promises the reference's window: s .. s + L - 1."""
    for n1, n2, tile in ((511, 300, None), (512, 300, None), (2600, 700, 2048)):
        fir_case(ya, oracle, kind, 1, L, n1, n2, tile, tail=5 if n1 == 511 else 0)
    if kind != "crcf":
        fir_case(ya, oracle, kind, 0, L, 2600, 700, 2048)


@pytest.mark.parametrize("L,n1,tile", [(3500, 1500, 1024), (6200, 700, None)])
def test_firfilt_general_kernel_long_filters(ya, oracle, L, n1, tile):
    """crcf, kernel 1 with a filter whose register-window span no longer fits 48 KiB: fir_block_kernel staged (L 3500,
    two tiles of 1024) and streamed from L2 (L 6200: no tile of 64 outputs fits)"""
    fir_case(ya, oracle, "crcf", 1, L, n1, 400, tile, combos={k: v[:1] for k, v in COMBOS.items()})


def slide_rule(L, auto=False):
    """kernel 2: every call; the auto choice: the calls of >= 1024 samples (a shorter one runs the register-window kernel,
    so the footprint of a sample near the end of call 1 depends on how long call 2 is)"""
    Lp = (L + 31) // 32 * 32
    return lambda cuts: padded_rule(L, Lp, cuts, padded=[crcf_auto_form(L, b - a) == "slide" for a, b in pairs(cuts)] if auto else None)


@pytest.mark.parametrize("L", FIR_L)
def test_firfilt_crcf_sliding_kernel_pads_to_32_taps(ya, oracle, L):
    """kernel 2 at any length, the auto choice from 1024 samples on: s .. s + Lp - 1, Lp = roundup(L, 32); below 1024
    samples the auto choice is the register-window kernel with the reference's window.  A sample in the last Lp - 1 but
    not the last L of call 1 does not reach call 2: the carried window holds L samples."""
    Lp = (L + 31) // 32 * 32
    more = {"c' behind the carried window": 4700 - L - 1} if Lp - 1 > L else None
    fir_case(ya, oracle, "crcf", 2, L, 600, 300, None, slide_rule(L), tail=5)
    fir_case(ya, oracle, "crcf", 2, L, 4700, 500, 4096, slide_rule(L), more=more)
    fir_case(ya, oracle, "crcf", 0, L, 1000, 300, None)
    fir_case(ya, oracle, "crcf", 0, L, 1024, 300, None, slide_rule(L, auto=True))
    fir_case(ya, oracle, "crcf", 0, L, 4700, 500, 4096, slide_rule(L, auto=True))
    fir_case(ya, oracle, "crcf", 0, L, 4700, 1100, 4096, slide_rule(L, auto=True), more=more)


def test_the_module_tells_a_widened_footprint_from_an_exact_one(ya, oracle):
    """positive control on the device: the crcf sliding kernel with L = 33 (Lp = 64).  The reference-window expectation
    must reject its output and only the Lp-dilated one accept it"""
    seen = []

    def control(got, clean, base, want, tag):
        check_footprint(got, clean, want, tag)
        with pytest.raises(AssertionError, match="poisoned but not expected: 31 elements in 1 runs"):
            check_footprint(got, clean, base, tag)
        with pytest.raises(AssertionError, match="footprint differs"):
            check_footprint(got, clean, dilate(base, 30), tag)
        with pytest.raises(AssertionError, match="footprint differs"):
            check_footprint(got, clean, dilate(base, 32), tag)
        seen.append(tag)
    n = fir_case(ya, oracle, "crcf", 2, 33, 2000, 300, None, slide_rule(33), control,
                 combos={"a": COMBOS["a"], "c": COMBOS["c"], "d": []})
    assert n == len(seen) == 3
    # the exact kernel on the same stream: the reference window is accepted, the dilated one rejected
    def exact(got, clean, base, want, tag):
        with pytest.raises(AssertionError, match="expected but finite:       31 elements"):
            check_footprint(got, clean, dilate(base, 31), tag)
    fir_case(ya, oracle, "crcf", 1, 33, 2000, 300, None, None, exact, combos={"a": COMBOS["a"], "c": [], "d": []})


def mfma_lm(L):
    return 64 if L <= 64 else 128 if L <= 128 else 256


@pytest.mark.parametrize("L", FIR_L)
def test_firfilt_crcf_mfma_kernel_pads_to_its_tap_class_and_nothing_before_the_sample(ya, oracle, L):
    """kernel 3: s .. s + Lm - 1 with Lm = 64 / 128 / 256 taps (mfma_rule), nothing before s wherever s sits in a row tile
    of 16 outputs or a tile of 2048; L = 257 has no MFMA form and runs the general kernel with the reference's window"""
    rule = (lambda cuts: mfma_rule(L, mfma_lm(L), cuts)) if L <= 256 else None
    more = {"m mid row tile": 1000 + 7, "b first sample of a row tile": 1008, "b last sample of a row tile": 1007 + 16}
    if L <= 256 and mfma_lm(L) - 1 > L:
        more["c' behind the carried window"] = 4700 - L - 1
    fir_case(ya, oracle, "crcf", 3, L, 600, 300, None, rule)
    fir_case(ya, oracle, "crcf", 3, L, 4700, 500, 2048, rule, more=more)


@pytest.mark.parametrize("kernel", [2, 3])
def test_firfilt_crcf_padded_kernels_with_several_bad_samples(ya, oracle, kernel):
    """NaN and both infinities, three of them inside one row tile of the MFMA kernel, one in a task of its own and one
    as the very last sample: the union of the single footprints, nothing else moved"""
    L, n = 33, 6000
    Lp = 64
    rng = np.random.default_rng(99)
    h, x = rand_taps(rng, "crcf", L), rand_samples(rng, "crcf", n)
    xp = x
    for s, value, part in ((1000, "nan", "re"), (1003, "-inf", "im"), (1011, "+inf", "both"), (3000, "nan", "im"), (n - 1, "+inf", "re")):
        xp = poison(xp, s, value, part)
    q, c = ya.FirFilter("crcf", h), ya.FirFilter("crcf", h)
    q.set_kernel(kernel), c.set_kernel(kernel)
    base = mask(oracle.FirFilter("crcf", h).execute_block(xp))
    check_footprint(q.execute_block(xp), c.execute_block(x), dilate(base, Lp - L), f"kernel {kernel}, five bad samples")


@pytest.mark.parametrize("L", [33, 256])
def test_firfilt_crcf_auto_takes_the_mfma_kernel_at_2_16(ya, oracle, L):
    """the auto choice from 2^16 samples on (L <= 256); call 2 is short and runs the register-window kernel"""
    fir_case(ya, oracle, "crcf", 0, L, 1 << 16, 600, 2048, lambda cuts: mfma_rule(L, mfma_lm(L), cuts, padded=[True, False]),
             combos={k: v[:1] for k, v in COMBOS.items()})


def test_firfilt_crcf_persistent_mfma_kernel(ya, oracle):
    """kernel 3 from 2^21 samples on: fir_crcf_mfma_stream_kernel, here 3 * 2^20 samples so that workgroups take a
    second tile, which arrives by LDS-DMA (tiles 1024 and up on a chip of 256 CUs)"""
    L, n1 = 33, 3 << 20                                        # 1536 tiles over at most 1024 workgroups
    more = {"b- seam in front of a DMA-staged tile": 1100 * 2048 - 1, "b+ first sample of a DMA-staged tile": 1100 * 2048,
            "m last tile": n1 - 700}
    fir_case(ya, oracle, "crcf", 3, L, n1, 600, 2048, lambda cuts: mfma_rule(L, 64, cuts), more=more,
             combos={k: v[:1] for k, v in COMBOS.items()})


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L", FIR_L)
def test_firfilt_fast_convolution_poisons_whole_blocks(ya, oracle, kind, L):
    """kernel 4: whole overlap-save blocks of V outputs (conv_rule); two blocks and a ragged third in call 1"""
    V, P0 = conv_geometry(L, kind == "rrrf")
    n1 = 2 * V + 500
    more = {"b- last sample of block 0": V - 1, "b+ first sample of block 1": V, "m in the overlap of block 1": V - 1 - (P0 // 2),
            "b just behind the overlap of block 1": V - P0 - 1}
    fir_case(ya, oracle, kind, 4, L, n1, 700, None, lambda cuts: conv_rule(L, cuts, kind == "rrrf"), more=more)


@pytest.mark.parametrize("kernel,L", [(1, 33), (0, 33), (0, 130)])
def test_firfilt_pipelined_calls_across_a_block_seam(ya, oracle, kernel, L):
    """set_pipeline(True): three device calls of >= L samples on the object's two lanes, each reading its window from
    the tail of the previous call's input; the footprint across both seams is the unpipelined kernel's"""
    kind = "crcf"
    rng = np.random.default_rng(77 + L)
    cuts = [0, 4700, 4700 + 1500, 4700 + 1500 + 2000]
    h, x = rand_taps(rng, kind, L), rand_samples(rng, kind, cuts[-1])
    rule = None if kernel == 1 else slide_rule(L, auto=True)(cuts)

    class Piped:
        def __init__(self):
            self.q = ya.FirFilter(kind, h)
            self.q.set_kernel(kernel)
            self.q.set_pipeline(True)

        def run(self, xs):
            xd, yd = ya.DeviceArray.from_numpy(xs), ya.DeviceArray(xs.size, np.complex64)
            for a, b in pairs(cuts):
                self.q.execute_block_dev(xd.ptr + 8 * a, b - a, yd.ptr + 8 * a)
            self.q.join()
            ya.synchronize()
            return yd.to_numpy()
    clean = Piped().run(x)
    for s in (0, 4095, 4096, 4700 - 3, 4699, 6199, 6200 - L + 1):
        xp = poison(x, s, "nan", "re")
        p = Piped()
        got = p.run(xp)
        m = oracle.FirFilter(kind, h)
        base = mask(np.concatenate([m.execute_block(xp[a:b]) for a, b in pairs(cuts)]))
        want = rule(base, s, np.array(cuts)) if rule else base
        check_footprint(got, clean, want, f"pipelined kernel {kernel} L {L} sample {s}")
        p.q.reset()
        assert np.array_equal(bits(p.run(x)), bits(clean))


# ---- FirDecimationFilter -------------------------------------------------------------------------------------------------
def decim_pitch(tile, L, M, R):
    ni = (L + M - 1) // M
    n = tile + ((ni + R - 1) & ~(R - 1)) + R
    return (n + n // R + 1) | 1


def decim_dispatch(kind, M, L, ny):
    """fir_kernels.hip launch_fir_block for M >= 2, restated: (the instantiation a shape reaches, its tile in outputs)"""
    size = 4 if kind == "rrrf" else 8
    budget = 48 * 1024
    min_steps = int(os.environ.get("YAGI_HIP_DECIM_WINDOW_MIN_STEPS", "8"))      # the library reads the same override
    if L >= M and L // M >= min_steps and ny >= 512:
        fits = lambda nt, r: M * decim_pitch(nt * r, L, M, r) * size <= budget
        long_phase = L // M >= 32
        short_ok = size == 8 or M <= 4
        if long_phase and fits(256, 8):
            return "consec<256,8>", 2048
        if long_phase or short_ok:
            if fits(256, 4):
                return "consec<256,4>", 1024
            if fits(128, 4):
                return "consec<128,4>", 512
        if long_phase and fits(64, 8):
            return "consec<64,8>", 512
        if long_phase and fits(64, 4):
            return "consec<64,4>", 256
    # fir_block_kernel: the largest tile (<= 1024 outputs, halved down to 64) whose phase-split span fits the LDS budget
    need = lambda t: M * ((((t - 1) * M + L + M - 1) // M) | 1) * size
    tile = 1024
    while tile >= 64 and need(tile) > budget:
        tile //= 2
    return "general", (tile if tile >= 64 else 1024)


DECIM_CASES = [("crcf", 2, 65), ("rrrf", 4, 129), ("crcf", 3, 64), ("cccf", 8, 129), ("crcf", 9, 288), ("cccf", 16, 513),
               ("rrrf", 16, 513), ("rrrf", 5, 7), ("crcf", 12, 50), ("rrrf", 8, 129)]
DECIM_FORMS = {"consec<256,8>", "consec<256,4>", "consec<128,4>", "consec<64,8>", "consec<64,4>", "general"}
# that DECIM_CASES reach every one of DECIM_FORMS is checked without a GPU: test_nonfinite_util_cpu.py


@pytest.mark.parametrize("kind,M,L", DECIM_CASES, ids=[f"{k}-M{M}-L{L}" for k, M, L in DECIM_CASES])
def test_firdecim_poisons_the_outputs_whose_window_holds_the_sample(ya, oracle, kind, M, L):
    """output o sees samples M o - (L - 1) .. M o (what test_firdecim_register_window_kernel asserts for one NaN in the
    middle of one call), here for NaN and +-Inf at the tile seams, in the carried window and at the end of call 1"""
    rng = np.random.default_rng(9100 + 37 * M + L)
    n1, n2 = 2600, 700
    form, tile = decim_dispatch(kind, M, L, n1)
    h, x = rand_taps(rng, kind, L), rand_samples(rng, kind, (n1 + n2) * M)
    cuts = [0, n1 * M, (n1 + n2) * M]

    def mk_gpu():
        q = ya.FirDecimationFilter(kind, M, h)
        q.set_scale(0.5)
        return Obj(q, lambda q, x, a, b: q.execute_block(x[a:b], (b - a) // M))

    def mk_model():
        m = oracle.FirDecimationFilter(kind, M, h)
        m.set_scale(0.5)
        return Obj(m, lambda m, x, a, b: m.execute_block(x[a:b], (b - a) // M))
    where = {"a first sample": 0, "b- newest sample of a tile's last output": (tile - 1) * M,
             "b+ first sample only the next tile sees": (tile - 1) * M + 1, "b newest sample of the next tile's first output": tile * M,
             "c in the carried window": n1 * M - 1 - (L - 1) // 2, "d last sample of call 1": n1 * M - 1,
             "m mid-call, off the decimation grid": 1300 * M + 1}

    def stated(base, s, ocuts):
        o = np.arange(n1 + n2)
        want = (M * o >= s) & (M * o - (L - 1) <= s)
        assert np.array_equal(want, base), "the model's mask is not the set the existing test states"
        return base
    sweep(f"FirDecimationFilter {kind} M {M} L {L} ({form}, tile {tile})", mk_gpu, mk_model, x, cuts, where, stated)


# ---- FirPfbFilter, FirInterpolationFilter, Rresamp, Resamp, MsResamp ----------------------------------------------------
def pfb_model(oracle, kind, nf, h, scale, pick):
    """per-sample loop over oracle.FirPfbFilter: push, then the branches pick(j) names for input j of the stream"""
    def mk():
        m = oracle.FirPfbFilter(kind, nf, h)
        m.set_scale(scale)

        def run(m, x, a, b):
            out = []
            for j in range(a, b):
                m.push(x[j])
                out += [m.execute(i) for i in pick(j)]
            return np.array(out, DT[kind])
        return Obj(m, run)
    return mk


@pytest.mark.parametrize("kind", KINDS)
def test_firpfb_block_all_and_select(ya, oracle, kind):
    rng = np.random.default_rng(31)
    scale = (0.5 - 0.25j) if kind == "cccf" else 0.75
    # execute_block: one branch of 33 taps over two tiles of the register-window kernel
    nf, Ls, n1, n2 = 4, 33, 2600, 700
    h, x = rand_taps(rng, kind, nf * Ls), rand_samples(rng, kind, n1 + n2)

    def gpu_block():
        q = ya.FirPfbFilter(kind, nf, h)
        q.set_scale(scale)
        return Obj(q, lambda q, x, a, b: q.execute_block(2, x[a:b]))
    def model_block():
        m = oracle.FirPfbFilter(kind, nf, h)
        m.set_scale(scale)
        return Obj(m, lambda m, x, a, b: m.execute_block(2, x[a:b]))
    sweep(f"FirPfbFilter {kind} execute_block", gpu_block, model_block, x, [0, n1, n1 + n2], spots(n1, 2048, Ls))
    # execute_all_dev: 4 branches (few-branch kernel, tiles of 256 samples) and 32 (all-branch kernel, tiles of 64)
    for nf, Ls, n1, n2, tile in ((4, 9, 700, 300, 256), (32, 9, 300, 100, 64), (3, 33, 700, 300, 256)):
        h, x = rand_taps(rng, kind, nf * Ls), rand_samples(rng, kind, n1 + n2)

        def gpu_all():
            q = ya.FirPfbFilter(kind, nf, h)
            q.set_scale(scale)
            return Obj(q, lambda q, x, a, b: q.execute_all(x[a:b]))
        sweep(f"FirPfbFilter {kind} execute_all_dev nf {nf}", gpu_all, pfb_model(oracle, kind, nf, h, scale, lambda j: range(nf)),
              x, [0, n1, n1 + n2], spots(n1, tile, Ls))
    # execute_select_dev: a branch index per sample, tiles of 1024
    nf, Ls, n1, n2 = 16, 12, 2600, 700
    h, x = rand_taps(rng, kind, nf * Ls), rand_samples(rng, kind, n1 + n2)
    idx = rng.integers(0, nf, n1 + n2).astype(np.uint32)

    def gpu_sel():
        q = ya.FirPfbFilter(kind, nf, h)
        q.set_scale(scale)
        return Obj(q, lambda q, x, a, b: q.execute_select(idx[a:b], x[a:b]))
    sweep(f"FirPfbFilter {kind} execute_select_dev", gpu_sel, pfb_model(oracle, kind, nf, h, scale, lambda j: [int(idx[j])]), x,
          [0, n1, n1 + n2], spots(n1, 1024, Ls))


@pytest.mark.parametrize("kind", KINDS)
def test_firinterp_padded_subfilters(ya, oracle, kind):
    """h_len 37 at rate 5: sub-filters of 8 taps over a bank padded with three zeros, in the reference as in the library,
    so the window is 8 input samples for every branch -- the padded branches included"""
    rng = np.random.default_rng(32)
    interp, hl, n1, n2 = 5, 37, 700, 300
    h, x = rand_taps(rng, kind, hl), rand_samples(rng, kind, n1 + n2)

    def mk_gpu():
        q = ya.FirInterpolationFilter(kind, interp, h)
        q.set_scale(0.5)
        return Obj(q, lambda q, x, a, b: q.execute_block(x[a:b]))

    def mk_model():
        m = oracle.FirInterpolationFilter(kind, interp, h)
        m.set_scale(0.5)
        return Obj(m, lambda m, x, a, b: m.execute_block(x[a:b]))

    def whole_window(base, s, ocuts):
        want = np.zeros_like(base)
        want[s * interp: (s + 8) * interp] = True
        assert np.array_equal(base, want), "the reference's window is not 8 samples x 5 branches"
        return base
    sweep(f"FirInterpolationFilter {kind}", mk_gpu, mk_model, x, [0, n1, n1 + n2], spots(n1, 256, 8), whole_window)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P,Q,m,tb", [(3, 5, 4, 204), (5, 3, 4, 204), (160, 147, 3, 6)])
def test_rresamp(ya, oracle, kind, P, Q, m, tb):
    rng = np.random.default_rng(33 + P)
    nb1, nb2 = (tb * 3) // 2, max(tb // 3, 3)
    h, x = rand_taps(rng, kind, 2 * P * m), rand_samples(rng, kind, (nb1 + nb2) * Q)

    def mk_gpu():
        q = ya.Rresamp(kind, P, Q, m, h)
        q.set_scale(0.5)
        return Obj(q, lambda q, x, a, b: q.execute_block(x[a:b], (b - a) // Q))

    def mk_model():
        r = oracle.Rresamp(kind, P, Q, m, h)
        r.set_scale(0.5)
        return Obj(r, lambda r, x, a, b: r.execute_block(x[a:b], (b - a) // Q))
    sweep(f"Rresamp {kind} {P}/{Q}", mk_gpu, mk_model, x, [0, nb1 * Q, (nb1 + nb2) * Q], spots(nb1 * Q, tb * Q, 2 * m))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rate", [0.3, 1.1, 3.7])
def test_resamp(ya, oracle, kind, rate):
    from resamp_util import RefResamp, designed_taps, rust_step
    m, npfb = 5, 32
    h = designed_taps(oracle, m, 0.4, 60.0, npfb)
    n1, n2 = int(2600 / rate) + 1, 300                         # about 2600 outputs in call 1: two tiles and a ragged third
    x = rand_samples(np.random.default_rng(34), kind, n1 + n2)
    seam_in = (1024 * rust_step(rate)) >> 24                  # the input the second tile's first output follows
    mk_gpu = lambda: Obj(ya.Resamp.from_taps(kind, rate, m, npfb, h), lambda q, x, a, b: q.execute_block(x[a:b]))
    mk_model = lambda: Obj(RefResamp(oracle, kind, rate, m, npfb, h), lambda r, x, a, b: r.execute_block(x[a:b]),
                           reset=lambda: None)
    sweep(f"Resamp {kind} rate {rate}", mk_gpu, mk_model, x, [0, n1, n1 + n2], spots(n1, seam_in, 2 * m))


@pytest.mark.parametrize("kind", ["rrrf", "crcf"])
@pytest.mark.parametrize("rate", [0.2, 5.3])
def test_msresamp(ya, oracle, kind, rate):
    """the model is the chain the object is built from (msresamp.rs:28-79): two half-band stages around a Resamp of 2 x 7
    taps and 256 branches; only which taps exist matters for a mask, not their values"""
    from resamp_util import RefResamp, designed_taps
    from test_gpu_msresamp import stages
    interp, ns, ra = stages(rate)
    assert ns == 2
    fc = float(min(np.float32(0.515) * ra, np.float32(0.49)))
    h = designed_taps(oracle, 7, fc, 60.0, 256)
    n1, n2 = (2000, 400) if interp else (8000, 1600)          # multiples of 2^ns: the decimator carries no leftover

    class Chain:
        def __init__(self):
            self.half = oracle.MsResamp2(kind, interp, ns, 0.4, 0.0, 60.0)
            self.arb = RefResamp(oracle, kind, float(ra), 7, 256, h.astype(np.float32))

        def execute(self, x):
            if interp:
                return self.half.execute_block(self.arb.execute_block(x))
            return self.arb.execute_block(self.half.execute_block(x))
    x = rand_samples(np.random.default_rng(35), kind, n1 + n2)
    mk_gpu = lambda: Obj(ya.MsResamp(kind, rate, 60.0), lambda q, x, a, b: q.execute(x[a:b]))
    mk_model = lambda: Obj(Chain(), lambda c, x, a, b: c.execute(x[a:b]), reset=lambda: None)
    sweep(f"MsResamp {kind} rate {rate}", mk_gpu, mk_model, x, [0, n1, n1 + n2], spots(n1, 1024, 14))


# ---- Resamp2, MsResamp2 ------------------------------------------------------------------------------------------------
R2_MODES = ["filter", "analyzer", "synthesizer", "decim", "interp"]


def r2_objs(ya, oracle, kind, hf, m, mode):
    def mk_gpu():
        q = ya.Resamp2(kind, hf, m)
        q.set_scale(0.37)
        return Obj(q, lambda q, x, a, b: q.execute_block(mode, x[a:b]))

    def mk_model():
        r = oracle.Resamp2(kind, hf, m)
        r.set_scale(0.37)
        return Obj(r, lambda r, x, a, b: r.execute_block(R2_MODES[mode], x[a:b]))
    return mk_gpu, mk_model


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", range(5), ids=R2_MODES)
def test_resamp2_forms(ya, oracle, kind, mode):
    m = 5
    hf = oracle.halfband_kaiser(m, 60.0)
    per = 1 if mode == 4 else 2                               # input samples per unit of the kernel's tile
    n1, n2 = 1300 * per, 300 * per
    x = rand_samples(np.random.default_rng(36 + mode), kind, n1 + n2)
    mk_gpu, mk_model = r2_objs(ya, oracle, kind, hf, m, mode)
    where = spots(n1, 1024 * per, 2 * m * per, {"b odd sample at the tile seam": 1024 * per + 1})
    sweep(f"Resamp2 {kind} {R2_MODES[mode]}", mk_gpu, mk_model, x, [0, n1, n1 + n2], where)


def test_resamp2_long_decimator_block_fast_middle_and_general_ends(ya, oracle):
    """2^19 + 202 input samples: outputs [0, 256) and the tail by msresamp2_decim_kernel<1>, the tiles of F = 1025 - 2m
    outputs in between by msresamp2_decim_fast_kernel<1>"""
    kind, m = "crcf", 5
    F = 1025 - 2 * m
    hf = oracle.halfband_kaiser(m, 60.0)
    n1, n2 = (1 << 19) + 202, 2 * 300
    nout = n1 // 2
    ntiles = (nout - 1 - 256) // F
    tail_first = 256 + ntiles * F
    assert ntiles * F >= 1024 * 231 and tail_first < nout
    x = rand_samples(np.random.default_rng(37), kind, n1 + n2)
    mk_gpu, mk_model = r2_objs(ya, oracle, kind, hf, m, 3)
    where = {"a general-kernel head": 2 * 100, "b- last input pair of the head": 2 * 256 - 1, "b+ first pair of the fast middle": 2 * 256,
             "m middle of a fast tile": 2 * (256 + 100 * F + F // 2) + 1, "b- fast tile seam": 2 * (256 + 100 * F) - 1,
             "b+ fast tile seam": 2 * (256 + 100 * F), "b last pair of the fast middle": 2 * tail_first - 1,
             "m general-kernel tail": 2 * tail_first + 7, "c in the carried window": n1 - 1 - 2 * m, "d last sample of call 1": n1 - 1}
    sweep("Resamp2 crcf decimator, 2^19 + 202 samples", mk_gpu, mk_model, x, [0, n1, n1 + n2], where,
          combos={k: v[:1] for k, v in COMBOS.items()})


def ms2_model(oracle, kind, interp, ms, hfs):
    """the chain of oracle.Resamp2 stages (msresamp2.rs:154-197): decimator from the last stage down, zeta = 1 / rate on
    the last one run; interpolator from stage 0 up"""
    def mk():
        chain = [oracle.Resamp2(kind, hfs[g], ms[g]) for g in range(len(ms))]
        if not interp:
            chain[0].set_scale(1.0 / (1 << len(ms)))

        def run(chain, x, a, b):
            v = x[a:b]
            order = range(len(ms)) if interp else range(len(ms) - 1, -1, -1)
            for g in order:
                v = chain[g].execute_block("interp" if interp else "decim", v)
            return v
        return Obj(chain, run, reset=lambda: None)
    return mk


@pytest.mark.parametrize("interp", [False, True], ids=["decim", "interp"])
@pytest.mark.parametrize("ms", [[5], [4, 3], [6, 3, 2], [3, 2, 4, 2]], ids=lambda v: f"{len(v)}-stages")
@pytest.mark.parametrize("kind", ["rrrf", "crcf"])
def test_msresamp2_chain(ya, oracle, kind, interp, ms):
    ns = len(ms)
    rate = 1 << ns
    hfs = [oracle.halfband_kaiser(m, 60.0) for m in ms]
    u1, u2 = 700, 200                                          # units (decimator outputs / interpolator inputs) per call
    per = 1 if interp else rate
    x = rand_samples(np.random.default_rng(38 + ns), kind, (u1 + u2) * per)
    T = ya.MsResamp2.INTERP if interp else ya.MsResamp2.DECIM
    mk_gpu = lambda: Obj(ya.MsResamp2.from_taps(kind, T, ms, hfs), lambda q, x, a, b: q.execute_block(x[a:b]))
    where = spots(u1 * per, 256 * per, 9, {"b odd sample at the tile seam": 256 * per + 1})
    sweep(f"MsResamp2 {kind} {'interp' if interp else 'decim'} {ms}", mk_gpu, ms2_model(oracle, kind, interp, ms, hfs), x,
          [0, u1 * per, (u1 + u2) * per], where)


def test_msresamp2_long_decimator_call_fast_middle(ya, oracle):
    """(1 << 21) + 1000 outputs, three stages (rrrf, m = 3, 2, 2): msresamp2_decim_fast_kernel<3> between the general
    kernel's head and tail"""
    kind, ms = "rrrf", [3, 2, 2]
    hfs = [oracle.halfband_kaiser(m, 60.0) for m in ms]
    n1, n2 = (1 << 21) + 1000, 300
    x = rand_samples(np.random.default_rng(39), kind, (n1 + n2) * 8)
    mk_gpu = lambda: Obj(ya.MsResamp2.from_taps(kind, ya.MsResamp2.DECIM, ms, hfs), lambda q, x, a, b: q.execute_block(x[a:b]))
    where = {"a general-kernel head": 8 * 50 + 3, "m fast middle": 8 * (1 << 20) + 5, "m general-kernel tail": 8 * (n1 - 20) + 1,
             "d last sample of call 1": 8 * n1 - 1}
    sweep("MsResamp2 rrrf decimator, 2^21 + 1000 outputs", mk_gpu, ms2_model(oracle, kind, False, ms, hfs), x,
          [0, 8 * n1, 8 * (n1 + n2)], where, combos={k: v[:1] for k, v in COMBOS.items()})


# ---- FirHilbertFilter, Fdelay -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["r2c", "c2r", "decim", "interp"])
def test_firhilb_modes(ya, mode):
    import firhilb_ref
    m = 12
    hq = ya.firhilb_design(m, 60.0)
    xin = np.float32 if mode in ("r2c", "decim") else np.complex64
    ydt = np.complex64 if mode in ("r2c", "decim") else np.float32
    per_in = 2 if mode == "decim" else 1                       # input samples per unit
    per_out = 1 if mode in ("r2c", "decim") else 2             # output elements per unit
    u1, u2, tail = 4096 + 700, 600, 6
    n = (u1 + u2 + tail) * per_in
    rng = np.random.default_rng(40)
    x = rand_samples(rng, "rrrf" if xin is np.float32 else "crcf", n)

    def mk_gpu():
        q = ya.FirHilbertFilter(m, 60.0)

        def run(q, x, a, b):
            nu = (b - a) // per_in
            return dev_call(ya, lambda xd, yd: getattr(q, mode + "_execute_block_dev")(xd, nu, yd), x[a:b], nu * per_out, ydt)

        def single(q, x, a, b):
            if mode == "r2c":
                return np.array([q.r2c_execute(v) for v in x[a:b]], np.complex64)
            if mode == "decim":
                return np.array([q.decim_execute(x[i:i + 2]) for i in range(a, b, 2)], np.complex64)
            if mode == "c2r":
                return np.array([q.c2r_execute(v) for v in x[a:b]], np.float32).reshape(-1)
            return np.concatenate([q.interp_execute(v) for v in x[a:b]])
        return Obj(q, run, single=single)

    class Model:
        def __init__(self):
            self.st = firhilb_ref.FirHilbRef(hq).state()

        def run(self, x, a, b):
            y, self.st = firhilb_ref.block(mode, hq, self.st, x[a:b])
            return y
    mk_model = lambda: Obj(Model(), lambda r, x, a, b: r.run(x, a, b), reset=lambda: None)
    cuts = [0, u1 * per_in, (u1 + u2) * per_in]
    where = spots(cuts[1], 4096 * per_in, 4 * m * per_in,
                  {"b odd sample at the tile seam": 4096 * per_in + 1, "e last sample of call 2": cuts[2] - 1})
    sweep(f"FirHilbertFilter {mode}", mk_gpu, mk_model, x, cuts, where, tail=tail * per_in)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("track", [False, True], ids=["fixed", "track"])
def test_fdelay(ya, oracle, kind, track):
    import fdelay_ref
    nmax, m, npfb = 40, 6, 16
    d = fdelay_ref.Design(oracle, kind, nmax, m, npfb)
    tile = 1024 if track or kind != "rrrf" else 2048
    n1, n2, tail = tile + 700, 500, 5
    rng = np.random.default_rng(41)
    x = rand_samples(rng, kind, n1 + n2 + tail)
    delays = (rng.uniform(0.0, nmax, n1 + n2 + tail)).astype(np.float32) if track else None
    fixed = np.float32(17.3)

    def mk_gpu():
        q = ya.Fdelay(kind, nmax, m, npfb)
        q.set_delay(fixed)

        def run(q, x, a, b):
            return q.execute_track(delays[a:b], x[a:b]) if track else q.execute_block(x[a:b])

        def single(q, x, a, b):
            out = []
            for j in range(a, b):
                if track:
                    q.set_delay(delays[j])
                q.push(x[j])
                out.append(q.execute())
            return np.array(out, DT[kind])

        def reset():
            q.reset()
            q.set_delay(fixed)
        return Obj(q, run, reset=reset, single=single)

    class Model:
        def __init__(self):
            w, f = fdelay_ref.lag(fixed, nmax, npfb)
            z = fdelay_ref.reset_state(d)
            self.st = (z[0], z[1], fixed, w, f)

        def run(self, x, a, b):
            y, self.st = fdelay_ref.block(d, self.st, x[a:b], delays[a:b] if track else None)
            return y
    mk_model = lambda: Obj(Model(), lambda r, x, a, b: r.run(x, a, b), reset=lambda: None)
    cuts = [0, n1, n1 + n2]
    where = spots(n1, tile, d.Ls + 18, {"e last sample of call 2": n1 + n2 - 1})
    sweep(f"Fdelay {kind} {'track' if track else 'fixed'}", mk_gpu, mk_model, x, cuts, where, tail=tail)


# ---- IIR objects ---------------------------------------------------------------------------------------------------------
IIR_N1, IIR_N2 = 4096 + 300, 100                               # filter steps of the two calls: a workgroup, a ragged second
IIR_SPOTS = {"a first step": 0, "b- last step of a chunk": 4096 - 65, "b+ first step of the next chunk": 4096 - 64,
             "b- last step of a workgroup": 4095, "b+ first step of the next workgroup": 4096, "m mid second workgroup": 4096 + 150,
             "c late in call 1": IIR_N1 - 3, "d last step of call 1": IIR_N1 - 1}
IIR_COMBOS = {"a": [("nan", "re")], "b": [("nan", "re")], "m": [("+inf", "both")], "c": [("-inf", "im")], "d": [("nan", "re")],
              "e": [("nan", "re")]}


class LoopModel:
    """a per-sample reference loop (iir_ref.Seq32, iirmap_ref.*) over the whole stream, call cuts being invisible to it.
    The loops cost ~0.4 ms a step, so the clean stream is run once per test, with a clone of the model kept every STEP
    inputs; a poisoned stream equals the clean one up to the bad sample and is run from the checkpoint in front of it."""
    STEP = 240                                                 # inputs between checkpoints (whole units of every form)

    def __init__(self, make, run, x, out_per_in):
        self.run, self.ratio, self.x = run, out_per_in, x
        m, self.marks, outs = make(), [], []
        for c in range(0, len(x), self.STEP):
            self.marks.append(m.clone())
            outs.append(run(m, x[c:c + self.STEP]))
        self.clean = np.concatenate(outs)

    def outputs(self, xp):
        bad = np.flatnonzero(mask(xp))
        if bad.size == 0:
            return self.clean
        assert np.array_equal(bits(xp[:bad[0]]), bits(self.x[:bad[0]]))
        c = int(bad[0]) // self.STEP * self.STEP
        m = self.marks[c // self.STEP].clone()
        o = int(round(c * self.ratio))
        return np.concatenate([self.clean[:o], self.run(m, xp[c:])])

    def factory(self):
        def mk():
            cache = {}

            def block(_, xp, a, b):
                if "y" not in cache:
                    cache["y"] = self.outputs(xp)
                return cache["y"][int(round(a * self.ratio)): int(round(b * self.ratio))]
            return Obj(None, block, reset=lambda: None)
        return mk


def from_some_index_on(base, s, ocuts):
    """a recursive filter never forgets: the model's mask is everything from its first non-finite output on"""
    if base.any():
        first = int(np.flatnonzero(base)[0])
        assert base[first:].all(), "the model's mask is not 'everything from some index on'"
    return base


@pytest.mark.parametrize("kind", ["rrrf", "crcf", "cccf"])
@pytest.mark.parametrize("form", ["tf", "sos"])
def test_iirfilt(ya, kind, form):
    """nothing before the bad sample is poisoned or moved by one bit: not in an earlier chunk of the wave's scan, not in
    an earlier workgroup, not in call 1 when the sample is its last"""
    from iir_ref import Seq32
    from test_gpu_iirmap import stable_sos, stable_tf
    rng = np.random.default_rng(42)
    if form == "tf":
        b, a = stable_tf(rng, kind, 5)
        mk_q, nsos = (lambda: ya.IirFilter(kind, b, a)), None
    else:
        b, a = stable_sos(rng, kind, 2)
        mk_q, nsos = (lambda: ya.IirFilter.new_sos(kind, b, a, 2)), 2
    tail = 4
    x = rand_samples(rng, kind, IIR_N1 + IIR_N2 + tail)

    def mk_gpu():
        return Obj(mk_q(), lambda q, x, a_, b_: q.execute_block(x[a_:b_]),
                   single=lambda q, x, a_, b_: np.array([q.execute(v) for v in x[a_:b_]], DT[kind]))
    model = LoopModel(lambda: Seq32(kind, b, a, nsos), lambda m, v: m.execute_block(v), x, 1)
    where = dict(IIR_SPOTS, **{"e last step of call 2": IIR_N1 + IIR_N2 - 1})
    sweep(f"IirFilter {kind} {form}", mk_gpu, model.factory(), x, [0, IIR_N1, IIR_N1 + IIR_N2], where, from_some_index_on,
          tail=tail, combos=IIR_COMBOS)


@pytest.mark.parametrize("kind", ["rrrf", "crcf"])
@pytest.mark.parametrize("interp", [False, True], ids=["decim", "interp"])
def test_iir_rate_changers(ya, kind, interp):
    from iirmap_ref import IirDecimRef, IirInterpRef
    from test_gpu_iirmap import stable_sos
    M = 3
    b, a = stable_sos(np.random.default_rng(43), kind, 2)
    u1, u2 = IIR_N1 // M + 1, 40                               # units: more than a workgroup of filter steps in call 1
    per = 1 if interp else M
    x = rand_samples(np.random.default_rng(44), kind, (u1 + u2) * per)
    R = IirInterpRef if interp else IirDecimRef

    def mk_gpu():
        W = ya.IirInterpolationFilter if interp else ya.IirDecimationFilter
        return Obj(W.new_sos(kind, M, b, a, 2), lambda q, x, a_, b_: q.execute_block(x[a_:b_]))
    model = LoopModel(lambda: R(kind, M, b, a, 2), lambda m, v: m.execute_block(v), x, M if interp else 1 / M)
    step = (lambda t: t // M) if interp else (lambda t: t)     # input index of filter step t
    where = {k: min(step(v), u1 * per - 1) for k, v in IIR_SPOTS.items() if k[0] in "abm"}
    where.update({"c late in call 1": u1 * per - 3, "d last sample of call 1": u1 * per - 1})
    sweep(f"Iir{'Interp' if interp else 'Decim'} {kind}", mk_gpu, model.factory(), x, [0, u1 * per, (u1 + u2) * per], where,
          from_some_index_on, combos=IIR_COMBOS)


@pytest.mark.parametrize("mode", ["r2c", "c2r", "decim", "interp"])
def test_iirhilb(ya, mode):
    """two real filters side by side: a sample poisons the one it enters, and from there on the outputs that one feeds --
    every output for r2c / decim / interp, every second one for c2r, as the model has it"""
    from iirmap_ref import IirHilbRef
    from test_gpu_iirmap import stable_sos
    b, a = stable_sos(np.random.default_rng(45), "rrrf", 2)
    per_in = 2 if mode == "decim" else 1
    per_out = 2 if mode == "interp" else 1
    steps = 2 if mode in ("decim", "interp") else 1            # filter steps per unit
    u1, u2 = IIR_N1 // steps + 1, 40
    xk = "rrrf" if mode in ("r2c", "decim") else "crcf"
    x = rand_samples(np.random.default_rng(46), xk, (u1 + u2) * per_in)
    mk_gpu = lambda: Obj(ya.IirHilbertFilter.new_sos(b, a, 2), lambda q, x, a_, b_: getattr(q, mode + "_execute_block")(x[a_:b_]))
    model = LoopModel(lambda: IirHilbRef(b, a, 2), lambda m, v: getattr(m, mode + "_execute_block")(v), x, per_out / per_in)
    n1 = u1 * per_in
    where = {k: min(v * per_in // steps, n1 - 1) for k, v in IIR_SPOTS.items() if k[0] in "abm"}
    where.update({"c late in call 1": n1 - 3, "d last sample of call 1": n1 - 1})
    sweep(f"IirHilbertFilter {mode}", mk_gpu, model.factory(), x, [0, n1, (u1 + u2) * per_in], where, combos=IIR_COMBOS)


# ---- FirFftStream, FftFilt ------------------------------------------------------------------------------------------------
def stream_case(ya, oracle, L, nfft, variant, rule_of, where, nf1=3, nf2=2):
    rng = np.random.default_rng(50 + L + variant)
    h, x = rand_taps(rng, "crcf", L), rand_samples(rng, "crcf", (nf1 + nf2) * nfft)
    cuts = [0, nf1 * nfft, (nf1 + nf2) * nfft]

    def mk_gpu():
        q = ya.FirFftStream(h, nfft)
        q.set_scale(0.4)
        q.set_variant(variant)
        return Obj(q, lambda q, x, a, b: q.execute(x[a:b]))

    class Model:
        """the sample-level model: oracle.FirFilter over the stream; the rule turns its mask into frames"""
        def __init__(self):
            self.f = oracle.FirFilter("crcf", h)
            self.f.set_scale(0.4)
    mk_model = lambda: Obj(Model(), lambda r, x, a, b: r.f.execute_block(x[a:b]), reset=lambda: None)
    sample_rule = rule_of(cuts) if rule_of else None

    def rule(base, s, ocuts):
        want = frames_of(sample_rule, nfft)(base, s, ocuts)
        # the composition's own model (FIR -> frames -> f32 FFT) on the same stream: the reference's frames
        if nfft & (nfft - 1) == 0:                             # the oracle's transform takes powers of two
            ref = mask(oracle.stream_fir_fft(h, 0.4, poison(x, s, "nan", "re"), nfft)).reshape(-1)
            assert np.array_equal(ref, frames_of(None, nfft)(base, s, ocuts)), "frame model and sample model disagree"
            if sample_rule is None:
                assert np.array_equal(ref, want)
        return want
    sweep(f"FirFftStream L {L} nfft {nfft} variant {variant}", mk_gpu, mk_model, x, cuts, where, rule,
          combos={"a": [("nan", "re")], "b": [("nan", "im"), ("+inf", "both")], "c": [("nan", "re")], "d": [("-inf", "re")],
                  "m": [("nan", "re")]})


def stream_spots(L, nfft, nf1):
    d = {"a first sample": 0, "b- last sample of frame 0": nfft - 1, "b+ first sample of frame 1": nfft,
         "m mid frame 1": nfft + nfft // 2, "d last sample of call 1": nf1 * nfft - 1}
    if L >= 3:
        d["c in the last L - 1 samples of frame 0"] = nfft - 1 - (L - 1) // 2
        d["c in the last L - 1 samples of call 1"] = nf1 * nfft - 1 - (L - 1) // 2
    if L < 256:
        d["b in the last 255 but not the last L - 1 samples of frame 1"] = 2 * nfft - 200
        d["b the same, at the end of call 1"] = nf1 * nfft - 200
    return d


# variant 2 (MFMA) takes at most 256 taps: 64, 130 and 256 for it, 257 as well for the others
STREAM_CASES = [(v, L) for v in range(5) for L in (64, 130, 256, 257) if not (v == 2 and L > 256)]


@pytest.mark.parametrize("variant,L", STREAM_CASES)
def test_firfftstream_4096_which_frames(ya, oracle, variant, L):
    """within a frame everything is poisoned (the transform mixes every sample); pinned is which frames: the one holding
    s, the next one if s lies in its last L - 1 samples (variants 0 and 4: exactly that, the 512-point correction masks
    what lies beyond L - 1 with a select), and what the padded direct forms (1, 2) and the overlap-save blocks (3) add.
    Variant 2: a bad first sample of a frame must leave the frame before it alone (placement b+)"""
    rule_of = {0: None, 4: None, 1: slide_rule(L), 2: lambda cuts: mfma_rule(L, mfma_lm(L), cuts),
               3: lambda cuts: conv_rule(L, cuts, False)}[variant]
    stream_case(ya, oracle, L, 4096, variant, rule_of, stream_spots(L, 4096, 3))


def test_firfftstream_nfft_1000(ya, oracle):
    L, nfft = 130, 1000
    where = stream_spots(L, nfft, 9)
    V, P0 = conv_geometry(L, False)
    where.update({"b- last sample of overlap-save block 0": V - 1, "b+ first sample of block 1": V})
    stream_case(ya, oracle, L, nfft, 0, lambda cuts: conv_rule(L, cuts, False), where, nf1=9, nf2=3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L,n", [(33, 1000), (257, 3000), (130, 5000)])
def test_fftfilt_short_filters_poison_overlap_save_blocks(ya, oracle, kind, L, n):
    """h_len <= 2049: execute and execute_blocks are FirFilter kernel 4 over the call's nblocks * n samples, so the
    footprint is conv_rule's blocks of V outputs of each CALL -- not the reference's block n and the one after it.
    Both hold the L outputs whose window has the sample (asserted: the model here is oracle.FirFilter)."""
    rng = np.random.default_rng(60 + L)
    nb1, nb2 = 3, 2
    h, x = rand_taps(rng, kind, L), rand_samples(rng, kind, (nb1 + nb2 + 1) * n)
    mk_model = lambda: Obj(oracle.FirFilter(kind, h), lambda r, x, a, b: r.execute_block(x[a:b]))
    V, P0 = conv_geometry(L, kind == "rrrf")
    # execute_blocks: calls of 3 n and 2 n samples, then one execute of n
    cuts = [0, nb1 * n, (nb1 + nb2) * n, (nb1 + nb2 + 1) * n]
    mk_gpu = lambda: Obj(ya.FftFilt(kind, h, n), lambda q, x, a, b: q.execute_blocks(x[a:b]) if b - a > n else q.execute(x[a:b]))
    where = spots(nb1 * n, V if V < nb1 * n else n, L, {"m second block of call 1": n + n // 2, "d last sample of call 2": cuts[2] - 1})
    sweep(f"FftFilt {kind} L {L} n {n} execute_blocks", mk_gpu, mk_model, x, cuts, where, conv_rule(L, cuts, kind == "rrrf"))
    # execute: every block a call of its own
    cuts1 = list(range(0, 4 * n + 1, n))
    mk_gpu1 = lambda: Obj(ya.FftFilt(kind, h, n), lambda q, x, a, b: q.execute(x[a:b]))
    where1 = {"a first sample": 0, "c in the carried window": n - 1 - (L - 1) // 2, "d last sample of call 1": n - 1,
              "b first sample of call 2": n, "m mid call 3": 2 * n + n // 2}
    sweep(f"FftFilt {kind} L {L} n {n} execute", mk_gpu1, mk_model, x[: 4 * n], cuts1, where1, conv_rule(L, cuts1, kind == "rrrf"))


def test_fftfilt_long_filter_keeps_the_reference_blocks(ya, oracle):
    """h_len 2100 > 2049: the reference's five stages; the footprint is the reference's -- block b and, through the
    overlap-add tail, block b + 1, whole"""
    kind, L, n = "crcf", 2100, 2100
    rng = np.random.default_rng(61)
    h, x = rand_taps(rng, kind, L), rand_samples(rng, kind, 5 * n)
    cuts = [0, 3 * n, 5 * n]
    mk_gpu = lambda: Obj(ya.FftFilt(kind, h, n), lambda q, x, a, b: q.execute_blocks(x[a:b]))

    def mk_model():
        m = oracle.FftFilt(kind, h, n)
        return Obj(m, lambda m, x, a, b: np.concatenate([m.execute(x[i:i + n]) for i in range(a, b, n)]))

    def two_blocks(base, s, ocuts):
        want = np.zeros_like(base)
        want[s // n * n: (s // n + 2) * n] = True
        assert np.array_equal(base, want), "the reference's footprint is not block b and block b + 1"
        return base
    where = {"a first sample": 0, "b first sample of block 1": n, "d last sample of call 1": 3 * n - 1}
    sweep("FftFilt crcf L 2100", mk_gpu, mk_model, x, cuts, where, two_blocks, combos={k: v[:1] for k, v in COMBOS.items()})


# ---- Spgram -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.complex64, np.float32], ids=["cf", "f"])
@pytest.mark.parametrize("nfft,wlen,delay", [(256, 100, 150), (1024, 700, 900), (4096, 3000, 3500), (1000, 400, 650)])
def test_spgram_covered_and_uncovered_samples(ya, oracle, dtype, nfft, wlen, delay):
    """frame f (newest sample delay (f + 1) - 1) tapers the wlen samples before it with a select; the delay - wlen
    samples between two windows belong to no frame: a non-finite value there leaves the PSD bit-identical, one inside a
    window poisons every bin (the model's bins): NaN bins read as the floor 1e-12 * scale, infinite ones as +Inf (see
    `marked`).  The fused kernels read the nfft samples from the window's start on (beyond wlen they are zeroed by a
    select, not multiplied)"""
    nfr1, nfr2 = 9, 4
    n1, n2 = (nfr1 + 1) * delay - wlen // 2, nfr2 * delay     # call 1 ends inside the window of its frame nfr1
    rng = np.random.default_rng(70 + nfft)
    x = rand_samples(rng, "crcf" if dtype is np.complex64 else "rrrf", n1 + n2)
    W = ya.WindowType.Hamming
    end = lambda f: delay * (f + 1) - 1                        # newest sample of frame f
    covered = {"a first sample of frame 0's window": end(0) - (wlen - 1), "b last sample of frame 3's window": end(3),
               "b first sample of frame 4's window": end(4) - (wlen - 1), "c window of the first frame of call 2": n1 - 3,
               "m frame 11, call 2": end(11) - 5}
    uncovered = {"a first sample of the stream": 0, "b just behind frame 3's window": end(3) + 1,
                 "b just before frame 4's window": end(4) - wlen, "b nfft - 1 past frame 4's window start": min(end(4) - (wlen - 1) + nfft - 1, end(5) - wlen),
                 "d last sample of the stream": n1 + n2 - 1}
    assert end(nfr1) - (wlen - 1) < n1 - 3 and n1 <= end(nfr1)

    def run(q):
        return lambda xs: (q.write(xs[:n1]), q.write(xs[n1:]), q.get_psd_mag())[2]
    # get_psd_mag is max(psd, 1e-12) * scale with f32::max, which drops a NaN operand (spgram.rs:302, spgram_psd_kernel's
    # fmaxf): a NaN bin of the accumulated PSD reads as the floor, an infinite one as +Inf.  Both count as poisoned
    floor = np.float32(1e-12) * np.float32(1.0 / (nfr1 + nfr2))

    def marked(y):
        y = y.copy()
        y[mask(y) | (y == floor)] = np.nan
        return y
    q0 = ya.Spgram(nfft, W, wlen, delay, dtype=dtype)
    clean = run(q0)(x)
    assert q0.get_num_transforms() == nfr1 + nfr2 and not mask(marked(clean)).any()
    for group, expect in ((covered, True), (uncovered, False)):
        for name, s in group.items():
            for value, part in COMBOS[name[0]][: 2 if name[0] == "m" else 1]:
                tag = f"Spgram nfft {nfft} wlen {wlen} delay {delay}: {name}, sample {s} {value}"
                xp = poison(x, s, value, "re" if dtype is np.float32 else part)
                q = ya.Spgram(nfft, W, wlen, delay, dtype=dtype)
                got = run(q)(xp)
                ref = oracle.Spgram(nfft, int(W), wlen, delay, dtype=dtype)
                ref.write(xp[:n1])
                ref.write(xp[n1:])
                base = mask(marked(ref.get_psd_mag()))
                assert base.all() if expect else not base.any(), tag
                if expect and value == "nan":
                    assert np.array_equal(bits(got), bits(np.full(nfft, floor))), f"{tag}: a NaN PSD reads as the floor"
                check_footprint(marked(got), clean, base, tag)
                q.reset()
                assert np.array_equal(bits(run(q)(x)), bits(clean)), f"{tag}: reset() does not clear the state"


# ---- channelizers ---------------------------------------------------------------------------------------------------------
def chan_built(op, M, k, nframes):
    """the branch length P the kernel a shape reaches is built for (chan_kernels.hip launch_firpfbch, launch_firpfbch_syn,
    launch_firpfbch2, launch_firpfbch2_syn), in taps per branch; None: the generic kernel, which runs p taps.
    firpfbch2 synthesizer: the ring of lags, in steps, in place of 4m."""
    col = M in (8, 16, 32, 64, 128, 256) and nframes >= 64
    if op == "ana":
        if M in (512, 1024) and k <= 8 and nframes >= 64:
            return 4 if k <= 4 else 8
        return (4 if k <= 4 else 8 if k <= 8 else 16 if k <= 16 else None) if col else None
    if op == "syn":
        return (4 if k <= 4 else 8 if k <= 8 else 16 if k <= 16 else None) if col else None
    p = 2 * k
    if op == "ana2":
        if nframes >= 64 and ((M == 512 and p <= 8) or (M == 1024 and p <= 4)):
            return 2 if p <= 2 else 4 if p <= 4 else 8
        return (2 if p <= 2 else 4 if p <= 4 else 8 if p <= 8 else 16 if p <= 16 else None) if col else None
    return (8 if k <= 2 else 16) if (col and k <= 4) else None


CHAN_SHAPES = [(12, 40, 200), (64, 40, 30), (64, 200, 100), (16, 200, 100), (512, 96, 70)]


def chan_case(ya, op, M, k, nf1, nf2):
    import torch
    from chan_ref import FirPfbCh2Ref, FirPfbChRef
    two = op.endswith("2")
    if two:
        hh = ya.fir_design_kaiser(2 * M * k + 1, (1.0 if op == "ana2" else 0.5) / M, 60.0)
        hh = (hh * M / hh.sum()).astype(np.float32)
    else:
        hh = ya.fir_design_kaiser(M * k + 1, 0.5 / M, 60.0)
    ui, uo = {"ana": (M, M), "syn": (M, M), "ana2": (M // 2, M), "syn2": (M, M // 2)}[op]
    x = rand_samples(np.random.default_rng(80 + M + k), "crcf", (nf1 + nf2) * ui)
    cuts = [0, nf1 * ui, (nf1 + nf2) * ui]
    name = "analyzer_execute" if op.startswith("ana") else "synthesizer_execute"

    def mk_gpu():
        q = ya.FirPfbCh2(M, k, hh) if two else ya.FirPfbCh(M, k, hh)
        return Obj(q, lambda q, x, a, b: getattr(q, name)(x[a:b]))

    def mk_model():
        r = FirPfbCh2Ref(M, k, hh) if two else FirPfbChRef(M, k, hh)
        return Obj(r, lambda r, x, a, b: getattr(r, name)(torch.from_numpy(x[a:b])).numpy().astype(np.complex64), reset=lambda: None)
    # units of the window: frames for firpfbch (p of them), steps for firpfbch2 (2p = 4m)
    win = 2 * (2 * k) if two else k
    P = chan_built(op, M, k, nf1)
    built = win if P is None else (P if op == "syn2" else (2 * P if two else P))
    assert built >= win
    hist = win - 1                                             # frames / steps the carried state holds
    rule = None
    if built > win:
        rule = padded_rule(win, built, cuts, unit=uo, hist=hist, in_unit=ui)
    run = 16 if P is not None else max(1, 4096 // M)           # frames per run / per tile of the generic kernels
    where = {"a first sample": 0, "m one column, mid call": 30 * ui + ui // 3, "c in the carried history": (nf1 - max(1, hist // 2)) * ui + 1,
             "d last sample of call 1": nf1 * ui - 1}
    if run < nf1:
        where.update({"b- last sample of a run": run * ui - 1, "b+ first sample of the next run": run * ui})
    if built > win:
        where["c' behind the carried history"] = (nf1 - hist - 1) * ui + 2
    what = f"{op} M {M} {'m' if two else 'p'} {k}, {nf1} + {nf2} {'steps' if two else 'frames'} (built {P})"

    def whole_units(base, s, ocuts):
        f0 = s // ui
        want = np.zeros(nf1 + nf2, bool)
        want[f0: f0 + win] = True
        assert np.array_equal(base, np.repeat(want, uo)), f"{what}: the model's footprint is not {win} whole frames / steps from {f0} on"
        return rule(base, s, ocuts) if rule else base
    sweep(what, mk_gpu, mk_model, x, cuts, where, whole_units,
          combos={"a": [("nan", "re")], "b": [("nan", "im")], "m": [("+inf", "both")], "c": [("nan", "re"), ("-inf", "im")], "d": [("nan", "re")]})


@pytest.mark.parametrize("M,nf1,nf2", CHAN_SHAPES, ids=[f"M{M}-{a}" for M, a, b in CHAN_SHAPES])
@pytest.mark.parametrize("p", [4, 5, 6, 8, 16])
@pytest.mark.parametrize("op", ["ana", "syn"])
def test_firpfbch(ya, op, M, nf1, nf2, p):
    chan_case(ya, op, M, p, nf1, nf2)


@pytest.mark.parametrize("M,nf1,nf2", CHAN_SHAPES, ids=[f"M{M}-{a}" for M, a, b in CHAN_SHAPES])
@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("op", ["ana2", "syn2"])
def test_firpfbch2(ya, op, M, nf1, nf2, m):
    chan_case(ya, op, M, m, nf1, nf2)
