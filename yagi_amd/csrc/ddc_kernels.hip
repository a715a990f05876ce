// ddc_kernels.hip -- Ddc and Duc: the oscillator mix of osc_kernels.hip fused into the decimator and interpolator
// kernels of fir_kernels.hip, one launch instead of two and no full-rate stream through HBM in between.
//
//   Ddc  y = FirDecimationFilter(Osc.mix_block_down(x)):  sample x[j] of the call is mixed with the phase word
//        theta0 + (u32)j * d_theta ON ITS WAY INTO LDS, once; samples taken from the carried window were mixed by the
//        call that staged them and are copied.  The kernel's write_next_window step leaves the MIXED tail of the block
//        as the next window.  Bodies: fir_decim_consec_body (all three staging branches) and fir_block_body<K, true>.
//   Duc  y = Osc.mix_block_up(FirInterpolationFilter(x)):  output n*I + b is mixed with theta0 + (u32)(n*I + b) * d_theta
//        at its store.  The window holds the unmixed inputs.  Bodies: firpfb_fewbranch_body, firpfb_all_body (both
//        tap-staging variants).
//
// The kernel bodies are those of the plain kernels (fir_bodies.hpp), chosen by the same fir_block_plan /
// firpfb_all_plan, so a shape reaches the same (NT, R) instantiation and the same accumulation order fused or not; the
// mix is osc_one (osc_mix.hpp).  Together: every output word equals the two-launch composition's.
//
// The oscillator table sits in LDS behind the span: 8 KiB (NCO float2 {sin, cos}) or 16 KiB (VCO float4).  The span
// keeps the plain kernels' 48 KiB budget -- that is what fixes (NT, R) -- and span + table must fit the 64 KiB a
// workgroup may ask for (kDdcLdsLimit); a shape that does not fit, or whose plan is a kernel without a staged span, is
// not served and the object runs two launches.
//
// The Makefile builds this file with -ffp-contract=off, as it does osc_kernels.hip: the VCO lookup and the complex
// product of the mix keep two roundings.  The FIR sums of the bodies go through mac / mul of devmath.hpp, which call
// fmaf explicitly or are single products, so they are the same instructions under either setting.
#pragma clang fp contract(off)

#include "fir_bodies.hpp"
#include "kernels.hpp"
#include "osc_mix.hpp"

namespace yagi {
namespace {

constexpr size_t kDdcLdsLimit = 64 * 1024;

template <int VCO, bool DOWN>
struct OscMixFn {
    const typename OscEntry<VCO>::E *tab;      // in LDS
    uint32_t theta0, dtheta;
    __device__ __forceinline__ cf32 operator()(cf32 v, long long idx) const {
        const float2 a = osc_one<VCO, DOWN>(tab, theta0 + (uint32_t)idx * dtheta, v.re, v.im);
        return cf32{a.x, a.y};
    }
};

constexpr size_t osc_table_bytes(int vco) { return vco ? 1024 * sizeof(float4) : 1024 * sizeof(float2); }
inline size_t round16(size_t b) { return (b + 15) / 16 * 16; }

// the table into LDS at smem + off, then a barrier: the bodies mix while they stage
template <int VCO, bool DOWN, int NT>
__device__ __forceinline__ OscMixFn<VCO, DOWN> stage_osc(const void *tabg, unsigned off, uint32_t theta0, uint32_t dtheta) {
    using E = typename OscEntry<VCO>::E;
    extern __shared__ __align__(16) unsigned char smem[];
    E *tab = reinterpret_cast<E *>(smem + off);
    const E *g = static_cast<const E *>(tabg);
    for (int e = threadIdx.x; e < 1024; e += NT) tab[e] = g[e];
    __syncthreads();
    return OscMixFn<VCO, DOWN>{tab, theta0, dtheta};
}

struct OscArgs {
    const void *tab;        // device table of the scheme (host.cpp: osc_device_table)
    uint32_t theta0, dtheta;
    unsigned lds_off;       // byte offset of the table in the workgroup's LDS
};

template <class K, int NT, int R, int VCO>
__global__ void __launch_bounds__(NT)
ddc_decim_consec_kernel(const cf32 *__restrict__ win, const cf32 *__restrict__ x, const typename K::C *__restrict__ taps,
                        int L, int M, typename K::C scale, cf32 *__restrict__ y, size_t ny, int pitch,
                        cf32 *__restrict__ win_next, OscArgs o) {
    const auto mix = stage_osc<VCO, true, NT>(o.tab, o.lds_off, o.theta0, o.dtheta);
    fir_decim_consec_body<K, NT, R>(win, x, taps, L, M, scale, y, ny, pitch, win_next, mix);
}

template <class K, int VCO>
__global__ void __launch_bounds__(kFirBlock)
ddc_block_kernel(const cf32 *__restrict__ win, const cf32 *__restrict__ x, const typename K::C *__restrict__ taps, int L,
                 int M, typename K::C scale, cf32 *__restrict__ y, size_t ny, int tile, long long x_len,
                 cf32 *__restrict__ win_next, OscArgs o) {
    const auto mix = stage_osc<VCO, true, kFirBlock>(o.tab, o.lds_off, o.theta0, o.dtheta);
    fir_block_body<K, true>(win, x, taps, L, M, scale, y, ny, tile, x_len, win_next, mix);
}

template <class K, bool TAPS_LDS, int VCO>
__global__ void __launch_bounds__(256)
duc_all_kernel(const cf32 *__restrict__ win, const cf32 *__restrict__ x, const typename K::C *__restrict__ hb, int nf,
               int Ls, typename K::C scale, cf32 *__restrict__ y, size_t n, cf32 *__restrict__ win_next, OscArgs o) {
    const auto mix = stage_osc<VCO, false, 256>(o.tab, o.lds_off, o.theta0, o.dtheta);
    firpfb_all_body<K, TAPS_LDS>(win, x, hb, nf, Ls, scale, y, n, win_next, mix);
}

template <class K, int VCO>
__global__ void __launch_bounds__(256)
duc_fewbranch_kernel(const cf32 *__restrict__ win, const cf32 *__restrict__ x, const typename K::C *__restrict__ hb,
                     int nf, int Ls, typename K::C scale, cf32 *__restrict__ y, size_t n, cf32 *__restrict__ win_next,
                     OscArgs o) {
    const auto mix = stage_osc<VCO, false, 256>(o.tab, o.lds_off, o.theta0, o.dtheta);
    firpfb_fewbranch_body<K>(win, x, hb, nf, Ls, scale, y, n, win_next, mix);
}

template <class K, int NT, int R, int VCO>
int run_ddc_decim(const cf32 *win, const cf32 *x, const typename K::C *taps, int L, int M, typename K::C scale, cf32 *y,
                  size_t ny, hipStream_t st, cf32 *win_next, const FirBlockPlan &p, OscArgs o) {
    constexpr int TILE = NT * R;
    const int pitch = decim_consec_pitch(TILE, L, M, R);
    const size_t nblk = (ny + TILE - 1) / TILE;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    ddc_decim_consec_kernel<K, NT, R, VCO><<<(unsigned)nblk, NT, round16(p.lds) + osc_table_bytes(VCO), st>>>(
        win, x, taps, L, M, scale, y, ny, pitch, win_next, o);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

template <class K, int VCO>
int run_ddc(const cf32 *win, const cf32 *x, const typename K::C *taps, int L, int M, typename K::C scale, cf32 *y,
            size_t ny, hipStream_t st, cf32 *win_next, const FirBlockPlan &p, OscArgs o) {
    if (p.kind == kFirPlanDecim) {
        if (p.nt == 256 && p.r == 8) return run_ddc_decim<K, 256, 8, VCO>(win, x, taps, L, M, scale, y, ny, st, win_next, p, o);
        if (p.nt == 256 && p.r == 4) return run_ddc_decim<K, 256, 4, VCO>(win, x, taps, L, M, scale, y, ny, st, win_next, p, o);
        if (p.nt == 128 && p.r == 4) return run_ddc_decim<K, 128, 4, VCO>(win, x, taps, L, M, scale, y, ny, st, win_next, p, o);
        if (p.nt == 64 && p.r == 8) return run_ddc_decim<K, 64, 8, VCO>(win, x, taps, L, M, scale, y, ny, st, win_next, p, o);
        return run_ddc_decim<K, 64, 4, VCO>(win, x, taps, L, M, scale, y, ny, st, win_next, p, o);
    }
    const size_t nblk = (ny + p.tile - 1) / p.tile;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    ddc_block_kernel<K, VCO><<<(unsigned)nblk, kFirBlock, round16(p.lds) + osc_table_bytes(VCO), st>>>(
        win, x, taps, L, M, scale, y, ny, p.tile, (long long)(ny * (size_t)M), win_next, o);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

template <class K, int VCO>
int run_duc(const cf32 *win, const cf32 *x, const typename K::C *hb, int nf, int Ls, typename K::C scale, cf32 *y,
            size_t n, hipStream_t st, cf32 *win_next, const FirPfbPlan &p, OscArgs o) {
    const size_t nblk = p.kind == kPfbPlanFew ? (n + 255) / 256 : (n + kPfbTN - 1) / kPfbTN;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    const size_t lds = round16(p.lds) + osc_table_bytes(VCO);
    if (p.kind == kPfbPlanFew)
        duc_fewbranch_kernel<K, VCO><<<(unsigned)nblk, 256, lds, st>>>(win, x, hb, nf, Ls, scale, y, n, win_next, o);
    else if (p.kind == kPfbPlanTapsLds)
        duc_all_kernel<K, true, VCO><<<(unsigned)nblk, 256, lds, st>>>(win, x, hb, nf, Ls, scale, y, n, win_next, o);
    else
        duc_all_kernel<K, false, VCO><<<(unsigned)nblk, 256, lds, st>>>(win, x, hb, nf, Ls, scale, y, n, win_next, o);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

}  // namespace

template <class K>
bool ddc_fused_serves(int L, int M, size_t ny, int vco) {
    if (L <= 0 || M < 2 || ny == 0) return false;
    const FirBlockPlan p = fir_block_plan(sizeof(cf32), L, M, ny, 0);
    if (p.kind != kFirPlanDecim && p.kind != kFirPlanStaged) return false;
    return round16(p.lds) + osc_table_bytes(vco) <= kDdcLdsLimit;
}

template <class K>
int launch_ddc_block(const cf32 *win, const cf32 *x, const typename K::C *taps, int L, int M, typename K::C scale,
                     cf32 *y, size_t ny, hipStream_t st, cf32 *win_next, int vco, const void *tab, uint32_t theta0,
                     uint32_t dtheta) {
    if (ny == 0) return YAGI_OK;
    if (!ddc_fused_serves<K>(L, M, ny, vco)) return fail(YAGI_ERR_INTERNAL, "ddc: no fused kernel for this shape");
    if (((uintptr_t)x | (uintptr_t)y) & 7) return fail(YAGI_ERR_CONFIG, "ddc: sample buffers must be 8-byte aligned");
    const FirBlockPlan p = fir_block_plan(sizeof(cf32), L, M, ny, 0);
    const OscArgs o{tab, theta0, dtheta, (unsigned)round16(p.lds)};
    return vco ? run_ddc<K, 1>(win, x, taps, L, M, scale, y, ny, st, win_next, p, o)
               : run_ddc<K, 0>(win, x, taps, L, M, scale, y, ny, st, win_next, p, o);
}

template <class K>
bool duc_fused_serves(int nf, int Ls, int vco) {
    const FirPfbPlan p = firpfb_all_plan(sizeof(cf32), sizeof(typename K::C), nf, Ls);
    if (p.kind == kPfbPlanNone) return false;
    return round16(p.lds) + osc_table_bytes(vco) <= kDdcLdsLimit;
}

template <class K>
int launch_duc_all(const cf32 *win, const cf32 *x, const typename K::C *hb, int nf, int Ls, typename K::C scale,
                   cf32 *y, size_t n, hipStream_t st, cf32 *win_next, int vco, const void *tab, uint32_t theta0,
                   uint32_t dtheta) {
    if (n == 0) return YAGI_OK;
    if (!duc_fused_serves<K>(nf, Ls, vco)) return fail(YAGI_ERR_INTERNAL, "duc: no fused kernel for this shape");
    if (((uintptr_t)x | (uintptr_t)y) & 7) return fail(YAGI_ERR_CONFIG, "duc: sample buffers must be 8-byte aligned");
    const FirPfbPlan p = firpfb_all_plan(sizeof(cf32), sizeof(typename K::C), nf, Ls);
    const OscArgs o{tab, theta0, dtheta, (unsigned)round16(p.lds)};
    return vco ? run_duc<K, 1>(win, x, hb, nf, Ls, scale, y, n, st, win_next, p, o)
               : run_duc<K, 0>(win, x, hb, nf, Ls, scale, y, n, st, win_next, p, o);
}

template bool ddc_fused_serves<CRCF>(int, int, size_t, int);
template bool ddc_fused_serves<CCCF>(int, int, size_t, int);
template int launch_ddc_block<CRCF>(const cf32 *, const cf32 *, const float *, int, int, float, cf32 *, size_t, hipStream_t,
                                    cf32 *, int, const void *, uint32_t, uint32_t);
template int launch_ddc_block<CCCF>(const cf32 *, const cf32 *, const cf32 *, int, int, cf32, cf32 *, size_t, hipStream_t,
                                    cf32 *, int, const void *, uint32_t, uint32_t);
template bool duc_fused_serves<CRCF>(int, int, int);
template bool duc_fused_serves<CCCF>(int, int, int);
template int launch_duc_all<CRCF>(const cf32 *, const cf32 *, const float *, int, int, float, cf32 *, size_t, hipStream_t,
                                  cf32 *, int, const void *, uint32_t, uint32_t);
template int launch_duc_all<CCCF>(const cf32 *, const cf32 *, const cf32 *, int, int, cf32, cf32 *, size_t, hipStream_t,
                                  cf32 *, int, const void *, uint32_t, uint32_t);

}  // namespace yagi
