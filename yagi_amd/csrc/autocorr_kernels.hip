// autocorr_kernels.hip -- Autocorr (yagi_hip.h; src/filter/autocorr.rs is an empty file): over a block, for every sample
// n, rxx[n] = sum_i X[n-W+1+i] conj(X[n-W+1+i-d]) and energy[n] = sum_i |X[n-W+1+i]|^2, i = 0 .. W-1 in that order from
// +0.0, every product and every add rounded on its own -- the reference's Window and dotprod composed.
//
// autocorr_kernel<T, ENERGY>: a workgroup of 256 lanes owns kAutocorrTile consecutive outputs.  ac_tile_sums
// (autocorr_tile.hpp, which describes the staging, the LDS layout and the rounding points) leaves every lane with the
// sums of its kAutocorrR consecutive outputs; they go back through LDS, where the staged terms were, and leave as
// contiguous stores.
//
// Every global access is guarded by the block length: x is read in [0, nb), rxx / energy written in [0, nb), the
// history read and written in [0, W + d).
//
// The Makefile builds this file with -ffp-contract=off; tests/test_autocorr_isa_cpu.py checks that the kernels hold no
// f32 FMA and no scratch.
#pragma clang fp contract(off)

#include "autocorr_tile.hpp"

namespace yagi {
namespace {

template <class T, bool ENERGY>
__global__ void __launch_bounds__(kWg) autocorr_kernel(const T *__restrict__ hist, T *__restrict__ hist_next,
                                                       const T *__restrict__ x, size_t nb, T *__restrict__ rxx,
                                                       float *__restrict__ energy, int W, int d) {
    using S = AcShape<T, ENERGY>;
    constexpr bool CPLX = S::CPLX, SEP_E = S::SEP_E;
    using X = typename S::X;
    __shared__ __attribute__((aligned(16))) float s_lds[S::kWordsV + S::kWordsE];
    float *const s_v = s_lds, *const s_e = s_lds + S::kWordsV;

    const int tid = (int)threadIdx.x;
    const size_t t0 = (size_t)blockIdx.x * kT;
    const int cnt = (int)std::min((size_t)kT, nb - t0);             // outputs of this tile
    typename S::V acc[kR];
    float en[SEP_E ? kR : 1];
    ac_tile_sums<T, ENERGY>(s_lds, hist, hist_next, x, nb, W, d, t0, cnt, acc, en);
    __syncthreads();                                                // the terms are read: the outputs go where they were

    // rxx at s_v[0 ..), energy at s_e[0 ..) or, for rrrf, behind rxx at s_v[kT ..)
    float *so = s_v, *eo = SEP_E ? s_e : s_v + kT;
#pragma unroll
    for (int r = 0; r < kR; r += 4) {
        const int o = tid * kR + r;
        if constexpr (CPLX) {
            *reinterpret_cast<ac_v4f *>(so + 2 * o) = ac_v4f{acc[r].x, acc[r].y, acc[r + 1].x, acc[r + 1].y};
            *reinterpret_cast<ac_v4f *>(so + 2 * o + 4) = ac_v4f{acc[r + 2].x, acc[r + 2].y, acc[r + 3].x, acc[r + 3].y};
            if constexpr (ENERGY) *reinterpret_cast<ac_v4f *>(eo + o) = ac_v4f{en[r], en[r + 1], en[r + 2], en[r + 3]};
        } else if constexpr (ENERGY) {
            *reinterpret_cast<ac_v4f *>(so + o) = ac_v4f{acc[r].x, acc[r + 1].x, acc[r + 2].x, acc[r + 3].x};
            *reinterpret_cast<ac_v4f *>(eo + o) = ac_v4f{acc[r].y, acc[r + 1].y, acc[r + 2].y, acc[r + 3].y};
        } else {
            *reinterpret_cast<ac_v4f *>(so + o) = ac_v4f{acc[r], acc[r + 1], acc[r + 2], acc[r + 3]};
        }
    }
    __syncthreads();

    X *yt = reinterpret_cast<X *>(rxx) + t0;
    const X *sx = reinterpret_cast<const X *>(so);
    for (int i = tid; i < cnt; i += kWg) yt[i] = sx[i];
    if constexpr (ENERGY) {
        float *et = energy + t0;
        for (int i = tid; i < cnt; i += kWg) et[i] = eo[i];
    }
}

}  // namespace

template <class T>
void autocorr_host(const T *h, int W, int d, T *rxx, float *energy) {
    constexpr bool CPLX = sizeof(T) == 2 * sizeof(float);
    const float *a = reinterpret_cast<const float *>(h + d), *b = reinterpret_cast<const float *>(h);
    float re = 0.0f, im = 0.0f, en = 0.0f;
    for (int i = 0; i < W; ++i) {
        if constexpr (CPLX) {
            const float rr = a[2 * i] * b[2 * i], ii = a[2 * i + 1] * b[2 * i + 1];
            const float ir = a[2 * i + 1] * b[2 * i], ri = a[2 * i] * b[2 * i + 1];
            const float pr = rr + ii, pi = ir - ri;
            re = re + pr;
            im = im + pi;
            const float er = a[2 * i] * a[2 * i], ei = a[2 * i + 1] * a[2 * i + 1];
            const float e = er + ei;
            en = en + e;
        } else {
            const float p = a[i] * b[i];
            re = re + p;
            const float e = a[i] * a[i];
            en = en + e;
        }
    }
    float *out = reinterpret_cast<float *>(rxx);
    out[0] = re;
    if constexpr (CPLX) out[1] = im;
    *energy = en;
}
template void autocorr_host<float>(const float *, int, int, float *, float *);
template void autocorr_host<cf32>(const cf32 *, int, int, cf32 *, float *);

template <class T>
int launch_autocorr(int W, int d, const T *hist, T *hist_next, const T *x, size_t nb, T *rxx, float *energy,
                    hipStream_t st) {
    if (nb == 0) return YAGI_OK;
    if (W < 1 || W > kAutocorrWmax || d < 0 || d > kAutocorrDmax)
        return fail(YAGI_ERR_INTERNAL, "autocorr: (window_size, delay) out of range");
    const size_t tiles = (nb + kT - 1) / kT;
    if (tiles > 0x7fffffffu) return fail(YAGI_ERR_CONFIG, "autocorr: block too long (%zu samples)", nb);
    if (energy)
        autocorr_kernel<T, true><<<(unsigned)tiles, kWg, 0, st>>>(hist, hist_next, x, nb, rxx, energy, W, d);
    else
        autocorr_kernel<T, false><<<(unsigned)tiles, kWg, 0, st>>>(hist, hist_next, x, nb, rxx, nullptr, W, d);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}
template int launch_autocorr<float>(int, int, const float *, float *, const float *, size_t, float *, float *, hipStream_t);
template int launch_autocorr<cf32>(int, int, const cf32 *, cf32 *, const cf32 *, size_t, cf32 *, float *, hipStream_t);

}  // namespace yagi
