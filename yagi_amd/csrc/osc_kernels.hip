// osc_kernels.hip -- block mixing of Osc (src/nco/osc.rs mix_block_up / mix_block_down) for both schemes.
//
// The reference mixes, then steps, once per sample, so output j of a call uses theta0 + j d_theta mod 2^32: exact u32
// arithmetic, and the low 32 bits of (u32)j * d_theta are that product for any j.  Each lane computes its own phase,
// looks the table up and multiplies, in the reference's f32 order: the NCO reads sin[i] and sin[(i + 256) & 1023] at
// i = ((theta + 2^21) >> 22) & 1023; the VCO reads {value, skew} at theta >> 22 and its quarter-turn neighbour and adds
// (theta & (2^22 - 1)) * skew, two roundings; then num_complex's Mul.  So every output word equals the sequential loop.
//
// The table lives in LDS, staged once per workgroup of a persistent grid: NCO float2 {sin, cos} (8 KiB), one
// ds_read_b64 per sample; VCO float4 {v_sin, s_sin, v_cos, s_cos} (16 KiB), one ds_read_b128.  Across lanes the index is
// an arithmetic progression, which some frequencies put on one bank (the NCO at 16 table entries per sample: every lane
// of a half-wave a different entry of one bank, 32-way).  Measured, that costs nothing at 2^24 and 2^26 samples (within
// 1.5 % of an ordinary frequency, profiles/r05_kbench_osc.txt): the LDS serves one sample per clock per CU even then,
// and HBM asks for about 0.6.  Eight (NCO) or four (VCO) bank-rotated copies of the table measured the same and were
// not kept.
//
// The Makefile builds this file with -ffp-contract=off (the project's -ffp-contract=fast would fuse the VCO lookup and
// the complex product); tests/test_osc_isa_cpu.py checks that the kernels hold no f32 FMA and no scratch.
#pragma clang fp contract(off)

#include "kernels.hpp"
#include "osc_mix.hpp"      // OscEntry, osc_one: shared with the fused kernels of ddc_kernels.hip

namespace yagi {
namespace {

typedef float osc_v2f __attribute__((ext_vector_type(2)));
typedef float osc_v4f __attribute__((ext_vector_type(4)));

// SPL samples per load: 2 (16-byte loads and stores, x and y 16-byte aligned) or 1
template <int VCO, bool DOWN, int SPL>
__global__ void __launch_bounds__(kOscWg)
osc_mix_kernel(const void *tabg, uint32_t theta0, uint32_t dtheta, const cf32 *x, cf32 *y, size_t n) {
    using E = typename OscEntry<VCO>::E;
    __shared__ E tab[1024];
    const int tid = (int)threadIdx.x;
    const E *g = static_cast<const E *>(tabg);
    for (int e = tid; e < 1024; e += kOscWg) tab[e] = g[e];
    __syncthreads();

    constexpr int U = kOscUnroll;
    constexpr size_t tile = (size_t)kOscWg * SPL * U;
#pragma unroll 1
    for (size_t t0 = (size_t)blockIdx.x * tile; t0 < n; t0 += (size_t)gridDim.x * tile) {
        if (t0 + tile <= n) {
            if constexpr (SPL == 2) {
                osc_v4f v[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    v[u] = __builtin_nontemporal_load(
                        reinterpret_cast<const osc_v4f *>(x + t0 + (size_t)(u * kOscWg + tid) * 2));
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const size_t j = t0 + (size_t)(u * kOscWg + tid) * 2;
                    const uint32_t th = theta0 + (uint32_t)j * dtheta;
                    const float2 a = osc_one<VCO, DOWN>(tab, th, v[u].x, v[u].y);
                    const float2 b = osc_one<VCO, DOWN>(tab, th + dtheta, v[u].z, v[u].w);
                    __builtin_nontemporal_store(osc_v4f{a.x, a.y, b.x, b.y}, reinterpret_cast<osc_v4f *>(y + j));
                }
            } else {
                osc_v2f v[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    v[u] = __builtin_nontemporal_load(reinterpret_cast<const osc_v2f *>(x + t0 + (size_t)(u * kOscWg + tid)));
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const size_t j = t0 + (size_t)(u * kOscWg + tid);
                    const float2 a = osc_one<VCO, DOWN>(tab, theta0 + (uint32_t)j * dtheta, v[u].x, v[u].y);
                    __builtin_nontemporal_store(osc_v2f{a.x, a.y}, reinterpret_cast<osc_v2f *>(y + j));
                }
            }
        } else {                                       // the last, partial tile: one guarded sample at a time
#pragma unroll 1
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int e = 0; e < SPL; ++e) {
                    const size_t j = t0 + (size_t)(u * kOscWg + tid) * SPL + e;
                    if (j < n) {
                        const cf32 xv = x[j];
                        const float2 a = osc_one<VCO, DOWN>(tab, theta0 + (uint32_t)j * dtheta, xv.re, xv.im);
                        y[j] = cf32{a.x, a.y};
                    }
                }
            }
        }
    }
}

int osc_cus() {
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cus[dev]) {
        int c = 0;
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
        cus[dev] = c;
    }
    return cus[dev];
}

template <int VCO, bool DOWN, int SPL>
int run_osc(const void *tab, uint32_t theta0, uint32_t dtheta, const cf32 *x, cf32 *y, size_t n, hipStream_t st) {
    const size_t tile = (size_t)kOscWg * SPL * kOscUnroll;
    const size_t tiles = (n + tile - 1) / tile;
    const size_t cap = (size_t)osc_cus() * kOscWgPerCu;
    const unsigned G = (unsigned)(tiles < cap ? tiles : cap);
    osc_mix_kernel<VCO, DOWN, SPL><<<G, kOscWg, 0, st>>>(tab, theta0, dtheta, x, y, n);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

}  // namespace

int launch_osc_mix(int vco, bool down, const void *tab, uint32_t theta0, uint32_t dtheta, const cf32 *x, cf32 *y,
                   size_t n, hipStream_t st) {
    if (n == 0) return YAGI_OK;
    if (((uintptr_t)x | (uintptr_t)y) & 7) return fail(YAGI_ERR_CONFIG, "osc: sample buffers must be 8-byte aligned");
    const bool wide = (((uintptr_t)x | (uintptr_t)y) & 15) == 0;     // 16-byte accesses need both 16-byte aligned
    if (!vco) {
        if (!down) return wide ? run_osc<0, false, 2>(tab, theta0, dtheta, x, y, n, st)
                               : run_osc<0, false, 1>(tab, theta0, dtheta, x, y, n, st);
        return wide ? run_osc<0, true, 2>(tab, theta0, dtheta, x, y, n, st)
                    : run_osc<0, true, 1>(tab, theta0, dtheta, x, y, n, st);
    }
    if (!down) return wide ? run_osc<1, false, 2>(tab, theta0, dtheta, x, y, n, st)
                           : run_osc<1, false, 1>(tab, theta0, dtheta, x, y, n, st);
    return wide ? run_osc<1, true, 2>(tab, theta0, dtheta, x, y, n, st)
                : run_osc<1, true, 1>(tab, theta0, dtheta, x, y, n, st);
}

}  // namespace yagi
