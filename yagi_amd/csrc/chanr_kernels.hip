// chanr_kernels.hip -- rational-oversampling polyphase channelizer multichannel::firpfbchr: M channels spaced 1/M, one
// output per channel every P input samples (1 <= P <= M, oversampling M/P).  firpfbch is P = M, firpfbch2 is P = M/2.
//
// The reference module is empty (see chan_kernels.hip), so the object is defined by closed forms (DESIGN.md section 4,
// "FirPfbChr").  Real prototype h[0 : 2Mm], X = hist ++ x with X[0] = x[0], s = step index counted from the start of the
// stream:
//   analyzer    : u_s[i] = sum_{n < 2m} h[i + nM] X[(s+1)P - 1 - i - nM]                    i in [0, M)
//                 Z_s[(i - sP) mod M] = u_s[i]
//                 y_s[k] = (1/M) sum_b Z_s[b] e^{+j 2 pi b k / M}
//   synthesizer : V_s[b] = sum_k X_s[k] e^{+j 2 pi k b / M}
//                 y[t] = (P/M) sum_{r >= 0, j + rP < 2Mm} h[j + rP] V_{floor(t/P) - r}[t mod M],   j = t mod P
//
// Analyzer, general kernel (any M, P, m): firpfbch2_kernel with a rotation that depends on the step -- a tile of steps per
// workgroup, lanes run over i so that sample reads are contiguous, u goes to LDS at the rotated index, the M-point inverse
// transforms run as Stockham passes in LDS, the 1/M scale is applied at the store.
//
// Analyzer, column kernel (M in {64, 128, 256}, P a multiple of M/8, 2m <= 16): with g = gcd(M, P), Q = M/g and D = P/g the
// steps s = c + Q k of one phase class c share their rotation (Q P = D M is a multiple of M), tap set i of the class
// always meets the same sample column X[(c+1)P - 1 - i + j M], and that column's window slides by D samples from one
// step of the class to the next.  A group of M lanes owns ONE class of one run of steps: lane i keeps its 2m taps and
// the last 2m samples of its column in registers (D coalesced 8-byte loads and 2m packed FMAs per output, no LDS in the
// FIR part).  The Q classes of a run are neighbouring groups, so every sample comes from HBM once and from L1/L2 Q - 1
// times.  Transforms per half tile of 8 class steps through LDS with static radix passes, as in firpfbch2_col_kernel.
//
// Synthesizer: two launches.  The first inverse-transforms the steps of the call into a scratch stream, the second
// combines: output t reads ceil((2Mm - j)/P) rows of one column of it.  The object keeps the last ceil(2Mm/P) - 1
// TRANSFORMED steps as its history.  The one-launch form that transforms a tile's halo again cannot hold small P (M 512,
// P 1, m 1 has a halo of 1023 steps: 8 MiB), so this is the form for every shape.  Whether the halo form is faster at
// P >= M/2 has not been measured (DESIGN.md section 4 keeps it as an open item).
#include <type_traits>

#include "chan_common.hpp"

namespace yagi {

// rotation of step s: (s P) mod M without overflow (M <= 8192)
__host__ __device__ inline int chanr_rot(unsigned long long s, int P, int M) {
    return (int)(((s % (unsigned long long)M) * (unsigned long long)P) % (unsigned long long)M);
}

// ---------------------------------------------------------------------------------------------
// general analyzer
// ---------------------------------------------------------------------------------------------
template <bool POW2>
__global__ void __launch_bounds__(256)
firpfbchr_kernel(const float2 *__restrict__ hist, int hist_len, const float2 *__restrict__ x,
                 const float *__restrict__ h, int M, int P, int p /* 2m */, const float2 *__restrict__ twM,
                 FacList fl, Pow2Plan plan, unsigned long long step0, float2 *__restrict__ y, size_t nsteps, int S) {
    extern __shared__ __align__(16) unsigned char smem[];
    float2 *va = reinterpret_cast<float2 *>(smem);             // S * M
    float2 *vb = va + (size_t)S * M;                           // S * M (Stockham partner)
    float2 *twl = vb + (size_t)S * M;                          // M
    float *hs = reinterpret_cast<float *>(twl + M);            // p * M taps, natural order h[i + n*M]
    const float invM = 1.0f / (float)M;
    const long long x_len = (long long)nsteps * P;
    for (int e = threadIdx.x; e < M; e += 256) twl[e] = twM[e];
    for (int e = threadIdx.x; e < p * M; e += 256) hs[e] = h[e];
    __syncthreads();
    for (size_t tile = blockIdx.x; tile * S < nsteps; tile += gridDim.x) {
        const size_t s0 = tile * S;
        const int ns = (int)((nsteps - s0) < (size_t)S ? (nsteps - s0) : (size_t)S);
        // oldest sample the tile needs: (s0 + 1) P - 1 - (pM - 1)  (>= 0 for interior tiles); newest: (s0 + ns) P - 1 < x_len
        const bool interior = (long long)(s0 + 1) * P - (long long)p * M >= 0;
        const int rot0 = chanr_rot(step0 + s0, P, M);          // rotation of the tile's first step
        for (int e = threadIdx.x; e < ns * M; e += 256) {
            const int sl = e / M, i = e - sl * M;
            const long long top = (long long)(s0 + sl + 1) * P - 1 - i;   // lanes hold consecutive i: a contiguous (descending) run of x
            const float *hp = hs + i;
            float2 acc = make_float2(0.f, 0.f);
            if (interior) {
                const float2 *xp = x + top;
                for (int n = 0; n < p; ++n) {
                    const float hv = hp[n * M];
                    const float2 sv = xp[-(long long)n * M];
                    acc.x = fmaf(sv.x, hv, acc.x);
                    acc.y = fmaf(sv.y, hv, acc.y);
                }
            } else {
                for (int n = 0; n < p; ++n) {
                    const float hv = hp[n * M];
                    const float2 sv = load_hist(hist, hist_len, x, top - (long long)n * M, x_len);
                    acc.x = fmaf(sv.x, hv, acc.x);
                    acc.y = fmaf(sv.y, hv, acc.y);
                }
            }
            const int rot = (int)(((long long)rot0 + (long long)sl * P) % M);
            int b = i - rot;
            if (b < 0) b += M;
            va[sl * M + b] = acc;
        }
        __syncthreads();
        float2 *res = POW2 ? lds_fft_pow2<+1>(va, vb, M, ns, plan, twl, 1)
                           : lds_dft_frames(va, vb, M, ns, fl, twl, 1, true);
        for (int e = threadIdx.x; e < ns * M; e += 256) {
            const float2 v = res[e];
            y[s0 * M + e] = make_float2(v.x * invM, v.y * invM);
        }
        __syncthreads();
    }
}

static size_t chanr_ana_lds(int M, int p, int S) {
    return 2 * (size_t)S * M * sizeof(float2) + (size_t)M * sizeof(float2) + (size_t)p * M * sizeof(float);
}
static size_t chanr_syn_lds(int M, int S) { return (2 * (size_t)S * M + (size_t)M) * sizeof(float2); }
static constexpr size_t kChanrLdsMax = 150 * 1024;

int firpfbchr_check_shape(int M, int P, int m) {
    if (M < 2 || P < 1 || P > M || m < 1) return fail(YAGI_ERR_CONFIG, "firpfbchr: need M >= 2, 1 <= P <= M, m >= 1");
    if (chanr_ana_lds(M, 2 * m, 1) > kChanrLdsMax || chanr_syn_lds(M, 1) > kChanrLdsMax)
        return fail(YAGI_ERR_CONFIG, "firpfbchr: M*m too large for LDS (%d x %d)", M, m);
    return YAGI_OK;
}

static int launch_firpfbchr_general(const cf32 *hist, int hist_len, const cf32 *x, const float *h, int M, int P, int m,
                                    const cf32 *twM, uint64_t step0, cf32 *y, size_t nsteps, hipStream_t st) {
    const int p = 2 * m;
    int S = 4096 / M;
    if (S < 1) S = 1;
    const size_t budget = M >= 512 ? 78 * 1024 : kChanLdsBudget;
    while (S > 1 && chanr_ana_lds(M, p, S) > budget) S /= 2;
    const size_t need = chanr_ana_lds(M, p, S);
    if (need > kChanrLdsMax) return fail(YAGI_ERR_CONFIG, "firpfbchr: M*m too large for LDS (%d x %d)", M, m);
    const bool pow2 = is_pow2(M);
    const void *fn = pow2 ? reinterpret_cast<const void *>(firpfbchr_kernel<true>)
                          : reinterpret_cast<const void *>(firpfbchr_kernel<false>);
    if (need > 64 * 1024) YG_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const size_t tiles = (nsteps + S - 1) / S;
    const unsigned grid = (unsigned)(tiles < 65536 ? tiles : 65536);
    const float2 *fh = reinterpret_cast<const float2 *>(hist), *fx = reinterpret_cast<const float2 *>(x);
    const float2 *ftw = reinterpret_cast<const float2 *>(twM);
    float2 *fy = reinterpret_cast<float2 *>(y);
    if (pow2)
        firpfbchr_kernel<true><<<grid, 256, need, st>>>(fh, hist_len, fx, h, M, P, p, ftw, FacList{0, {0}}, make_pow2_plan(M),
                                                       (unsigned long long)step0, fy, nsteps, S);
    else
        firpfbchr_kernel<false><<<grid, 256, need, st>>>(fh, hist_len, fx, h, M, P, p, ftw, factorize_small(M), Pow2Plan{0, {0}},
                                                        (unsigned long long)step0, fy, nsteps, S);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

// ---------------------------------------------------------------------------------------------
// column analyzer.  PB = built branch length (>= 2m, the taps behind 2m are zero), D = P / gcd(M, P), M = 2^LGM.
// Work unit u = (run r, class c) = (u / Q, u % Q): class steps k < run at the call's steps first + Q k, first = r Q run + c.
// A workgroup holds G = 256/M consecutive units.  Column sample j of lane i is X[(first + 1) P - 1 - i + j M]; class
// step k needs j in (kD - PB, kD] and keeps sample j in ring slot j mod PB.  `run` is a multiple of 16 and PB divides
// 16, so the slots of a half tile are compile-time constants.  Every access is range-checked or proven inside x by the
// unit's `interior` test; a unit past the end of the block loads zeros and stores nothing.
// ---------------------------------------------------------------------------------------------
template <int PB, int D, int LGM>
__global__ void __launch_bounds__(256)
firpfbchr_col_kernel(const float2 *__restrict__ hist, int hist_len, const float2 *__restrict__ x,
                     const float *__restrict__ h, const float2 *__restrict__ twM, unsigned long long step0,
                     int P, int Q, float2 *__restrict__ y, size_t nsteps, int run, int p_real) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int M = 1 << LGM, lgM = LGM, G = 256 / M;
    constexpr int DL = D < PB ? D : PB;                         // D >= PB: the whole window is replaced, only its PB samples are read
    constexpr int R0 = LGM == 6 ? 8 : 16, R1 = M / R0;          // 64 = 8 x 8, 128 = 16 x 8, 256 = 16 x 16
    constexpr int nq = G * kColHalf, lgnq = 8 - LGM + 3;
    constexpr int pitch = col_pitch(M, nq);
    __shared__ long long u_first[G];                            // per unit of the workgroup: the call's step of k = 0
    __shared__ int u_nk[G];                                     // and the class steps that exist
    float2 *va = reinterpret_cast<float2 *>(smem);              // [G units][8 class steps][pitch]
    float2 *vb = va + nq * pitch;
    float2 *twl = vb + nq * pitch;                              // M
    const int g = threadIdx.x >> lgM, i = threadIdx.x & (M - 1);
    for (int e = threadIdx.x; e < M; e += 256) twl[e] = twM[e];
    float hc[PB];
#pragma unroll
    for (int n = 0; n < PB; ++n) hc[n] = n < p_real ? h[i + n * M] : 0.0f;
    const float invM = 1.0f / (float)M;
    const long long x_len = (long long)nsteps * P;
    const long long unit = (long long)blockIdx.x * G + g;
    const long long r = unit / Q;
    const int c = (int)(unit - r * Q);
    const long long first = r * (long long)Q * run + c;
    const long long left = (long long)nsteps - first;
    const long long cnt = left <= 0 ? 0 : (left + Q - 1) / Q;
    const int nk = (int)(cnt < run ? cnt : run);
    if (i == 0) { u_first[g] = first; u_nk[g] = nk; }           // read behind the first barrier of half_tile
    const int rot = chanr_rot(step0 + (unsigned long long)first, P, M);
    const int bidx = (i - rot + M) & (M - 1);
    const long long colbase = (first + 1) * P - 1 - i;
    const bool interior = nk == run && colbase - (long long)(PB - 1) * M >= 0;   // then 0 <= every index <= top of the unit's last step < x_len
    auto ld = [&](long long j) {
        const long long idx = colbase + j * M;
        return interior ? x[idx] : load_hist(hist, hist_len, x, idx, x_len);
    };
    float2 w[PB];
    w[0] = make_float2(0.f, 0.f);
#pragma unroll
    for (int n = 1; n < PB; ++n) w[PB - n] = ld(-n);
    auto half_tile = [&](int t, auto slot0) {
        constexpr int S0 = decltype(slot0)::value;               // ring slot of column sample t D
#pragma unroll
        for (int j = 0; j < kColHalf; ++j) {
#pragma unroll
            for (int d = DL - 1; d >= 0; --d) w[(S0 + j * D - d + 64 * PB) % PB] = ld((long long)(t + j) * D - d);
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int n = 0; n < PB; ++n) {
                const float2 sv = w[(S0 + j * D - n + 64 * PB) % PB];
                acc.x = fmaf(sv.x, hc[n], acc.x);
                acc.y = fmaf(sv.y, hc[n], acc.y);
            }
            va[(g * kColHalf + j) * pitch + bidx] = acc;
        }
        __syncthreads();
        stockham_pass<R0, +1, true>(va, vb, M, 1, nq, twl, 1, true, pitch, lgnq);
        __syncthreads();
        auto put = [&](int q, int k, float2 v) {                 // transform q = unit gq, class step t + fr
            const int gq = q / kColHalf, fr = q - gq * kColHalf;
            if (t + fr < u_nk[gq])
                y[(size_t)(u_first[gq] + (long long)Q * (t + fr)) * M + k] = make_float2(v.x * invM, v.y * invM);
        };
        if constexpr (M / R1 >= 16) {
            // last pass straight from registers to y in 128-byte runs (M = 128, 256); no barrier behind it: the next half
            // tile writes va first, and its own barrier stands between this pass's reads of vb and the next writes to it
            stockham_last_pass_out<R1, +1>(vb, M, nq, twl, 1, true, pitch, put);
        } else {
            stockham_pass<R1, +1, true>(vb, va, M, R0, nq, twl, 1, true, pitch, lgnq);
            __syncthreads();
#pragma unroll
            for (int ii = 0; ii < kColHalf; ++ii) {
                const int e = threadIdx.x + 256 * ii;
                const int q = e >> lgM, k = e & (M - 1);
                put(q, k, va[q * pitch + k]);
            }
            __syncthreads();
        }
    };
    for (int t0 = 0; t0 < run; t0 += kColTile) {
        half_tile(t0, std::integral_constant<int, 0>{});
        half_tile(t0 + kColHalf, std::integral_constant<int, (kColHalf * D) % PB>{});
    }
}

static int gcd_int(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

bool firpfbchr_col_served(int M, int P, int m) {
    return (M == 64 || M == 128 || M == 256) && P >= 1 && P <= M && (8 * P) % M == 0 && m >= 1 && 2 * m <= 16;
}

template <int PB, int D, int LGM>
static int launch_firpfbchr_col(const cf32 *hist, int hist_len, const cf32 *x, const float *h, const cf32 *twM,
                                uint64_t step0, int P, int Q, cf32 *y, size_t nsteps, hipStream_t st, int p_real) {
    constexpr int M = 1 << LGM, G = 256 / M;
    // class steps per unit: about kColWgs workgroups, runs of 16 ... 256 class steps
    size_t run = nsteps / (kColWgs * G);
    run = run / kColTile * kColTile;
    if (run < (size_t)kColTile) run = kColTile;
    if (run > 256) run = 256;
    const size_t nruns = (nsteps + (size_t)Q * run - 1) / ((size_t)Q * run);
    const size_t nblk = (nruns * Q + G - 1) / G;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    const size_t lds = (2 * (size_t)G * kColHalf * col_pitch(M, G * kColHalf) + (size_t)M) * sizeof(float2);
    firpfbchr_col_kernel<PB, D, LGM><<<(unsigned)nblk, 256, lds, st>>>(
        reinterpret_cast<const float2 *>(hist), hist_len, reinterpret_cast<const float2 *>(x), h,
        reinterpret_cast<const float2 *>(twM), (unsigned long long)step0, P, Q, reinterpret_cast<float2 *>(y), nsteps,
        (int)run, p_real);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

template <int PB, int D, class... A>
static int launch_firpfbchr_col_m(int M, A... a) {
    return M == 64 ? launch_firpfbchr_col<PB, D, 6>(a...)
         : M == 128 ? launch_firpfbchr_col<PB, D, 7>(a...)
                    : launch_firpfbchr_col<PB, D, 8>(a...);
}
template <int PB, class... A>
static int launch_firpfbchr_col_d(int D, int M, A... a) {
    switch (D) {
        case 1: return launch_firpfbchr_col_m<PB, 1>(M, a...);
        case 3: return launch_firpfbchr_col_m<PB, 3>(M, a...);
        case 5: return launch_firpfbchr_col_m<PB, 5>(M, a...);
        case 7: return launch_firpfbchr_col_m<PB, 7>(M, a...);
        default: return fail(YAGI_ERR_INTERNAL, "firpfbchr: no column kernel for P/gcd(M,P) = %d", D);
    }
}

// auto (choice 0): the column kernel only where profiles/r13_kbench_chanr.txt shows it ahead of the general one at both
// measured block lengths (2^20 and 2^24 input samples; shorter calls were not measured and stay on the general kernel).
//   D = 1 (P = M/8, M/4, M/2, M): 1.39 ... 5.54x at every M and built branch length; against the general kernel at HALF
//          the taps still >= 1.22x, so the zero-padded lengths 4 < 2m < 16 take it too (2m = 2 was not measured)
//   D = 3: 16 taps 1.52 ... 3.55x; 8 taps 1.08 ... 1.79x at M 64, 128 (M 256: 0.92 at 2^20); 4 taps 0.79 ... 1.35: general
//   D = 5: 16 taps 1.26 ... 2.01x; fewer taps 0.46 ... 1.18: general
//   D = 7: 16 taps at M 64 1.24 ... 1.70x (M 128: 0.64 at 2^20, M 256: 1.05); fewer taps 0.45 ... 1.26: general
// For D > 1 only 2m equal to a built length was measured, and the general kernel at half the taps beats the column
// kernel there, so other 2m stay on the general kernel.  tests/chanr_ref.py auto_takes_column restates this function;
// tests/test_chanr_table_cpu.py holds that restatement to the table, tests/test_gpu_chanr.py this function to it.
static bool firpfbchr_auto_col(int M, int P, int m, size_t nsteps) {
    if ((nsteps + 1) * (size_t)P <= ((size_t)1 << 20)) return false;   // the measured short block: floor(2^20 / P) steps
    const int D = P / gcd_int(M, P), p = 2 * m;
    if (D == 1) return p >= 4;
    if (p == 16) return D == 3 || D == 5 || (D == 7 && M == 64);
    if (p == 8) return D == 3 && M <= 128;
    return false;
}

int launch_firpfbchr(const cf32 *hist, int hist_len, const cf32 *x, const float *h, int M, int P, int m,
                     const cf32 *twM, uint64_t step0, cf32 *y, size_t nsteps, hipStream_t st, int choice, int *ran) {
    if (ran) *ran = 0;
    if (nsteps == 0) return YAGI_OK;
    if (M < 2 || P < 1 || P > M || m < 1) return fail(YAGI_ERR_CONFIG, "firpfbchr: need M >= 2, 1 <= P <= M, m >= 1");
    if ((long long)hist_len != 2ll * M * m - P) return fail(YAGI_ERR_INTERNAL, "firpfbchr: bad history length");
    const bool served = firpfbchr_col_served(M, P, m);
    if (choice == 2 && !served)
        return fail(YAGI_ERR_CONFIG, "firpfbchr: the column kernel serves M in {64,128,256}, P a multiple of M/8, 2m <= 16");
    if (choice == 2 || (choice == 0 && served && firpfbchr_auto_col(M, P, m, nsteps))) {
        const int g = gcd_int(M, P), Q = M / g, D = P / g, p = 2 * m;
        if (ran) *ran = 2;
        // branch lengths between the built sizes take the next one with zero taps behind theirs
        return p <= 4 ? launch_firpfbchr_col_d<4>(D, M, hist, hist_len, x, h, twM, step0, P, Q, y, nsteps, st, p)
             : p <= 8 ? launch_firpfbchr_col_d<8>(D, M, hist, hist_len, x, h, twM, step0, P, Q, y, nsteps, st, p)
                      : launch_firpfbchr_col_d<16>(D, M, hist, hist_len, x, h, twM, step0, P, Q, y, nsteps, st, p);
    }
    if (ran) *ran = 1;
    return launch_firpfbchr_general(hist, hist_len, x, h, M, P, m, twM, step0, y, nsteps, st);
}

// ---------------------------------------------------------------------------------------------
// synthesizer
// ---------------------------------------------------------------------------------------------
template <bool POW2>
__global__ void __launch_bounds__(256)
firpfbchr_syn_transform_kernel(const float2 *__restrict__ x, int M, const float2 *__restrict__ twM, FacList fl,
                               Pow2Plan plan, float2 *__restrict__ v, size_t nsteps, int S) {
    extern __shared__ __align__(16) unsigned char smem[];
    float2 *va = reinterpret_cast<float2 *>(smem);              // S * M
    float2 *vb = va + (size_t)S * M;
    float2 *twl = vb + (size_t)S * M;                           // M
    for (int e = threadIdx.x; e < M; e += 256) twl[e] = twM[e];
    for (size_t tile = blockIdx.x; tile * S < nsteps; tile += gridDim.x) {
        const size_t s0 = tile * S;
        const int ns = (int)((nsteps - s0) < (size_t)S ? (nsteps - s0) : (size_t)S);
        for (int e = threadIdx.x; e < ns * M; e += 256) va[e] = x[s0 * M + e];
        __syncthreads();
        const float2 *res = POW2 ? lds_fft_pow2<+1>(va, vb, M, ns, plan, twl, 1, true)
                                 : lds_dft_frames(va, vb, M, ns, fl, twl, 1, true);
        for (int e = threadIdx.x; e < ns * M; e += 256) v[s0 * M + e] = res[e];
        __syncthreads();
    }
}

int launch_firpfbchr_syn_transform(const cf32 *x, int M, const cf32 *twM, cf32 *v, size_t nsteps, hipStream_t st) {
    if (nsteps == 0) return YAGI_OK;
    int S = 4096 / M;
    if (S < 1) S = 1;
    while (S > 1 && chanr_syn_lds(M, S) > 78 * 1024) S /= 2;
    const size_t need = chanr_syn_lds(M, S);
    if (need > kChanrLdsMax) return fail(YAGI_ERR_CONFIG, "firpfbchr synthesizer: M too large for LDS (%d)", M);
    const bool pow2 = is_pow2(M);
    const void *fn = pow2 ? reinterpret_cast<const void *>(firpfbchr_syn_transform_kernel<true>)
                          : reinterpret_cast<const void *>(firpfbchr_syn_transform_kernel<false>);
    if (need > 64 * 1024) YG_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const size_t tiles = (nsteps + S - 1) / S;
    const unsigned grid = (unsigned)(tiles < 65536 ? tiles : 65536);
    const float2 *fx = reinterpret_cast<const float2 *>(x), *ftw = reinterpret_cast<const float2 *>(twM);
    float2 *fv = reinterpret_cast<float2 *>(v);
    if (pow2)
        firpfbchr_syn_transform_kernel<true><<<grid, 256, need, st>>>(fx, M, ftw, FacList{0, {0}}, make_pow2_plan(M), fv, nsteps, S);
    else
        firpfbchr_syn_transform_kernel<false><<<grid, 256, need, st>>>(fx, M, ftw, factorize_small(M), Pow2Plan{0, {0}}, fv, nsteps, S);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

// one output per lane: neighbouring lanes read neighbouring columns of the same rows (the column index wraps at M), taps
// h[j + rP] in the order r = 0, 1, ...
__global__ void __launch_bounds__(256)
firpfbchr_syn_combine_kernel(const float2 *__restrict__ vhist, int hist_rows, const float2 *__restrict__ v,
                             const float *__restrict__ h, int M, int P, int L /* 2Mm */, int b0 /* (step0 P) mod M */,
                             float scale, float2 *__restrict__ y, size_t nout) {
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < nout; t += (size_t)gridDim.x * blockDim.x) {
        const long long s = (long long)(t / (size_t)P);
        const int j = (int)(t - (size_t)s * P);
        const int b = (int)(((size_t)b0 + t) % (size_t)M);
        // the sum has ceil((2Mm - j)/P) terms -- 1024 at M 512, P 1, m 1, where an f32 accumulator measured 1.2e-6 of the
        // step's norm against 1e-7 for the short sums -- so it is kept in f64 (the loads bound this kernel, not the FMAs)
        double ax = 0.0, ay = 0.0;
        long long row = s;
        for (int l = j; l < L; l += P, --row) {
            float2 sv;
            if (row >= 0) sv = v[(size_t)row * M + b];
            else if (hist_rows + row >= 0) sv = vhist[(size_t)(hist_rows + row) * M + b];
            else sv = make_float2(0.f, 0.f);
            const double hv = (double)h[l];
            ax = fma((double)sv.x, hv, ax);
            ay = fma((double)sv.y, hv, ay);
        }
        y[t] = make_float2((float)(ax * (double)scale), (float)(ay * (double)scale));
    }
}

int launch_firpfbchr_syn_combine(const cf32 *vhist, int hist_rows, const cf32 *v, const float *h, int M, int P, int m,
                                 uint64_t step0, cf32 *y, size_t nsteps, hipStream_t st) {
    const size_t nout = nsteps * (size_t)P;
    if (nout == 0) return YAGI_OK;
    const long long L = 2ll * M * m;
    if ((long long)hist_rows != (L + P - 1) / P - 1) return fail(YAGI_ERR_INTERNAL, "firpfbchr synthesizer: bad history length");
    size_t g = (nout + 255) / 256;
    if (g > 16384) g = 16384;
    firpfbchr_syn_combine_kernel<<<(unsigned)g, 256, 0, st>>>(
        reinterpret_cast<const float2 *>(vhist), hist_rows, reinterpret_cast<const float2 *>(v), h, M, P, (int)L,
        chanr_rot(step0, P, M), (float)P / (float)M, reinterpret_cast<float2 *>(y), nout);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

}  // namespace yagi
