// fir_kernels.hip -- direct-form FIR kernels for all three type combinations:
//   FirFilter::execute_block        (src/filter/fir/firfilt.rs:267-278)      M = 1
//   FirDecimationFilter::execute_block (src/filter/fir/firdecim.rs:179-205)  stride M
//   FirPfbFilter branch forms       (src/filter/fir/firpfb.rs:255-301)
//
// Data layout in HBM: samples contiguous (interleaved {re,im} for complex), taps h[0..L) in
// natural order, the filter state ("window") = the L samples preceding x[0], oldest first
// (what Window::read() returns, window.rs:66-68).  X below is the virtual stream win ++ x with
// X[0] = x[0]; the kernels never materialise it.
//
// fir_block_kernel: one workgroup produces `tile` consecutive outputs.  It stages the input
// span ((tile-1)*M + L samples, coalesced) and the taps in LDS, then every lane accumulates R
// outputs that are 256 apart, so at tap k the wave reads 64 consecutive samples (conflict-free
// ds_read) and one broadcast tap.  Algorithmic HBM traffic: sizeof(T)*(M + 1) bytes per output
// (+ the (L-1)-sample halo per tile, which is L2-resident).  This is the general kernel (any
// L, M, type); the crcf M=1 hot case has an MFMA version in fir_mfma.hip.
//
// The bodies of fir_block_kernel, fir_decim_consec_kernel and the two bank kernels, and the choice among them, live in
// fir_bodies.hpp: ddc_kernels.hip runs the same bodies with an oscillator mix fused in.
#include <type_traits>

#include "devmath.hpp"
#include <cstdlib>

#include "fir_bodies.hpp"
#include "kernels.hpp"

namespace yagi {

template <class K, bool STAGE>
__global__ void __launch_bounds__(kFirBlock)
fir_block_kernel(const typename K::T *__restrict__ win, const typename K::T *__restrict__ x,
                 const typename K::C *__restrict__ taps, int L, int M, typename K::C scale,
                 typename K::T *__restrict__ y, size_t ny, int tile, long long x_len,
                 typename K::T *__restrict__ win_next) {
    fir_block_body<K, STAGE>(win, x, taps, L, M, scale, y, ny, tile, x_len, win_next, FirNoMix{});
}

// one chunk of eight samples of the rrrf body below (FULL: all eight inside d <= L-8; else wave-uniform guards)
template <bool FULL>
__device__ __forceinline__ void fir_consec_rrrf_chunk(v2f (&a2)[4], const float *xl, const float *__restrict__ taps,
                                                      int L, int Lp, int c) {
    const int d0 = 1 + 8 * c;                                // samples d0 .. d0+7 live in one pad group:
    const float *rb = xl + 9 * ((Lp >> 3) - c - 1);          // sample d0 + u at rb[7 - u]
    v2f g2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) g2[i] = v2f{rb[2 * i], rb[2 * i + 1]};
    float ht[15];
#pragma unroll
    for (int i = 0; i < 15; ++i) ht[i] = taps[(FULL || d0 + i < L) ? d0 + i : L - 1];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int gi = 7 - u;
        if (FULL || d0 + u <= L - 8) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const v2f hp = v2f{ht[u + 2 * p], ht[u + 2 * p + 1]};
                if (gi & 1)
                    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(a2[p]) : "v"(g2[gi >> 1]), "s"(hp));
                else
                    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(a2[p]) : "v"(g2[gi >> 1]), "s"(hp));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// rrrf body of fir_consec_kernel.  Real samples would have to sit in adjacent registers in exactly the pairing a
// packed FMA wants, and a sliding window breaks that on every other tap (the compiler patches it with one v_mov per
// two v_pk_fma_f32).  Turned around -- outer loop over the SAMPLE, which is broadcast to both halves (op_sel), packed
// operand = two adjacent TAPS from an SGPR pair -- no register pairing of samples is needed at all:
//     (y[8l+2p], y[8l+2p+1]) += X[8l - d] * (h[d+2p], h[d+2p+1]),   p < 4,  d = 1 .. L-8   (all 8 taps inside h)
// Samples come from LDS eight at a time (one pad group of the lane's row), taps through the scalar cache.  The
// 15 edge samples (d = -7..0 and d > L-8), where only some of the lane's outputs have a tap, are two static
// triangles of scalar FMAs.  Every output still adds its taps in the order k = 0, 1, .. L-1 with one FMA each: bit-identical
// to fir_block_kernel, and no tap outside h is ever multiplied.  xl = lane's row (slot of sample 8l - d:
// e + (e >> 3), e = Lp - d).  Needs L >= 16.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void fir_consec_rrrf_body(const float *xl, const float *__restrict__ taps, int L, int Lp,
                                                     float (&acc)[8]) {
    v2f a2[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) a2[p] = v2f{0.f, 0.f};
    // head: samples X[8l + j], j = 7 .. 0 (d = -j); output r >= j takes tap h[r - j] -- a static triangle
    {
        const float *rb = xl + 9 * (Lp >> 3);                    // sample 8l + j at rb[j]
        float g[8], h0[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { g[j] = rb[j]; h0[j] = taps[j]; }
#pragma unroll
        for (int j = 7; j >= 0; --j)
#pragma unroll
            for (int r = j; r < 8; ++r) a2[r >> 1][r & 1] = fmaf(g[j], h0[r - j], a2[r >> 1][r & 1]);
    }
    // body: d = 1 .. L-8 in chunks of 8 samples (fir_consec_rrrf_chunk); the last chunk may be partial
    const int nch = (L - 8) >> 3;
#pragma unroll 1
    for (int c = 0; c < nch; ++c) fir_consec_rrrf_chunk<true>(a2, xl, taps, L, Lp, c);
    if (((L - 8) & 7) != 0) fir_consec_rrrf_chunk<false>(a2, xl, taps, L, Lp, nch);
    // tail: d = L-8+t, t = 1 .. 7; output r <= 7 - t takes tap h[L-8+t+r] -- the other static triangle
    {
        float hl[8];
#pragma unroll
        for (int i = 1; i < 8; ++i) hl[i] = taps[L - 8 + i];
#pragma unroll
        for (int t = 1; t < 8; ++t) {
            const int e = Lp - (L - 8 + t);
            const float xv = xl[e + (e >> 3)];
#pragma unroll
            for (int r = 0; r + t < 8; ++r) a2[r >> 1][r & 1] = fmaf(xv, hl[t + r], a2[r >> 1][r & 1]);
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = a2[r >> 1][r & 1];
}

// ---------------------------------------------------------------------------------------------
// M = 1 direct form with register reuse (all three type combinations): a lane owns 8 CONSECUTIVE outputs and walks
// the taps with an 8-sample register window that slides by one sample per tap -- one LDS read per 8 multiply-
// accumulates instead of one per MAC (the interleaved-output kernel above is bound by exactly that read).
// Tile = 256 lanes x 8 outputs; the span is staged with one pad element after every 8 samples, so that the 64 lanes
// of a wave (8 samples = 9 slots apart) hit distinct banks.  The window geometry is that of Lp = roundup(L, 8) taps
// (the span reaches up to 7 samples further back); the taps past L are skipped, never multiplied, so a NaN in the
// stream poisons exactly the outputs it poisons in the reference.  Taps come through the scalar cache 8 at a time.  Same sums in the same tap order as fir_block_kernel (bit-identical results).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int consec_pad(int i) { return i + (i >> 3); }

template <class K>
__global__ void __launch_bounds__(256)
fir_consec_kernel(const typename K::T *__restrict__ win, const typename K::T *__restrict__ x,
                  const typename K::C *__restrict__ taps, int L, typename K::C scale,
                  typename K::T *__restrict__ y, size_t ny, typename K::T *__restrict__ win_next) {
    using T = typename K::T;
    using C = typename K::C;
    extern __shared__ __align__(16) unsigned char smem[];
    T *xs = reinterpret_cast<T *>(smem);
    write_next_window(win, x, ny, L, win_next);
    const int Lp = (L + 7) & ~7;
    const size_t o0 = (size_t)blockIdx.x * kConsecTile;
    const int nt = (int)((ny - o0) < (size_t)kConsecTile ? (ny - o0) : (size_t)kConsecTile);
    const long long base = (long long)o0 - Lp;                  // stream index of span sample 0: a multiple of 8,
    const int span = kConsecTile + Lp;                          // so an aligned x is read 16 bytes per lane
    // X = win ++ x; indices before the window (no tap reaches them) and past the end of x read as zero
    if (base >= 0 && base + span <= (long long)ny && (reinterpret_cast<unsigned long long>(x) & 15ull) == 0) {
        constexpr int VEC = 16 / sizeof(T);
        const float4 *src = reinterpret_cast<const float4 *>(x + base);
        const int nvec = span / VEC;
        for (int v0 = threadIdx.x; v0 < nvec; v0 += 4 * 256) {  // four 16-byte loads in flight per lane
            float4 q[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) q[b] = src[v0 + 256 * b < nvec ? v0 + 256 * b : nvec - 1];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int v = v0 + 256 * b;
                if (v < nvec) {
                    T *dst = xs + consec_pad(v * VEC);           // VEC divides 8: the elements share a pad group
                    const T *e = reinterpret_cast<const T *>(&q[b]);
#pragma unroll
                    for (int c = 0; c < VEC; ++c) dst[c] = e[c];
                }
            }
        }
    } else {
        for (int i = threadIdx.x; i < span; i += 256) {
            const long long idx = base + i;
            T v = zero_of<T>();
            if (idx >= 0) { if (idx < (long long)ny) v = x[idx]; }
            else if (idx >= -(long long)L) v = win[L + idx];
            xs[consec_pad(i)] = v;
        }
    }
    __syncthreads();
    const int l = threadIdx.x;
    T acc[kConsecR], w[kConsecR];
#pragma unroll
    for (int r = 0; r < kConsecR; ++r) acc[r] = zero_of<T>();
    // at tap k (j = Lp-1-k) output r of the lane needs span sample 8l + q with q = r + j + 1, i.e. slot
    // 9l + q + (q >> 3); it is kept in w[(r + j) & 7]
    const T *xl = xs + 9 * l;
    bool done = false;
    if constexpr (K::id == 0) {
        if (L >= 16) {                                           // block-uniform
            fir_consec_rrrf_body(xl, taps, L, Lp, acc);
            done = true;
        }
    }
    if (!done) {
    {
        const int j = Lp - 1;                                    // j & 7 == 7
#pragma unroll
        for (int r = 1; r < kConsecR; ++r) w[(r + 7) & 7] = xl[(r + j + 1) + ((r + j + 1) >> 3)];
    }
    auto eight_taps = [&](const C (&hk)[8], int k0, auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        const int jb = Lp - 8 - k0;                              // multiple of 8: j = jb + 7 - u
        const T *xb = xl + jb + (jb >> 3);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            w[(7 - u) & 7] = xb[(8 - u) + ((8 - u) >> 3)];       // the window's new lowest sample (r = 0, q = j + 1)
            if (FULL || k0 + u < L) {                            // wave-uniform: taps past L are skipped, not zeroed
#pragma unroll
                for (int r = 0; r < kConsecR; ++r) acc[r] = mac(acc[r], w[(r + 7 - u) & 7], hk[u]);
            }
        }
    };
    int k0 = 0;
    for (; k0 + 8 <= L; k0 += 8) {
        C hk[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) hk[u] = taps[k0 + u];
        eight_taps(hk, k0, std::true_type{});
    }
    if (k0 < L) {
        C hk[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) hk[u] = taps[k0 + u < L ? k0 + u : L - 1];
        eight_taps(hk, k0, std::false_type{});
    }
    }
    const int o = kConsecR * l;
    if (o + kConsecR <= nt) {
#pragma unroll
        for (int r = 0; r < kConsecR; ++r) y[o0 + o + r] = mul(acc[r], scale);
    } else {
#pragma unroll
        for (int r = 0; r < kConsecR; ++r)
            if (o + r < nt) y[o0 + o + r] = mul(acc[r], scale);
    }
}

template <class K>
static int launch_fir_consec(const typename K::T *win, const typename K::T *x, const typename K::C *taps, int L,
                             typename K::C scale, typename K::T *y, size_t ny, hipStream_t st,
                             typename K::T *win_next) {
    using T = typename K::T;
    const size_t lds = fir_consec_lds(sizeof(T), L);
    const size_t nblk = (ny + kConsecTile - 1) / kConsecTile;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    fir_consec_kernel<K><<<(unsigned)nblk, 256, lds, st>>>(win, x, taps, L, scale, y, ny, win_next);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

// Decimator (M >= 2) with the same register window, one decimation phase at a time (fir_bodies.hpp)
template <class K, int NT, int R>
__global__ void __launch_bounds__(NT)
fir_decim_consec_kernel(const typename K::T *__restrict__ win, const typename K::T *__restrict__ x,
                        const typename K::C *__restrict__ taps, int L, int M, typename K::C scale,
                        typename K::T *__restrict__ y, size_t ny, int pitch, typename K::T *__restrict__ win_next) {
    fir_decim_consec_body<K, NT, R>(win, x, taps, L, M, scale, y, ny, pitch, win_next, FirNoMix{});
}

template <class K, int NT, int R>
static int launch_fir_decim_consec(const typename K::T *win, const typename K::T *x, const typename K::C *taps, int L,
                                   int M, typename K::C scale, typename K::T *y, size_t ny, hipStream_t st,
                                   typename K::T *win_next) {
    using T = typename K::T;
    constexpr int TILE = NT * R;
    const int pitch = decim_consec_pitch(TILE, L, M, R);
    const size_t lds = (size_t)M * pitch * sizeof(T);
    const size_t nblk = (ny + TILE - 1) / TILE;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    fir_decim_consec_kernel<K, NT, R><<<(unsigned)nblk, NT, lds, st>>>(win, x, taps, L, M, scale, y, ny, pitch, win_next);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

template <class K>
int launch_fir_block(const typename K::T *win, const typename K::T *x, const typename K::C *taps,
                     int L, int M, typename K::C scale, typename K::T *y, size_t ny, hipStream_t st,
                     size_t x_len, typename K::T *win_next) {
    using T = typename K::T;
    if (ny == 0) return YAGI_OK;
    if (L <= 0 || M <= 0) return fail(YAGI_ERR_INTERNAL, "fir_block: bad L/M");
    const FirBlockPlan p = fir_block_plan(sizeof(T), L, M, ny, x_len);      // fir_bodies.hpp: thresholds and budgets
    if (p.kind == kFirPlanConsec) return launch_fir_consec<K>(win, x, taps, L, scale, y, ny, st, win_next);
    if (p.kind == kFirPlanDecim) {
        if (p.nt == 256 && p.r == 8) return launch_fir_decim_consec<K, 256, 8>(win, x, taps, L, M, scale, y, ny, st, win_next);
        if (p.nt == 256 && p.r == 4) return launch_fir_decim_consec<K, 256, 4>(win, x, taps, L, M, scale, y, ny, st, win_next);
        if (p.nt == 128 && p.r == 4) return launch_fir_decim_consec<K, 128, 4>(win, x, taps, L, M, scale, y, ny, st, win_next);
        if (p.nt == 64 && p.r == 8) return launch_fir_decim_consec<K, 64, 8>(win, x, taps, L, M, scale, y, ny, st, win_next);
        return launch_fir_decim_consec<K, 64, 4>(win, x, taps, L, M, scale, y, ny, st, win_next);
    }
    const size_t nblk = (ny + p.tile - 1) / p.tile;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    // x_len = samples readable at x (0 = unknown: the outputs' own span, ny*M)
    const long long xl = (long long)(x_len ? x_len : ny * (size_t)M);
    if (p.kind == kFirPlanStaged)
        fir_block_kernel<K, true><<<(unsigned)nblk, kFirBlock, p.lds, st>>>(win, x, taps, L, M, scale, y, ny, p.tile, xl, win_next);
    else
        fir_block_kernel<K, false><<<(unsigned)nblk, kFirBlock, 0, st>>>(win, x, taps, L, M, scale, y, ny, p.tile, xl, win_next);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

template int launch_fir_block<RRRF>(const float *, const float *, const float *, int, int, float, float *, size_t, hipStream_t, size_t, float *);
template int launch_fir_block<CRCF>(const cf32 *, const cf32 *, const float *, int, int, float, cf32 *, size_t, hipStream_t, size_t, cf32 *);
template int launch_fir_block<CCCF>(const cf32 *, const cf32 *, const cf32 *, int, int, cf32, cf32 *, size_t, hipStream_t, size_t, cf32 *);

// polyphase bank, all branches per pushed sample (interpolator form); the bodies are in fir_bodies.hpp
template <class K, bool TAPS_LDS>
__global__ void __launch_bounds__(256)
firpfb_all_kernel(const typename K::T *__restrict__ win, const typename K::T *__restrict__ x,
                  const typename K::C *__restrict__ hb, int nf, int Ls, typename K::C scale,
                  typename K::T *__restrict__ y, size_t n, typename K::T *__restrict__ win_next) {
    firpfb_all_body<K, TAPS_LDS>(win, x, hb, nf, Ls, scale, y, n, win_next, FirNoMix{});
}

template <class K>
__global__ void __launch_bounds__(256)
firpfb_fewbranch_kernel(const typename K::T *__restrict__ win, const typename K::T *__restrict__ x,
                        const typename K::C *__restrict__ hb, int nf, int Ls, typename K::C scale,
                        typename K::T *__restrict__ y, size_t n, typename K::T *__restrict__ win_next) {
    firpfb_fewbranch_body<K>(win, x, hb, nf, Ls, scale, y, n, win_next, FirNoMix{});
}

template <class K>
int launch_firpfb_all(const typename K::T *win, const typename K::T *x, const typename K::C *hb,
                      int nf, int Ls, typename K::C scale, typename K::T *y, size_t n, hipStream_t st,
                      typename K::T *win_next) {
    using T = typename K::T;
    using C = typename K::C;
    if (n == 0) return YAGI_OK;
    const FirPfbPlan p = firpfb_all_plan(sizeof(T), sizeof(C), nf, Ls);     // fir_bodies.hpp
    if (p.kind == kPfbPlanNone) return fail(YAGI_ERR_CONFIG, "branch filters too long (%d taps)", Ls);
    const size_t nblk = p.kind == kPfbPlanFew ? (n + 255) / 256 : (n + kPfbTN - 1) / kPfbTN;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    if (p.kind == kPfbPlanFew)
        firpfb_fewbranch_kernel<K><<<(unsigned)nblk, 256, p.lds, st>>>(win, x, hb, nf, Ls, scale, y, n, win_next);
    else if (p.kind == kPfbPlanTapsLds)
        firpfb_all_kernel<K, true><<<(unsigned)nblk, 256, p.lds, st>>>(win, x, hb, nf, Ls, scale, y, n, win_next);
    else
        firpfb_all_kernel<K, false><<<(unsigned)nblk, 256, p.lds, st>>>(win, x, hb, nf, Ls, scale, y, n, win_next);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}
template int launch_firpfb_all<RRRF>(const float *, const float *, const float *, int, int, float, float *, size_t, hipStream_t, float *);
template int launch_firpfb_all<CRCF>(const cf32 *, const cf32 *, const float *, int, int, float, cf32 *, size_t, hipStream_t, cf32 *);
template int launch_firpfb_all<CCCF>(const cf32 *, const cf32 *, const cf32 *, int, int, cf32, cf32 *, size_t, hipStream_t, cf32 *);

// ---------------------------------------------------------------------------------------------
// branch index per sample (the arbitrary resampler's access pattern, resamp.rs:141-154 with the
// phase schedule precomputed): y[n] = scale * sum_k hb[idx[n]][k] * X[n-k].
// One lane per output; samples from an LDS tile, taps gathered from L2.
// ---------------------------------------------------------------------------------------------
constexpr int kSelTile = 1024;

template <class K>
__global__ void __launch_bounds__(256)
firpfb_select_kernel(const typename K::T *__restrict__ win, const typename K::T *__restrict__ x,
                     const typename K::C *__restrict__ hb, const uint32_t *__restrict__ idx,
                     int nf, int Ls, typename K::C scale, typename K::T *__restrict__ y, size_t n) {
    using T = typename K::T;
    using C = typename K::C;
    extern __shared__ __align__(16) unsigned char smem[];
    T *xs = reinterpret_cast<T *>(smem);
    const size_t n0 = (size_t)blockIdx.x * kSelTile;
    const int nt = (int)((n - n0) < (size_t)kSelTile ? (n - n0) : (size_t)kSelTile);
    const long long base = (long long)n0 - (Ls - 1);
    batched_for<256>(nt + Ls - 1, [&](int i) { return load_stream(win, x, base + i, Ls); }, [&](int i, T v) { xs[i] = v; });
    __syncthreads();
    for (int nl = threadIdx.x; nl < nt; nl += 256) {
        uint32_t b = idx[n0 + nl];
        if (b >= (uint32_t)nf) b = (uint32_t)nf - 1;     // host validates; clamp keeps the read in range
        const C *hrow = hb + (size_t)b * Ls;
        T acc = zero_of<T>();
        for (int k = 0; k < Ls; ++k) acc = mac(acc, xs[nl + (Ls - 1) - k], hrow[k]);
        y[n0 + nl] = mul(acc, scale);
    }
}

template <class K>
int launch_firpfb_select(const typename K::T *win, const typename K::T *x, const typename K::C *hb,
                         const uint32_t *idx, int nf, int Ls, typename K::C scale,
                         typename K::T *y, size_t n, hipStream_t st) {
    using T = typename K::T;
    if (n == 0) return YAGI_OK;
    const size_t xs_bytes = (size_t)(kSelTile + Ls - 1) * sizeof(T);
    if (xs_bytes > kFirLdsBudget) return fail(YAGI_ERR_CONFIG, "branch filters too long (%d taps)", Ls);
    const size_t nblk = (n + kSelTile - 1) / kSelTile;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    firpfb_select_kernel<K><<<(unsigned)nblk, 256, xs_bytes, st>>>(win, x, hb, idx, nf, Ls, scale, y, n);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}
template int launch_firpfb_select<RRRF>(const float *, const float *, const float *, const uint32_t *, int, int, float, float *, size_t, hipStream_t);
template int launch_firpfb_select<CRCF>(const cf32 *, const cf32 *, const float *, const uint32_t *, int, int, float, cf32 *, size_t, hipStream_t);
template int launch_firpfb_select<CCCF>(const cf32 *, const cf32 *, const cf32 *, const uint32_t *, int, int, cf32, cf32 *, size_t, hipStream_t);

// ---------------------------------------------------------------------------------------------
// Rresamp<T,Coeff>::execute_primitive over many blocks (rresamp.rs:162-183): every Q inputs give P
// outputs; output n of a block is branch (n Q) mod P of the bank, evaluated after input floor(n Q / P)
// of that block has been pushed -- a static schedule, so every output is an independent Ls-tap dot
// product:   y[blk P + n] = scale * sum_k hb[(nQ) mod P][k] X[blk Q + floor(nQ/P) - k].
// One lane per output; the tile's input span sits in LDS, the bank is gathered through L1/L2.
// ---------------------------------------------------------------------------------------------
template <class K>
__global__ void __launch_bounds__(256)
rresamp_kernel(const typename K::T *__restrict__ win, const typename K::T *__restrict__ x,
               const typename K::C *__restrict__ hb, int P, int Q, int Ls, typename K::C scale,
               typename K::T *__restrict__ y, size_t nblocks, int tile_blocks, typename K::T *__restrict__ win_next) {
    using T = typename K::T;
    using C = typename K::C;
    extern __shared__ __align__(16) unsigned char smem[];
    T *xs = reinterpret_cast<T *>(smem);
    write_next_window(win, x, nblocks * (size_t)Q, Ls, win_next);
    const size_t b0 = (size_t)blockIdx.x * tile_blocks;
    const int nb = (int)((nblocks - b0) < (size_t)tile_blocks ? (nblocks - b0) : (size_t)tile_blocks);
    const long long base = (long long)b0 * Q - (Ls - 1);
    const int span = nb * Q + Ls - 1;
    batched_for<256>(span, [&](int i) { return load_stream(win, x, base + i, Ls); }, [&](int i, T v) { xs[i] = v; });
    __syncthreads();
    const int nout = nb * P;
    for (int o = threadIdx.x; o < nout; o += 256) {
        const int bl = o / P, n = o - bl * P;
        const int nq = n * Q, i = nq / P, br = nq - i * P;
        const C *hrow = hb + (size_t)br * Ls;
        const T *xp = xs + (Ls - 1) + bl * Q + i;
        // one FMA chain in tap order (bit-identical to the per-sample loop), the reads of four taps issued together
        T acc = zero_of<T>();
        int k = 0;
        for (; k + 4 <= Ls; k += 4) {
            const T x0 = xp[-k], x1 = xp[-k - 1], x2 = xp[-k - 2], x3 = xp[-k - 3];
            const C h0 = hrow[k], h1 = hrow[k + 1], h2 = hrow[k + 2], h3 = hrow[k + 3];
            acc = mac(acc, x0, h0);
            acc = mac(acc, x1, h1);
            acc = mac(acc, x2, h2);
            acc = mac(acc, x3, h3);
        }
        for (; k < Ls; ++k) acc = mac(acc, xp[-k], hrow[k]);
        y[b0 * P + o] = mul(acc, scale);
    }
}

template <class K>
int launch_rresamp(const typename K::T *win, const typename K::T *x, const typename K::C *hb, int P, int Q,
                   int Ls, typename K::C scale, typename K::T *y, size_t nblocks, hipStream_t st,
                   typename K::T *win_next) {
    using T = typename K::T;
    if (nblocks == 0) return YAGI_OK;
    const RresampPlan p = rresamp_plan(sizeof(T), P, Q, Ls);                // fir_bodies.hpp: blocks per tile
    if (p.tb == 0) return fail(YAGI_ERR_CONFIG, "rresamp: Q and the branch length do not fit the LDS (%d, %d)", Q, Ls);
    const size_t nblk = (nblocks + p.tb - 1) / p.tb;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    rresamp_kernel<K><<<(unsigned)nblk, 256, p.lds, st>>>(win, x, hb, P, Q, Ls, scale, y, nblocks, p.tb, win_next);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}
template int launch_rresamp<RRRF>(const float *, const float *, const float *, int, int, int, float, float *, size_t, hipStream_t, float *);
template int launch_rresamp<CRCF>(const cf32 *, const cf32 *, const float *, int, int, int, float, cf32 *, size_t, hipStream_t, cf32 *);
template int launch_rresamp<CCCF>(const cf32 *, const cf32 *, const cf32 *, int, int, int, cf32, cf32 *, size_t, hipStream_t, cf32 *);

// ---------------------------------------------------------------------------------------------
// Resamp<T,Coeff>::execute_block (resamp.rs:141-165).  The control loop only adds integers (phase += step per output,
// phase -= 2^24 per input), so with A_j = p0 + j*step (64-bit) output j of the call comes after input i_j = A_j >> 24
// has been pushed and uses branch (A_j & 0xFFFFFF) >> (24 - bits):
//     y[j] = sum_k hb[b_j][k] X[i_j - k]        (scale 1, firpfb.rs:277-286)
// One workgroup per `tile` consecutive outputs; the host picks the tile so that the input span
// [i_{j0} - (Ls-1), i_{j0+tile-1}] fits the LDS.  One lane per output; the bank is gathered through L1/L2.
// ---------------------------------------------------------------------------------------------
template <class K>
__global__ void __launch_bounds__(256)
resamp_kernel(const typename K::T *__restrict__ win, const typename K::T *__restrict__ x,
              const typename K::C *__restrict__ hb, int Ls, int bits, uint32_t step, uint32_t p0,
              typename K::T *__restrict__ y, size_t ny, size_t nx, int tile, typename K::T *__restrict__ win_next) {
    using T = typename K::T;
    using C = typename K::C;
    extern __shared__ __align__(16) unsigned char smem[];
    T *xs = reinterpret_cast<T *>(smem);
    write_next_window(win, x, nx, Ls, win_next);
    const uint64_t j0 = (uint64_t)blockIdx.x * (uint64_t)tile;
    const int nt = (int)((ny - j0) < (uint64_t)tile ? (ny - j0) : (uint64_t)tile);
    const uint64_t a0 = (uint64_t)p0 + j0 * step;
    const uint64_t i_first = a0 >> 24, i_last = (a0 + (uint64_t)(nt - 1) * step) >> 24;
    const long long base = (long long)i_first - (Ls - 1);
    const int span = (int)(i_last - i_first) + Ls;
    batched_for<256>(span, [&](int i) { return load_stream(win, x, base + i, Ls); }, [&](int i, T v) { xs[i] = v; });
    __syncthreads();
    const int shift = 24 - bits;
    for (int o = threadIdx.x; o < nt; o += 256) {
        const uint64_t a = a0 + (uint64_t)o * step;
        const int li = (int)((a >> 24) - i_first);
        const uint32_t br = ((uint32_t)a & 0xFFFFFFu) >> shift;
        const C *hrow = hb + (size_t)br * Ls;
        const T *xp = xs + (Ls - 1) + li;
        y[j0 + o] = resamp_branch_dot<T, C>(xp, hrow, Ls);     // fir_bodies.hpp
    }
}

template <class K>
int launch_resamp(const typename K::T *win, const typename K::T *x, const typename K::C *hb, int Ls, int bits,
                  uint32_t step, uint32_t p0, typename K::T *y, size_t ny, size_t nx, hipStream_t st,
                  typename K::T *win_next) {
    using T = typename K::T;
    if (ny == 0) return YAGI_OK;
    if (bits < 1 || bits > 16 || step == 0) return fail(YAGI_ERR_CONFIG, "resamp: bad schedule (bits %d, step %u)", bits, step);
    const ResampPlan p = resamp_plan(sizeof(T), Ls, step);                  // fir_bodies.hpp: outputs per tile
    if (p.tile == 0) return fail(YAGI_ERR_CONFIG, "resamp: branch length %d does not fit the LDS", Ls);
    const size_t nblk = (ny + p.tile - 1) / p.tile;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    resamp_kernel<K><<<(unsigned)nblk, 256, p.lds, st>>>(win, x, hb, Ls, bits, step, p0, y, ny, nx, p.tile, win_next);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}
template int launch_resamp<RRRF>(const float *, const float *, const float *, int, int, uint32_t, uint32_t, float *, size_t, size_t, hipStream_t, float *);
template int launch_resamp<CRCF>(const cf32 *, const cf32 *, const float *, int, int, uint32_t, uint32_t, cf32 *, size_t, size_t, hipStream_t, cf32 *);
template int launch_resamp<CCCF>(const cf32 *, const cf32 *, const cf32 *, int, int, uint32_t, uint32_t, cf32 *, size_t, size_t, hipStream_t, cf32 *);

// ---------------------------------------------------------------------------------------------
// Plan queries (include/yagi_hip.h, diagnostics): what the launchers above would run for a shape, from the planners
// they call themselves.  Host arithmetic only, no device needed.  A shape that does not fit leaves tile = 0.
// ---------------------------------------------------------------------------------------------
namespace {

static_assert(kFirPlanConsec == YAGI_PLAN_FIR_CONSEC && kFirPlanDecim == YAGI_PLAN_FIR_DECIM &&
                  kFirPlanStaged == YAGI_PLAN_FIR_STAGED && kFirPlanUnstaged == YAGI_PLAN_FIR_UNSTAGED &&
                  kPfbPlanFew == YAGI_PLAN_PFB_FEW && kPfbPlanTapsLds == YAGI_PLAN_PFB_TAPS_LDS &&
                  kPfbPlanTapsGlobal == YAGI_PLAN_PFB_TAPS_GLOBAL && kPfbPlanNone == YAGI_PLAN_PFB_NONE &&
                  kDecimStageElement == YAGI_PLAN_STAGE_ELEMENT && kDecimStageDescriptor == YAGI_PLAN_STAGE_DESCRIPTOR &&
                  kDecimStagePow2 == YAGI_PLAN_STAGE_POW2,
              "the header's plan codes are the planners' enums");

bool plan_elem_ok(size_t elem) { return elem == sizeof(float) || elem == sizeof(cf32); }

yagi_hip_plan fir_block_plan_of(size_t elem, int L, int M, size_t ny) {
    const FirBlockPlan p = fir_block_plan(elem, L, M, ny, 0);
    yagi_hip_plan o{};
    o.kind = p.kind;
    o.nt = p.nt;
    o.r = p.r;
    o.tile = p.kind == kFirPlanConsec ? kConsecTile : p.kind == kFirPlanDecim ? p.nt * p.r : p.tile;
    o.lds = p.lds;
    if (p.kind == kFirPlanConsec) o.lds = fir_consec_lds(elem, L);
    if (p.kind == kFirPlanDecim) o.staging = decim_interior_staging(elem, L, M, p.nt, p.r);
    return o;
}
yagi_hip_plan firpfb_all_plan_of(size_t elem, size_t celem, int nf, int Ls) {
    const FirPfbPlan p = firpfb_all_plan(elem, celem, nf, Ls);
    yagi_hip_plan o{};
    o.kind = p.kind;
    o.tile = p.kind == kPfbPlanNone ? 0 : p.kind == kPfbPlanFew ? 256 : kPfbTN;
    o.lds = p.lds;
    return o;
}
yagi_hip_plan rresamp_plan_of(size_t elem, int P, int Q, int Ls) {
    const RresampPlan p = rresamp_plan(elem, P, Q, Ls);
    yagi_hip_plan o{};
    o.tile = p.tb;
    o.lds = p.lds;
    return o;
}
yagi_hip_plan resamp_plan_of(size_t elem, int Ls, uint32_t step) {
    const ResampPlan p = resamp_plan(elem, Ls, step);
    yagi_hip_plan o{};
    o.tile = p.tile;
    o.lds = p.lds;
    return o;
}

}  // namespace
}  // namespace yagi

using namespace yagi;

#define PLAN_CHECK(cond, what)                                                                   \
    do {                                                                                         \
        if (!out) return fail(YAGI_ERR_CONFIG, "null pointer argument");                         \
        if (!(cond)) return fail(YAGI_ERR_CONFIG, "plan query: bad " what);                      \
    } while (0)

extern "C" {

int yagi_hip_plan_fir_block(size_t elem, size_t L, size_t M, size_t ny, yagi_hip_plan *out) try {
    return yagi_hip_plan_fir_block_range(elem, L, 1, M, ny, out);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_plan_fir_block_range(size_t elem, size_t L0, size_t count, size_t M, size_t ny, yagi_hip_plan *out) try {
    PLAN_CHECK(plan_elem_ok(elem) && L0 >= 1 && count <= (size_t)1 << 24 && L0 + count <= ((size_t)1 << 24) + 1 && M >= 1 && M <= (size_t)1 << 20 && ny >= 1,
               "shape (elem 4 or 8, 1 <= L <= 2^24, 1 <= M <= 2^20, ny >= 1)");
    for (size_t i = 0; i < count; ++i) out[i] = fir_block_plan_of(elem, (int)(L0 + i), (int)M, ny);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_plan_firpfb_all(size_t elem, size_t coeff_elem, size_t nf, size_t Ls, yagi_hip_plan *out) try {
    return yagi_hip_plan_firpfb_all_range(elem, coeff_elem, nf, Ls, 1, out);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_plan_firpfb_all_range(size_t elem, size_t coeff_elem, size_t nf, size_t Ls0, size_t count,
                                   yagi_hip_plan *out) try {
    PLAN_CHECK(plan_elem_ok(elem) && plan_elem_ok(coeff_elem) && coeff_elem <= elem && nf >= 1 && nf <= (size_t)1 << 20 &&
                   Ls0 >= 1 && count <= (size_t)1 << 24 && Ls0 + count <= ((size_t)1 << 20) + 1,
               "shape (elem, coeff_elem 4 or 8, 1 <= nf, Ls <= 2^20)");
    for (size_t i = 0; i < count; ++i) out[i] = firpfb_all_plan_of(elem, coeff_elem, (int)nf, (int)(Ls0 + i));
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_plan_rresamp(size_t elem, size_t P, size_t Q, size_t Ls, yagi_hip_plan *out) try {
    YG_TRY(yagi_hip_plan_rresamp_range(elem, P, Q, Ls, 1, out));
    if (out->tile == 0) return fail(YAGI_ERR_CONFIG, "rresamp: Q and the branch length do not fit the LDS (%zu, %zu)", Q, Ls);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_plan_rresamp_range(size_t elem, size_t P, size_t Q, size_t Ls0, size_t count, yagi_hip_plan *out) try {
    PLAN_CHECK(plan_elem_ok(elem) && P >= 1 && P <= (size_t)1 << 15 && Q >= 1 && Q <= (size_t)1 << 15 && Ls0 >= 1 &&
                   count <= (size_t)1 << 24 && Ls0 + count <= ((size_t)1 << 20) + 1,
               "shape (elem 4 or 8, 1 <= P, Q <= 2^15, 1 <= Ls <= 2^20)");
    for (size_t i = 0; i < count; ++i) out[i] = rresamp_plan_of(elem, (int)P, (int)Q, (int)(Ls0 + i));
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_plan_resamp(size_t elem, size_t Ls, uint32_t step, yagi_hip_plan *out) try {
    YG_TRY(yagi_hip_plan_resamp_range(elem, Ls, 1, step, out));
    if (out->tile == 0) return fail(YAGI_ERR_CONFIG, "resamp: branch length %zu does not fit the LDS", Ls);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_plan_resamp_range(size_t elem, size_t Ls0, size_t count, uint32_t step, yagi_hip_plan *out) try {
    PLAN_CHECK(plan_elem_ok(elem) && Ls0 >= 1 && count <= (size_t)1 << 24 && Ls0 + count <= ((size_t)1 << 21) + 1 && step > 0,
               "shape (elem 4 or 8, 1 <= Ls <= 2^21, step > 0)");
    for (size_t i = 0; i < count; ++i) out[i] = resamp_plan_of(elem, (int)(Ls0 + i), step);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"
