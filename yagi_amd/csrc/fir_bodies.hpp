// fir_bodies.hpp -- the bodies of the decimating FIR kernels and of the polyphase-bank kernels, and the choice
// launch_fir_block makes among them, shared by fir_kernels.hip (the plain kernels) and ddc_kernels.hip (Ddc / Duc: the
// same bodies with an oscillator mix on the way into LDS or at the store).  A body takes a functor:
//   decimators   mix(v, idx): the value staged for x[idx] (idx >= 0; samples of the carried window are copied as they
//                are), also applied to the tail of x that write_next_window leaves as the next window
//   bank kernels mix(v, idx): the value stored to y[idx]
// FirNoMix returns v, and the plain kernels compile to what they were before the bodies moved here.
// At the end: the per-output sums of resamp_kernel and of the bank kernels' single-branch loop, and the LFSR symbol
// source of symstream_kernel, each shared with symstreamr_kernels.hip (SymStreamR), which runs them back to back.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "devmath.hpp"
#include "kernels.hpp"

namespace yagi {

constexpr int kFirBlock = 256;
constexpr int kFirR = 4;                         // outputs per lane
constexpr size_t kFirLdsBudget = 48 * 1024;

struct FirNoMix {
    template <class T> __device__ __forceinline__ T operator()(T v, long long) const { return v; }
};

template <class T>
__device__ __forceinline__ T load_stream(const T *__restrict__ win, const T *__restrict__ x,
                                         long long idx, int L) {
    return (idx < 0) ? win[L + idx] : x[idx];
}
template <class T, class Mix>
__device__ __forceinline__ T load_stream_mix(const T *__restrict__ win, const T *__restrict__ x,
                                             long long idx, int L, const Mix &mix) {
    return (idx < 0) ? win[L + idx] : mix(x[idx], idx);
}

// The state a Window<T> holds after the block (window.rs:77-85): new_win = last L samples of (win ++ x[0..n)).
// Written by the LAST workgroup of the block's own kernel (reads only; `win_next` is the object's other window
// buffer), which saves the separate 4-5 us window-update launch after every execute_block.
template <class T, class Mix = FirNoMix>
__device__ __forceinline__ void write_next_window(const T *__restrict__ win, const T *__restrict__ x, size_t n, int L,
                                                  T *__restrict__ win_next, const Mix &mix = Mix{}) {
    if (win_next == nullptr || blockIdx.x != gridDim.x - 1) return;
    for (int j = threadIdx.x; j < L; j += blockDim.x) {
        const size_t c = n + (size_t)j;            // index into win ++ x
        win_next[j] = (c < (size_t)L) ? win[c] : mix(x[c - (size_t)L], (long long)(c - (size_t)L));
    }
}

// STAGE = span in LDS.  The span is stored de-interleaved by decimation phase, xs[phase][j] = X[base + j*M + phase]
// (pitch P = ceil(span/M) + pad), so at tap k the 64 lanes of a wave -- 64 consecutive outputs, M samples
// apart in the stream -- read 64 CONSECUTIVE LDS words of one phase row (with the plain layout a decimator
// reads with a lane stride of M samples: 2M-way bank conflicts on ds_read_b64).  Taps come through the scalar
// cache (k is wave-uniform): one LDS read and one FMA group per MAC.
template <class K, bool STAGE, class Mix>
__device__ __forceinline__ void fir_block_body(const typename K::T *win, const typename K::T *x,
                                               const typename K::C *taps, int L, int M, typename K::C scale,
                                               typename K::T *y, size_t ny, int tile, long long x_len,
                                               typename K::T *win_next, const Mix &mix) {
    using T = typename K::T;
    using C = typename K::C;
    static_assert(STAGE || std::is_same<Mix, FirNoMix>::value, "a mix is applied on the way into LDS");
    extern __shared__ __align__(16) unsigned char smem[];
    write_next_window(win, x, ny * (size_t)M, L, win_next, mix);
    const size_t o0 = (size_t)blockIdx.x * (size_t)tile;
    const int nt = (int)((ny - o0) < (size_t)tile ? (ny - o0) : (size_t)tile);
    const long long base = (long long)o0 * M - (L - 1);
    const int span = (nt - 1) * M + L;
    const int pitch = (((tile - 1) * M + L + M - 1) / M) | 1;          // odd: phase rows start on different banks

    T *xs = reinterpret_cast<T *>(smem);
    if (STAGE) {
        // loads issued in batches before the LDS writes (devmath.hpp: batched_for)
        if (base >= 0 && base + span <= x_len) {       // block-uniform: the whole span lies inside x
            const T *src = x + base;
            if (M == 1) {
                batched_for<kFirBlock>(span, [&](int i) { return src[i]; }, [&](int i, T v) { xs[i] = mix(v, base + i); });
            } else {
                batched_for<kFirBlock>(span, [&](int i) { return src[i]; }, [&](int i, T v) {
                    const int j = i / M, ph = i - j * M;
                    xs[ph * pitch + j] = mix(v, base + i);
                });
            }
        } else {
            batched_for<kFirBlock>(span, [&](int i) { return load_stream_mix(win, x, base + i, L, mix); }, [&](int i, T v) {
                const int j = i / M, ph = i - j * M;
                xs[ph * pitch + j] = v;
            });
        }
        __syncthreads();
    }

    T acc[kFirR];
#pragma unroll
    for (int r = 0; r < kFirR; ++r) acc[r] = zero_of<T>();

    // newest sample of output o sits at span offset o*M + (L-1); tap k reads offset o*M + (L-1-k):
    // phase (L-1-k) mod M, row index o + (L-1-k) div M.  Taps are fetched 8 at a time (one scalar load),
    // a full tile (all 4 x 256 outputs exist) runs without per-output guards.
    auto run = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        int ph = (L - 1) % M, jq = (L - 1) / M;
        auto tap = [&](C hk, int k) {
            if (STAGE) {
                const T *row = xs + ph * pitch + jq + threadIdx.x;
#pragma unroll
                for (int r = 0; r < kFirR; ++r)
                    if (FULL || (int)threadIdx.x + r * kFirBlock < nt) acc[r] = mac(acc[r], row[r * kFirBlock], hk);
                if (--ph < 0) { ph = M - 1; --jq; }
            } else {
#pragma unroll
                for (int r = 0; r < kFirR; ++r) {
                    const int o = threadIdx.x + r * kFirBlock;
                    if (FULL || o < nt)
                        acc[r] = mac(acc[r], load_stream(win, x, base + (long long)o * M + (L - 1) - k, L), hk);
                }
            }
        };
        int k = 0;
        for (; k + 8 <= L; k += 8) {
            C hk[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) hk[u] = taps[k + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) tap(hk[u], k + u);
        }
        for (; k < L; ++k) tap(taps[k], k);
    };
    if (nt == kFirR * kFirBlock) run(std::true_type{});
    else run(std::false_type{});
#pragma unroll
    for (int r = 0; r < kFirR; ++r) {
        const int o = threadIdx.x + r * kFirBlock;
        if (o < nt) y[o0 + o] = mul(acc[r], scale);
    }
}

// ---------------------------------------------------------------------------------------------
// Decimator (M >= 2) with the same register window, one decimation phase at a time: the taps of phase p are
// h[L-1-p-M*i], i = 0.., and at step i output o reads row p of the phase-split span at index o + i -- so a lane
// that owns 8 consecutive outputs slides an 8-sample window along the row, one LDS read per 8 MACs.  Rows carry
// the 9/8 padding of fir_consec_kernel.  The sum runs phase by phase instead of in tap order (same products,
// f32 rounding may differ from fir_block_kernel in the last bit; exact on integer data).  NT lanes per
// workgroup (tile = 8*NT outputs) so that the M rows fit the LDS budget.
// ---------------------------------------------------------------------------------------------
template <class K, int NT, int R, class Mix>
__device__ __forceinline__ void fir_decim_consec_body(const typename K::T *win,
                                                      const typename K::T *x,
                                                      const typename K::C *taps, int L, int M,
                                                      typename K::C scale, typename K::T *y, size_t ny,
                                                      int pitch, typename K::T *win_next, const Mix &mix) {
    using T = typename K::T;
    using C = typename K::C;
    constexpr int TILE = NT * R, LG = R == 8 ? 3 : 2;
    static_assert(R == 8 || R == 4, "window of 4 or 8 samples");
    extern __shared__ __align__(16) unsigned char smem[];
    T *xs = reinterpret_cast<T *>(smem);
    write_next_window(win, x, ny * (size_t)M, L, win_next, mix);
    const size_t o0 = (size_t)blockIdx.x * TILE;
    const int nt = (int)((ny - o0) < (size_t)TILE ? (ny - o0) : (size_t)TILE);
    const long long base = (long long)o0 * M - (L - 1);         // stream index of row 0, entry 0
    const long long xlen = (long long)ny * M;
    const int ni = (L + M - 1) / M;                              // steps of the longest row
    const int total = (TILE + ni - 1) * M;                       // entries any (o, i) of a full tile can reach
    // entry e = jj*M + ph; (jj, ph) advance by NT entries per trip without a division
    const int djj = NT / M, dph = NT - djj * M;
    int jj = (int)threadIdx.x / M, ph = (int)threadIdx.x - jj * M;
    // eight loads per lane in flight before the LDS writes; (jj, ph) advance with the stores, in order
    const bool inside = base >= 0 && base + total <= xlen;       // block-uniform: every entry lies inside x
    // Interior tile, M a power of two with NT / M a multiple of R: the lane's decimation phase is fixed
    // (ph = tid mod M) and its row index advances by NT / M per trip, so the LDS slot advances by a constant and the
    // samples come through a buffer descriptor of exactly `total` entries (entries past it are range-checked away, never read):
    // no address arithmetic per entry -- the generic staging below spent as many vector instructions as the taps.
    // (decim_interior_staging below repeats `desc` and `fast` for the plan queries: change the two together)
    const int lgM = 31 - __builtin_clz((unsigned)M);
    const bool desc = inside && (unsigned long long)total * sizeof(T) < 0xffffffffull;
    const bool fast = desc && (M & (M - 1)) == 0 && M <= NT && ((NT >> lgM) & (R - 1)) == 0;
    if (desc && !fast) {
        // any other M: the same descriptor loads, the (row, phase) of an entry advanced incrementally per trip
        const __amdgpu_buffer_rsrc_t rx = make_rsrc(x + base, (unsigned)((size_t)total * sizeof(T)));
        const unsigned vo = (unsigned)sizeof(T) * threadIdx.x;
        for (int t0 = 0; t0 * NT < total; t0 += 8) {
            T r[8];
#pragma unroll
            for (int it = 0; it < 8; ++it)
                r[it] = buf_ld_t<T>(rx, vo + (unsigned)sizeof(T) * NT * (unsigned)(t0 + it), 0u);
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int e = (int)threadIdx.x + NT * (t0 + it);
                if (e < total) xs[ph * pitch + jj + (jj >> LG)] = mix(r[it], base + e);
                jj += djj; ph += dph;
                if (ph >= M) { ph -= M; ++jj; }
            }
        }
    } else if (fast) {
        const __amdgpu_buffer_rsrc_t rx = make_rsrc(x + base, (unsigned)((size_t)total * sizeof(T)));
        const unsigned vo = (unsigned)sizeof(T) * threadIdx.x;
        const int rows = NT >> lgM;                              // row entries per trip
        const int sstride = rows + (rows >> LG);
        const int jj0 = (int)threadIdx.x >> lgM;
        T *dst = xs + ((int)threadIdx.x & (M - 1)) * pitch + jj0 + (jj0 >> LG);
        for (int t0 = 0; t0 * NT < total; t0 += 8) {
            T r[8];
#pragma unroll
            for (int it = 0; it < 8; ++it)       // the trip goes into the VGPR offset: that is the part the range check covers
                r[it] = buf_ld_t<T>(rx, vo + (unsigned)sizeof(T) * NT * (unsigned)(t0 + it), 0u);
            if ((t0 + 8) * NT <= total) {
#pragma unroll
                for (int it = 0; it < 8; ++it)
                    dst[sstride * (t0 + it)] = mix(r[it], base + ((int)threadIdx.x + NT * (t0 + it)));
            } else {
#pragma unroll
                for (int it = 0; it < 8; ++it)
                    if ((int)threadIdx.x + NT * (t0 + it) < total)
                        dst[sstride * (t0 + it)] = mix(r[it], base + ((int)threadIdx.x + NT * (t0 + it)));
            }
        }
    } else
    for (int e0 = threadIdx.x; e0 < total; e0 += 8 * NT) {
        T r[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int e = e0 + NT * it;
            const long long idx = base + (e < total ? e : total - 1);
            T v = zero_of<T>();
            if (inside) v = mix(x[idx], idx);
            else if (idx < 0) v = win[L + idx];
            else if (idx < xlen) v = mix(x[idx], idx);
            r[it] = v;
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            if (e0 + NT * it < total) xs[ph * pitch + jj + (jj >> LG)] = r[it];
            jj += djj; ph += dph;
            if (ph >= M) { ph -= M; ++jj; }
        }
    }
    __syncthreads();
    const int l = threadIdx.x;
    T acc[R], w[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = zero_of<T>();
    const int np_phases = M < L ? M : L;
#pragma unroll 1
    for (int ph = 0; ph < np_phases; ++ph) {
        const int n_p = (L - 1 - ph) / M + 1;
        const T *row = xs + ph * pitch + (R + 1) * l;            // slot of row index R l + q: (R+1) l + q + (q >> LG)
        const C *tp = taps + (L - 1 - ph);                       // step i multiplies by tp[-M*i]
#pragma unroll
        for (int r = 0; r < R - 1; ++r) w[r] = row[r];           // w[(r + i) & (R-1)] = row entry R l + r + i
        auto eight_steps = [&](int i0, auto full_tag) {
            constexpr bool FULL = decltype(full_tag)::value;
            C hk[R];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int i = (FULL || i0 + u < n_p) ? i0 + u : n_p - 1;
                hk[u] = tp[-(long long)M * i];
            }
            const T *rb = row + i0 + (i0 >> LG);                 // i0 is a multiple of R
#pragma unroll
            for (int u = 0; u < R; ++u) {
                w[(R - 1 + u) & (R - 1)] = rb[(R - 1 + u) + ((R - 1 + u) >> LG)];   // the window's new highest sample
                if (FULL || i0 + u < n_p) {
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r] = mac(acc[r], w[(r + u) & (R - 1)], hk[u]);
                }
            }
        };
        int i0 = 0;
        for (; i0 + R <= n_p; i0 += R) eight_steps(i0, std::true_type{});
        if (i0 < n_p) eight_steps(i0, std::false_type{});
    }
    const int o = R * l;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (o + r < nt) y[o0 + o + r] = mul(acc[r], scale);
}

// row pitch of the decimator kernel: entries any step can touch (tile + steps rounded up to 8, + the 8 of the
// last window refill), padded 9/8, odd so that the M rows start on different banks
static inline int decim_consec_pitch(int tile, int L, int M, int R) {
    const int ni = (L + M - 1) / M;
    const int n = tile + ((ni + R - 1) & ~(R - 1)) + R;
    return (n + n / R + 1) | 1;
}

// ---------------------------------------------------------------------------------------------
// What launch_fir_block runs for a shape.  elem = sizeof(T), complex = the samples are complex.
// ---------------------------------------------------------------------------------------------
enum { kFirPlanConsec = 0, kFirPlanDecim = 1, kFirPlanStaged = 2, kFirPlanUnstaged = 3 };
struct FirBlockPlan {
    int kind = kFirPlanUnstaged;
    int nt = 0, r = 0;          // kFirPlanDecim: lanes per workgroup and outputs per lane
    int tile = 0;               // kFirPlanStaged / kFirPlanUnstaged: outputs per workgroup
    size_t lds = 0;             // dynamic LDS of the launch, bytes
};

inline int decim_window_min_steps() {
    static const int min_steps = [] {
        const char *e = getenv("YAGI_HIP_DECIM_WINDOW_MIN_STEPS");
        return e ? atoi(e) : 8;
    }();
    return min_steps;
}

// size of the M = 1 register-window kernel's span (fir_kernels.hip: kConsecTile outputs)
constexpr int kConsecR = 8, kConsecTile = 256 * kConsecR;
// its dynamic LDS: the tile + the taps rounded up to 8, padded 9/8
inline size_t fir_consec_lds(size_t elem, int L) {
    const int span = kConsecTile + ((L + 7) & ~7);
    return (size_t)(span + (span >> 3) + 1) * elem;
}

inline FirBlockPlan fir_block_plan(size_t elem, int L, int M, size_t ny, size_t x_len) {
    FirBlockPlan p;
    // M = 1 with a block long enough to fill tiles, span within 48 KiB: the register-window kernel
    if (M == 1 && ny >= 512 && ((size_t)(kConsecTile + L + 8) * 9 / 8 + 1) * elem <= kFirLdsBudget && x_len == 0) {
        p.kind = kFirPlanConsec;
        return p;
    }
    // decimators: the same register window per decimation phase, with the widest workgroup whose M rows fit
    // (pays once a phase has enough taps to amortise its window fill: 8-sample window from 32 taps per phase,
    // 4-sample window with full 256-lane workgroups from 8; YAGI_HIP_DECIM_WINDOW_MIN_STEPS overrides the 8)
    if (M >= 2 && L >= M && L / M >= decim_window_min_steps() && ny >= 512 && x_len == 0) {
        auto bytes = [&](int nt, int r) { return (size_t)M * decim_consec_pitch(nt * r, L, M, r) * elem; };
        auto fits = [&](int nt, int r) { return bytes(nt, r) <= kFirLdsBudget; };
        auto take = [&](int nt, int r) {
            p.kind = kFirPlanDecim;
            p.nt = nt;
            p.r = r;
            p.lds = bytes(nt, r);
            return p;
        };
        const bool long_phase = L / M >= 32;
        // short phases: measured wins for complex samples and for M <= 4 (rrrf M = 8, 16 taps per phase: the general
        // kernel's 4-byte LDS reads are cheaper than eight window fills)
        const bool short_ok = elem == 8 || M <= 4;
        if (long_phase && fits(256, 8)) return take(256, 8);
        if (long_phase || short_ok) {
            if (fits(256, 4)) return take(256, 4);
            if (fits(128, 4)) return take(128, 4);
        }
        if (long_phase && fits(64, 8)) return take(64, 8);
        if (long_phase && fits(64, 4)) return take(64, 4);
    }
    // largest tile (<= R*256 outputs) whose phase-split span fits the LDS budget
    auto need = [&](int t) {
        const size_t pitch = (size_t)((((long long)(t - 1) * M + L + M - 1) / M) | 1);
        return (size_t)M * pitch * elem;
    };
    int tile = kFirR * kFirBlock;
    while (tile >= 64 && need(tile) > kFirLdsBudget) tile /= 2;
    if (tile < 64) {           // span too large for LDS staging: stream from L2/HBM
        p.kind = kFirPlanUnstaged;
        p.tile = kFirR * kFirBlock;
    } else {
        p.kind = kFirPlanStaged;
        p.tile = tile;
        p.lds = need(tile);
    }
    return p;
}

// ---------------------------------------------------------------------------------------------
// polyphase bank, all branches per pushed sample (interpolator form):
//   y[n*nf + i] = scale * sum_{k<Ls} hb[i][k] * X[n-k]
// A workgroup owns TN consecutive input samples x all nf branches.  Samples + halo are staged
// in LDS; branch taps are staged TRANSPOSED (hsT[k][i]) so the 64 lanes of a wave, which hold
// 64 consecutive branches i, read consecutive LDS words; stores are coalesced along i.
// Traffic: sizeof(T) read + nf*sizeof(T) written per input sample (write-bound).
// ---------------------------------------------------------------------------------------------
constexpr int kPfbTN = 64;

template <class K, bool TAPS_LDS, class Mix>
__device__ __forceinline__ void firpfb_all_body(const typename K::T *win, const typename K::T *x,
                                                const typename K::C *hb, int nf, int Ls, typename K::C scale,
                                                typename K::T *y, size_t n,
                                                typename K::T *win_next, const Mix &mix) {
    using T = typename K::T;
    using C = typename K::C;
    extern __shared__ __align__(16) unsigned char smem[];
    T *xs = reinterpret_cast<T *>(smem);                       // kPfbTN + Ls - 1 samples
    write_next_window(win, x, n, Ls, win_next);
    C *hsT = reinterpret_cast<C *>(smem + ((size_t)(kPfbTN + Ls - 1) * sizeof(T) + 15) / 16 * 16);
    const size_t n0 = (size_t)blockIdx.x * kPfbTN;
    const int nt = (int)((n - n0) < (size_t)kPfbTN ? (n - n0) : (size_t)kPfbTN);
    const long long base = (long long)n0 - (Ls - 1);
    batched_for<256>(nt + Ls - 1, [&](int i) { return load_stream(win, x, base + i, Ls); }, [&](int i, T v) { xs[i] = v; });
    if (TAPS_LDS)
        for (int e = threadIdx.x; e < nf * Ls; e += 256) {
            const int i = e / Ls, k = e - i * Ls;
            hsT[k * nf + i] = hb[e];
        }
    __syncthreads();
    const int total = nt * nf;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int nl = e / nf, i = e - nl * nf;
        T acc = zero_of<T>();
        for (int k = 0; k < Ls; ++k) {
            const C hk = TAPS_LDS ? hsT[k * nf + i] : hb[i * Ls + k];
            acc = mac(acc, xs[nl + (Ls - 1) - k], hk);
        }
        const size_t o = (n0 + nl) * (size_t)nf + i;
        y[o] = mix(mul(acc, scale), (long long)o);
    }
}

// Few branches (interpolators: nf = 2 .. 16): with a lane per (sample, branch) the 64 lanes of a wave share 64/nf
// samples and nf taps -- two LDS reads per MAC and a tile of only 64 samples.  Here a lane owns ONE input sample
// and walks the branches four at a time: one LDS read (consecutive across lanes) per 4 MACs, the taps through
// the scalar cache (branch and tap index are wave-uniform), 256 samples per workgroup, and each lane stores 4
// consecutive outputs.  Same tap order as firpfb_all_kernel.
template <class K, class Mix>
__device__ __forceinline__ void firpfb_fewbranch_body(const typename K::T *win,
                                                      const typename K::T *x,
                                                      const typename K::C *hb, int nf, int Ls,
                                                      typename K::C scale, typename K::T *y, size_t n,
                                                      typename K::T *win_next, const Mix &mix) {
    using T = typename K::T;
    using C = typename K::C;
    extern __shared__ __align__(16) unsigned char smem[];
    T *xs = reinterpret_cast<T *>(smem);                       // 256 + Ls - 1 samples
    write_next_window(win, x, n, Ls, win_next);
    const size_t n0 = (size_t)blockIdx.x * 256;
    const int nt = (int)((n - n0) < (size_t)256 ? (n - n0) : (size_t)256);
    const long long base = (long long)n0 - (Ls - 1);
    batched_for<256>(nt + Ls - 1, [&](int i) { return load_stream(win, x, base + i, Ls); }, [&](int i, T v) { xs[i] = v; });
    __syncthreads();
    const int nl = threadIdx.x;
    if (nl >= nt) return;
    const T *xr = xs + nl + (Ls - 1);                          // tap k reads xr[-k]
    const size_t ob = (n0 + nl) * (size_t)nf;
    T *yo = y + ob;
    int g0 = 0;
    for (; g0 + 4 <= nf; g0 += 4) {
        const C *h0 = hb + (size_t)g0 * Ls;
        T acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = zero_of<T>();
#pragma unroll 4
        for (int k = 0; k < Ls; ++k) {
            const T sk = xr[-k];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = mac(acc[j], sk, h0[(size_t)j * Ls + k]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) yo[g0 + j] = mix(mul(acc[j], scale), (long long)(ob + g0 + j));
    }
    for (; g0 < nf; ++g0) {                                    // the last nf % 4 branches
        const C *h0 = hb + (size_t)g0 * Ls;
        T acc = zero_of<T>();
        for (int k = 0; k < Ls; ++k) acc = mac(acc, xr[-k], h0[k]);
        yo[g0] = mix(mul(acc, scale), (long long)(ob + g0));
    }
}

// which bank kernel launch_firpfb_all runs
enum { kPfbPlanFew = 0, kPfbPlanTapsLds = 1, kPfbPlanTapsGlobal = 2, kPfbPlanNone = 3 };
struct FirPfbPlan {
    int kind = kPfbPlanNone;
    size_t lds = 0;
};
inline FirPfbPlan firpfb_all_plan(size_t elem, size_t celem, int nf, int Ls) {
    FirPfbPlan p;
    if (nf <= 16 && (size_t)(256 + Ls - 1) * elem <= kFirLdsBudget) {
        p.kind = kPfbPlanFew;
        p.lds = (size_t)(256 + Ls - 1) * elem;
        return p;
    }
    const size_t xs_bytes = ((size_t)(kPfbTN + Ls - 1) * elem + 15) / 16 * 16;
    if (xs_bytes > kFirLdsBudget) return p;
    const size_t tap_bytes = (size_t)nf * Ls * celem;
    if (xs_bytes + tap_bytes <= kFirLdsBudget) {
        p.kind = kPfbPlanTapsLds;
        p.lds = xs_bytes + tap_bytes;
    } else {
        p.kind = kPfbPlanTapsGlobal;
        p.lds = xs_bytes;
    }
    return p;
}

// How fir_decim_consec_body<K, nt, r> stages a tile whose whole span lies inside x (`inside` there; a tile that touches
// the carried window or the end of the block always stages entry by entry): the body's `desc` and `fast`, repeated
// here for the plan queries because the body's instruction stream is pinned -- change the two together.
enum { kDecimStageElement = 0, kDecimStageDescriptor = 1, kDecimStagePow2 = 2 };
inline int decim_interior_staging(size_t elem, int L, int M, int nt, int r) {
    const int ni = (L + M - 1) / M;
    const long long total = (long long)(nt * r + ni - 1) * M;
    if (!((unsigned long long)total * elem < 0xffffffffull)) return kDecimStageElement;
    const int lgM = 31 - __builtin_clz((unsigned)M);
    const bool fast = (M & (M - 1)) == 0 && M <= nt && ((nt >> lgM) & (r - 1)) == 0;
    return fast ? kDecimStagePow2 : kDecimStageDescriptor;
}

// blocks per tile of rresamp_kernel: ~1024 outputs or inputs, whichever is larger, inside the LDS budget;
// tb = 0: even one block's span (Q + Ls - 1 samples) does not fit
struct RresampPlan {
    int tb = 0;
    size_t lds = 0;
};
inline RresampPlan rresamp_plan(size_t elem, int P, int Q, int Ls) {
    RresampPlan p;
    const int big = P > Q ? P : Q;
    int tb = 1024 / big;
    if (tb < 1) tb = 1;
    auto bytes = [&](int t) { return ((size_t)t * Q + Ls - 1) * elem; };
    while (tb > 1 && bytes(tb) > kFirLdsBudget) tb /= 2;
    if (bytes(tb) > kFirLdsBudget) return p;
    p.tb = tb;
    p.lds = bytes(tb);
    return p;
}

// input span of `t` consecutive outputs of resamp_kernel, an upper bound over every starting phase
inline uint64_t resamp_span(uint64_t t, uint32_t step, int Ls) {
    return (((t - 1) * (uint64_t)step) >> 24) + 1 + (uint64_t)Ls;
}
// outputs per tile of resamp_kernel: up to 1024 (four per lane), fewer where 1/rate makes the input span outgrow the
// LDS; tile = 0: one output's span (Ls + 1 samples) does not fit.  step > 0.
struct ResampPlan {
    int tile = 0;
    size_t lds = 0;
};
inline ResampPlan resamp_plan(size_t elem, int Ls, uint32_t step) {
    ResampPlan p;
    const uint64_t cap = kFirLdsBudget / elem;
    if (resamp_span(1, step, Ls) > cap) return p;
    uint64_t tile = 1024;
    const uint64_t room = cap - (uint64_t)Ls - 1;                       // >= 0 after the check above
    const uint64_t fit = (((room + 1) << 24) - 1) / step + 1;           // largest t with ((t-1) step) >> 24 <= room
    if (fit < tile) tile = fit;
    while (tile > 1 && resamp_span(tile, step, Ls) > cap) --tile;
    p.tile = (int)tile;
    p.lds = (size_t)resamp_span(tile, step, Ls) * elem;
    return p;
}

// One output of resamp_kernel: the branch's FMA chain in tap order (bit-identical to the per-sample loop on exact data),
// four taps' reads together.  xp = the newest sample of the output's window (tap k reads xp[-k]), hrow = the branch's Ls
// taps.  Shared with symstreamr_kernel, which runs it from samples it has just formed in LDS.
template <class T, class C>
__device__ __forceinline__ T resamp_branch_dot(const T *xp, const C *__restrict__ hrow, int Ls) {
    T acc = zero_of<T>();
    int k = 0;
    if constexpr (std::is_same<C, float>::value) {
        if ((Ls & 1) == 0) {                    // even rows (Ls = 2m) start 8-byte aligned: the taps in pairs
            const float2 *h2 = reinterpret_cast<const float2 *>(hrow);
            for (; k + 4 <= Ls; k += 4) {
                const T x0 = xp[-k], x1 = xp[-k - 1], x2 = xp[-k - 2], x3 = xp[-k - 3];
                const float2 ha = h2[k >> 1], hc = h2[(k >> 1) + 1];
                acc = mac(acc, x0, ha.x);
                acc = mac(acc, x1, ha.y);
                acc = mac(acc, x2, hc.x);
                acc = mac(acc, x3, hc.y);
            }
            if (k < Ls) {
                const float2 ha = h2[k >> 1];
                acc = mac(acc, xp[-k], ha.x);
                acc = mac(acc, xp[-k - 1], ha.y);
                k += 2;
            }
        }
    }
    for (; k + 4 <= Ls; k += 4) {
        const T x0 = xp[-k], x1 = xp[-k - 1], x2 = xp[-k - 2], x3 = xp[-k - 3];
        const C h0 = hrow[k], h1 = hrow[k + 1], h2 = hrow[k + 2], h3 = hrow[k + 3];
        acc = mac(acc, x0, h0);
        acc = mac(acc, x1, h1);
        acc = mac(acc, x2, h2);
        acc = mac(acc, x3, h3);
    }
    for (; k < Ls; ++k) acc = mac(acc, xp[-k], hrow[k]);
    return acc;
}

// One branch of a polyphase bank at one input sample, as the last nf % 4 branches of firpfb_fewbranch_body form it: the
// chain over the taps in order, then the scale.  xr = the newest sample (tap k reads xr[-k]), h0 = the branch's Ls taps.
template <class T, class C>
__device__ __forceinline__ T pfb_branch_dot(const T *xr, const C *__restrict__ h0, int Ls, C scale) {
    T acc = zero_of<T>();
    for (int k = 0; k < Ls; ++k) acc = mac(acc, xr[-k], h0[k]);
    return mul(acc, scale);
}

// ---- the LFSR symbol source of symstream_kernel and symstreamr_kernel ------------------------------------------------
// the matrix (32 column words) applied to s.  All 32 columns, unrolled: the matrix then comes in two wide scalar loads
// and one wait; a loop over the m columns a state can have set waits for a scalar load per column, and that latency
// (a few hundred cycles, 20 matrices deep) was most of a workgroup's time.
__device__ __forceinline__ unsigned sym_apply(const unsigned *__restrict__ M, unsigned s) {
    unsigned acc = 0u;
#pragma unroll
    for (int j = 0; j < 32; ++j) acc ^= (0u - ((s >> j) & 1u)) & M[j];
    return acc;
}

// s0 advanced by `off` bits with the T^(2^b) matrices; wave-uniform where the arguments are
__device__ __forceinline__ unsigned sym_jump(const unsigned *__restrict__ pow, unsigned s0, unsigned long long off) {
    unsigned s = s0;
    for (int b = 0; off != 0; ++b, off >>= 1)
        if (off & 1u) s = sym_apply(pow + 32 * b, s);
    return s;
}

// Lane `tid` of a workgroup: from the state `s` at the first of `ngen` consecutive symbols, add tid * run symbols with
// the eight lane-stride matrices T^(run * bps * 2^b), step its `run` symbols and leave tab[symbol] in dst[tid * run ..].
template <class T>
__device__ __forceinline__ void sym_lane_fill(const unsigned *__restrict__ stride, unsigned s, int tid, int run, int bps,
                                              unsigned g, unsigned nmask, const T *tab, T *dst, int ngen) {
#pragma unroll
    for (int b = 0; b < kSymStrides; ++b) {
        const unsigned t = sym_apply(stride + 32 * b, s);
        s = ((tid >> b) & 1) ? t : s;
    }
    int e = tid * run;
    for (int r = 0; r < run; ++r, ++e) {
        unsigned v = 0u;
        for (int c = 0; c < bps; ++c) {
            const unsigned bit = (unsigned)__popc(s & g) & 1u;
            s = ((s << 1) | bit) & nmask;
            v = (v << 1) | bit;
        }
        if (e < ngen) dst[e] = tab[v];
    }
}

}  // namespace yagi
