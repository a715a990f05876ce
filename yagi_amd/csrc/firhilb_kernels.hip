// firhilb_kernels.hip -- block forms of FirHilbertFilter (src/filter/fir/firhilb.rs): decim, interp, r2c and c2r.
//
// Closed form.  Every mode pushes its inputs into two or four of the object's Window<f32>s of length L = 2m and reads
// index(m - 1) of one window and hq . read() of another.  Written as virtual streams V = window ++ pushed values, a call
// of n units needs, for "pair" i (one input pair of r2c / c2r, one unit of decim / interp):
//     QE(i) = sum_k hq[k] FE[i + 1 + k],   QO(i) = sum_k hq[k] FO[i + k],   DE(i) = DE[i + m],   DO(i) = DO[i + m]
// with these streams (t0 = the toggle at the call; x the call's floats):
//     r2c:    FE = DE = A ++ x[0::2],  FO = DO = B ++ x[1::2],  A = t0 ? w1 : w0, B the other
//             y[2i] = (DE, QO), y[2i + 1] = (DO, QE)
//     decim:  FE = w1 ++ x[0::2],  DO = w0 ++ x[1::2];   y[i] = +-(DO, QE), negated where t0 ^ (i & 1)
//     interp: FE = w1 ++ s x.re,  DO = w0 ++ s x.im (s = -1 where t0 ^ (i & 1));   y[2i] = DO, y[2i + 1] = QE
//     c2r:    DE = Ar ++ re of even inputs, FO = Bi ++ im of odd inputs, DO = Br ++ re of odd, FE = Ai ++ im of even,
//             (Ar, Ai, Br, Bi) = t0 ? (w2, w3, w0, w1) : (w0, w1, w2, w3);   y[4i..4i+4) = (DE+QO, DE-QO, DO+QE, DO-QE)
// Each window after the call is the last L values of its stream (firhilb_state_kernel), and the toggle advances by n,
// which the host tracks.  The sums run k = 0 .. L-1 from +0.0 with unfused f32 products and adds, the sign flips are
// sign flips, so every output word equals the reference's sequential loop.
//
// Fast form (m <= kFirhilbFastM): a workgroup owns kFirhilbTile pairs; it stages each stream's span (tile + halo) in LDS,
// de-interleaved, with one coalesced pass over the input, and each lane computes kFirhilbR consecutive pairs with a
// register window that slides over its LDS row (one 16-byte LDS read per 4 taps of 8 outputs).  The taps come through
// the scalar cache.  The outputs go back through LDS in output order and leave as contiguous 16-byte stores (lanes
// storing their own pairs, 128 B apart, reached half the rate).  Larger m: firhilb_general_kernel, one lane per pair reading the streams from global memory.
//
// The Makefile builds this file with -ffp-contract=off; tests/test_firhilb_isa_cpu.py checks that the kernels hold no
// f32 FMA and no scratch.
#pragma clang fp contract(off)

#include "kernels.hpp"

namespace yagi {
namespace {

typedef float fh_v2f __attribute__((ext_vector_type(2)));
typedef float fh_v4f __attribute__((ext_vector_type(4)));

constexpr int kR = kFirhilbR;
constexpr int kTile = kFirhilbTile;            // pairs per workgroup = kFirhilbWg * kR

// One virtual stream: V[q] = win[wi L + q] for q < L, else the call's float at stride * (q - L) + off (times the
// interp sign of its unit), zero past the end of the call.
struct FhStream {
    int wi, off, stride;
};

struct FhArgs {
    const float *win;          // 4 L floats: w0, w1, w2, w3, oldest first
    const float *x;            // the call's floats
    size_t nf;                 // number of floats in x
    size_t np;                 // pairs
    size_t n;                  // units of the call
    const float *hq;           // L taps
    float *y;
    int L, m, t0;
};

template <int MODE> struct FhMode;
// streams: FE, FO, DE, DO (FO / DE unused where the mode has none); stride = floats per pair of the input
template <> struct FhMode<FIRHILB_R2C> {
    static constexpr int S = 2;
    static constexpr bool kQO = true, kSign = false, kSepD = false;
    __device__ static FhStream fe(int t0) { return {t0 ? 1 : 0, 0, 2}; }
    __device__ static FhStream fo(int t0) { return {t0 ? 0 : 1, 1, 2}; }
    __device__ static FhStream de(int t0) { return fe(t0); }
    __device__ static FhStream dO(int t0) { return fo(t0); }
};
template <> struct FhMode<FIRHILB_DECIM> {
    static constexpr int S = 2;
    static constexpr bool kQO = false, kSign = false, kSepD = false;
    __device__ static FhStream fe(int) { return {1, 0, 2}; }
    __device__ static FhStream fo(int) { return {0, 1, 2}; }
    __device__ static FhStream de(int t0) { return fe(t0); }
    __device__ static FhStream dO(int t0) { return fo(t0); }
};
template <> struct FhMode<FIRHILB_INTERP> : FhMode<FIRHILB_DECIM> {
    static constexpr bool kSign = true;
};
template <> struct FhMode<FIRHILB_C2R> {
    static constexpr int S = 4;
    static constexpr bool kQO = true, kSign = false, kSepD = true;
    __device__ static FhStream fe(int t0) { return {t0 ? 3 : 1, 1, 4}; }
    __device__ static FhStream fo(int t0) { return {t0 ? 1 : 3, 3, 4}; }
    __device__ static FhStream de(int t0) { return {t0 ? 2 : 0, 0, 4}; }
    __device__ static FhStream dO(int t0) { return {t0 ? 0 : 2, 2, 4}; }
};

// interp pushes -x where the toggle is set: a sign flip, exact on +-0 and NaN
__device__ __forceinline__ float fh_flip(float v, bool neg) {
    return __uint_as_float(__float_as_uint(v) ^ (neg ? 0x80000000u : 0u));
}

template <bool SIGN>
__device__ __forceinline__ float fh_value(const FhArgs &a, const FhStream &s, long long q) {
    if (q < a.L) return a.win[s.wi * a.L + (int)q];
    const size_t k = (size_t)(q - a.L);
    const size_t f = (size_t)s.stride * k + (size_t)s.off;
    if (f >= a.nf) return 0.0f;
    const float v = a.x[f];
    return SIGN ? fh_flip(v, ((unsigned)a.t0 ^ (unsigned)(k & 1)) != 0) : v;
}

// acc[r] += sum over taps k of hq[k] * row[r + k], k ascending; row is the lane's LDS row (16-byte aligned)
__device__ __forceinline__ void fh_slide(const float *row, const float *__restrict__ hq, int L, float (&acc)[kR]) {
    float w[2 * kR];
    *reinterpret_cast<fh_v4f *>(&w[0]) = *reinterpret_cast<const fh_v4f *>(row);
    *reinterpret_cast<fh_v4f *>(&w[4]) = *reinterpret_cast<const fh_v4f *>(row + 4);
    const int full = L / kR;
#pragma unroll 1
    for (int c = 0; c < full; ++c) {
        *reinterpret_cast<fh_v4f *>(&w[kR]) = *reinterpret_cast<const fh_v4f *>(row + kR * (c + 1));
        *reinterpret_cast<fh_v4f *>(&w[kR + 4]) = *reinterpret_cast<const fh_v4f *>(row + kR * (c + 1) + 4);
        const float *h = hq + kR * c;
#pragma unroll
        for (int t = 0; t < kR; ++t) {
            const float ht = h[t];
#pragma unroll
            for (int r = 0; r < kR; ++r) acc[r] = acc[r] + ht * w[r + t];
        }
#pragma unroll
        for (int e = 0; e < kR; ++e) w[e] = w[kR + e];
    }
    const int rem = L - full * kR;                       // block-uniform
    if (rem) {
        *reinterpret_cast<fh_v4f *>(&w[kR]) = *reinterpret_cast<const fh_v4f *>(row + kR * (full + 1));
        *reinterpret_cast<fh_v4f *>(&w[kR + 4]) = *reinterpret_cast<const fh_v4f *>(row + kR * (full + 1) + 4);
        const float *h = hq + kR * full;
#pragma unroll
        for (int t = 0; t < kR; ++t) {
            if (t < rem) {
                const float ht = h[t];
#pragma unroll
                for (int r = 0; r < kR; ++r) acc[r] = acc[r] + ht * w[r + t];
            }
        }
    }
}

// LDS row length of a dotted stream: the tile, the halo, and the slack the last chunk of fh_slide reads
__host__ __device__ constexpr int fh_frow(int L) { return kTile + ((L + kR - 1) / kR) * kR + kR; }

template <int MODE>
__global__ void __launch_bounds__(kFirhilbWg) firhilb_block_kernel(FhArgs a) {
    using M = FhMode<MODE>;
    extern __shared__ __align__(16) float fh_smem[];
    const int L = a.L, m = a.m;
    const int frow = fh_frow(L);
    float *sFE = fh_smem;                                  // FE[i0 + 1 + t]
    float *sFO = sFE + frow;                               // FO[i0 + t]
    float *sDE = M::kQO ? sFO + frow : sFO;                // c2r: DE[i0 + m + t]
    float *sDO = sDE + (M::kSepD ? kTile : 0);             // decim / interp / c2r: DO[i0 + m + t]
    const int tid = (int)threadIdx.x;
    const size_t i0 = (size_t)blockIdx.x * kTile;
    const FhStream fe = M::fe(a.t0), fo = M::fo(a.t0), de = M::de(a.t0), dO = M::dO(a.t0);

    // staging: virtual pair index q over [i0, i0 + span); each lane loads P pairs (16 bytes) at a time where they are in
    // range and the input is 16-byte aligned, else element by element
    const int span = kTile + L + kR;
    constexpr int P = 4 / M::S;                          // pairs per 16-byte load
    const bool vec = (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
    for (int t0 = tid * P; t0 < span; t0 += kFirhilbWg * P) {
        float v[P][M::S];
        const long long k0 = (long long)i0 + t0 - L;     // even where P = 2 (i0, t0 and L are)
        if (k0 >= 0 && vec && (size_t)(k0 + P) * M::S <= a.nf) {
            const fh_v4f g = *reinterpret_cast<const fh_v4f *>(a.x + (size_t)k0 * M::S);
            const float gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const bool neg = M::kSign && ((unsigned)a.t0 ^ (unsigned)((k0 + p) & 1));
#pragma unroll
                for (int e = 0; e < M::S; ++e) v[p][e] = fh_flip(gg[p * M::S + e], neg);
            }
        } else {
            // window part, a partial pair at the end, past the end, or an input not 16-byte aligned
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const long long q = (long long)i0 + t0 + p;
                v[p][fe.off] = fh_value<M::kSign>(a, fe, q);
                v[p][fo.off] = fh_value<M::kSign>(a, fo, q);
                if constexpr (M::S == 4) {
                    v[p][de.off] = fh_value<M::kSign>(a, de, q);
                    v[p][dO.off] = fh_value<M::kSign>(a, dO, q);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int t = t0 + p;
            if (t >= span) break;
            if (t >= 1) sFE[t - 1] = v[p][fe.off];
            if (M::kQO && t < frow) sFO[t] = v[p][fo.off];
            const int td = t - m;
            if (td >= 0 && td < kTile) {
                if (M::kSepD) sDE[td] = v[p][de.off];
                if (!M::kQO || M::kSepD) sDO[td] = v[p][dO.off];
            }
        }
    }
    __syncthreads();

    const int l0 = tid * kR;
    float qe[kR], qo[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) qe[r] = qo[r] = 0.0f;
    fh_slide(sFE + l0, a.hq, L, qe);
    if constexpr (M::kQO) fh_slide(sFO + l0, a.hq, L, qo);

    // outputs: each lane's kR pairs into LDS in output order (a 16-byte pad after every lane's row keeps the rows on
    // different banks), then the tile leaves as contiguous 16-byte stores
    constexpr int OPF = M::kQO ? 4 : 2;                  // output floats per pair
    float o[kR][OPF];
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        if constexpr (MODE == FIRHILB_R2C) {
            o[r][0] = sFE[l0 + r + m - 1];
            o[r][1] = qo[r];
            o[r][2] = sFO[l0 + r + m];
            o[r][3] = qe[r];
        } else if constexpr (MODE == FIRHILB_C2R) {
            const float dE = sDE[l0 + r], dOv = sDO[l0 + r];
            o[r][0] = dE + qo[r];
            o[r][1] = dE - qo[r];
            o[r][2] = dOv + qe[r];
            o[r][3] = dOv - qe[r];
        } else if constexpr (MODE == FIRHILB_DECIM) {
            const bool neg = ((unsigned)a.t0 ^ (unsigned)((i0 + l0 + r) & 1)) != 0;
            o[r][0] = fh_flip(sDO[l0 + r], neg);
            o[r][1] = fh_flip(qe[r], neg);
        } else {
            o[r][0] = sDO[l0 + r];
            o[r][1] = qe[r];
        }
    }
    __syncthreads();                                     // every lane is done with the staged streams
    constexpr int ROW = kR * OPF + 4;
    float *sOut = fh_smem;
#pragma unroll
    for (int r = 0; r < kR; ++r)
#pragma unroll
        for (int e = 0; e < OPF; e += 2)
            *reinterpret_cast<fh_v2f *>(sOut + tid * ROW + r * OPF + e) = fh_v2f{o[r][e], o[r][e + 1]};
    __syncthreads();
    const size_t ytot = 2 * a.n;                         // output floats of the call
    const size_t yb = i0 * OPF;
    const int nout = (int)((ytot - yb) < (size_t)(kTile * OPF) ? (ytot - yb) : (size_t)(kTile * OPF));
    if ((reinterpret_cast<uintptr_t>(a.y) & 15) == 0 && nout == kTile * OPF) {
        for (int c = tid; c < kTile * OPF / 4; c += kFirhilbWg) {
            const int w = 4 * c;
            *reinterpret_cast<fh_v4f *>(a.y + yb + w) = *reinterpret_cast<const fh_v4f *>(sOut + w + (w / (kR * OPF)) * 4);
        }
    } else {
        for (int w = tid; w < nout; w += kFirhilbWg) a.y[yb + w] = sOut[w + (w / (kR * OPF)) * 4];
    }
}

// any m: one lane per pair, the streams read from global memory (the same sums in the same order)
template <int MODE>
__global__ void __launch_bounds__(256) firhilb_general_kernel(FhArgs a) {
    using M = FhMode<MODE>;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.np) return;
    const FhStream fe = M::fe(a.t0), fo = M::fo(a.t0), de = M::de(a.t0), dO = M::dO(a.t0);
    const long long q = (long long)i;
    float qe = 0.0f, qo = 0.0f;
    for (int k = 0; k < a.L; ++k) qe = qe + a.hq[k] * fh_value<M::kSign>(a, fe, q + 1 + k);
    if constexpr (M::kQO)
        for (int k = 0; k < a.L; ++k) qo = qo + a.hq[k] * fh_value<M::kSign>(a, fo, q + k);
    const float dE = fh_value<M::kSign>(a, de, q + a.m), dOv = fh_value<M::kSign>(a, dO, q + a.m);
    float *yp = a.y + 4 * i;
    if constexpr (MODE == FIRHILB_R2C) {
        yp[0] = dE; yp[1] = qo;
        if (2 * i + 1 < a.n) { yp[2] = dOv; yp[3] = qe; }
    } else if constexpr (MODE == FIRHILB_C2R) {
        yp[0] = dE + qo; yp[1] = dE - qo;
        if (2 * i + 1 < a.n) { yp[2] = dOv + qe; yp[3] = dOv - qe; }
    } else if constexpr (MODE == FIRHILB_DECIM) {
        const bool neg = ((unsigned)a.t0 ^ (unsigned)(i & 1)) != 0;
        a.y[2 * i] = fh_flip(dOv, neg);
        a.y[2 * i + 1] = fh_flip(qe, neg);
    } else {
        a.y[2 * i] = dOv;
        a.y[2 * i + 1] = qe;
    }
}

// the windows the call leaves: window w = the last L values of the stream that feeds it (w2 and w3 of r2c, decim and
// interp are copied).  Thread (w, p) of 4 L.
template <int MODE>
__global__ void __launch_bounds__(256) firhilb_state_kernel(FhArgs a, float *next) {
    using M = FhMode<MODE>;
    const int g = (int)(blockIdx.x * 256 + threadIdx.x);
    if (g >= 4 * a.L) return;
    const int w = g / a.L, p = g - w * a.L;
    const FhStream ss[4] = {M::fe(a.t0), M::fo(a.t0), M::de(a.t0), M::dO(a.t0)};
    float v = a.win[g];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const FhStream s = ss[e];
        if (s.wi == w) {
            const size_t cnt = a.nf > (size_t)s.off ? (a.nf - (size_t)s.off + (size_t)s.stride - 1) / (size_t)s.stride : 0;
            v = fh_value<M::kSign>(a, s, (long long)cnt + p);
            break;
        }
    }
    next[g] = v;
}

template <int MODE>
int run_firhilb(const FhArgs &a, float *next, hipStream_t st) {
    if (a.np > 0) {
        if (a.m <= kFirhilbFastM) {
            using M = FhMode<MODE>;
            const size_t tiles = (a.np + kTile - 1) / kTile;
            const int frow = fh_frow(a.L);
            const size_t in = (size_t)frow * (M::kQO ? 2 : 1) + (M::kSepD ? 2 : (M::kQO ? 0 : 1)) * kTile;
            const size_t out = (size_t)kFirhilbWg * (kR * (M::kQO ? 4 : 2) + 4);
            const size_t lds = sizeof(float) * (in > out ? in : out);
            firhilb_block_kernel<MODE><<<(unsigned)tiles, kFirhilbWg, lds, st>>>(a);
        } else {
            firhilb_general_kernel<MODE><<<(unsigned)((a.np + 255) / 256), 256, 0, st>>>(a);
        }
        YG_LAUNCH_CHECK();
    }
    firhilb_state_kernel<MODE><<<(unsigned)((4 * a.L + 255) / 256), 256, 0, st>>>(a, next);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

}  // namespace

int launch_firhilb(int mode, int m, const float *hq, const float *win, float *win_next, int toggle, const float *x,
                   size_t n, float *y, hipStream_t st) {
    if (n == 0) return YAGI_OK;
    if (((uintptr_t)x | (uintptr_t)y) & 3) return fail(YAGI_ERR_CONFIG, "firhilb: buffers must be 4-byte aligned");
    FhArgs a;
    a.win = win;
    a.x = x;
    a.hq = hq;
    a.y = y;
    a.L = 2 * m;
    a.m = m;
    a.t0 = toggle ? 1 : 0;
    a.n = n;
    switch (mode) {
    case FIRHILB_R2C:
        a.nf = n;
        a.np = (n + 1) / 2;
        return run_firhilb<FIRHILB_R2C>(a, win_next, st);
    case FIRHILB_C2R:
        a.nf = 2 * n;
        a.np = (n + 1) / 2;
        return run_firhilb<FIRHILB_C2R>(a, win_next, st);
    case FIRHILB_DECIM:
        a.nf = 2 * n;
        a.np = n;
        return run_firhilb<FIRHILB_DECIM>(a, win_next, st);
    case FIRHILB_INTERP:
        a.nf = 2 * n;
        a.np = n;
        return run_firhilb<FIRHILB_INTERP>(a, win_next, st);
    default:
        return fail(YAGI_ERR_CONFIG, "firhilb: unknown mode %d", mode);
    }
}

}  // namespace yagi
