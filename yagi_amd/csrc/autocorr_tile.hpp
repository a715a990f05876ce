// autocorr_tile.hpp -- the front end that autocorr_kernels.hip and burstdet_kernels.hip share: a tile's sums
//     rxx[n] = sum_i X[n-W+1+i] conj(X[n-W+1+i-d]),  energy[n] = sum_i |X[n-W+1+i]|^2,  i = 0 .. W-1 in that order from +0.0,
// every product and every add rounded on its own.  Both files are built with -ffp-contract=off and hold
// no f32 FMA (tests/test_autocorr_isa_cpu.py, tests/test_burstdet_isa_cpu.py).
//
// Rounding points.  With a = X[k] and b = X[k - d] (so v = conj(b)), num-complex's product a * conj(b) is
//     re = fl(a.re b.re) - fl(a.im (-b.im)) = fl(a.re b.re) + fl(a.im b.im)
//     im = fl(a.re (-b.im)) + fl(a.im b.re) = fl(a.im b.re) - fl(a.re b.im)
// exactly (a negation is exact and x - (-y) = x + y), so the kernel never forms the conjugate.  At d = 0 this makes
// rxx.re the energy's own expression and rxx.im = fl(p) - fl(p) = +0.0.
//
// The term of sample k, P[k] = X[k] conj(X[k - d]) and E[k] = |X[k]|^2, is the same rounded value in each of the W
// outputs it enters: only the sums differ from output to output, and each of them keeps its own order.  So the products
// are formed once per sample and every output costs W complex adds, not W complex multiply-adds.
//
// ac_tile_sums<T, ENERGY>: a workgroup of 256 lanes owns kAutocorrTile consecutive outputs.  It reads the two spans
// of cnt + W - 1 samples the tile needs -- the current one, which starts W - 1 samples in front of the tile, and the
// same span d samples earlier, each sample from x or from the object's history in front of x[0] -- and stages their
// terms P (and E) in LDS.  Lane t owns the kAutocorrR consecutive outputs t R .. t R + R - 1 and slides a register
// window of R + 4 terms along them: four terms of all R outputs per 16-byte LDS read.  The terms lie in rows of R
// padded by 16 bytes, so that the 16 lanes a ds_read_b128 serves together, at consecutive rows, cover all 64 banks;
// every lane walks the same offsets from its own row, so that holds for every read of the loop.  Every workgroup also
// copies its share of the history the call leaves (the last W + d samples of history ++ x) into the other of the
// object's two buffers.
//
// LDS element per sample: cccf P as two floats and, with ENERGY, E in a second array; rrrf (P, E) as two floats with
// ENERGY, else P alone (autocorr_lds_bytes, kernels.hpp).
//
// Every global access is guarded by the block length: x is read in [0, nb), the history read and written in [0, W + d).
#pragma once

#include <algorithm>
#include <type_traits>

#include "kernels.hpp"

namespace yagi {
namespace {

typedef float ac_v2f __attribute__((ext_vector_type(2)));
typedef float ac_v4f __attribute__((ext_vector_type(4)));

constexpr int kWg = kAutocorrWg;
constexpr int kT = kAutocorrTile;
constexpr int kR = kAutocorrR;                         // outputs per lane
constexpr int kC = 4;                                  // terms per step of the window
constexpr int kStage = kT + kAutocorrWmax;             // staged positions: all a lane's last step can read
constexpr int kRows = kStage / kR;
constexpr int kPerLane = kStage / kWg;
constexpr int kHistWgs = 1024;                         // workgroups that share the copy of the history
static_assert(kR == 8 && kT == kWg * kR && kStage % kWg == 0 && kAutocorrWmax % kC == 0,
              "a lane reads its row as 16-byte words and steps by half a row");

// LDS word offset of position p in rows of kR elements of `words` words each, padded by four words
template <int words>
__device__ __forceinline__ int ac_at(int p) {
    return (p / kR) * (kR * words + 4) + (p % kR) * words;
}

// element k of a window held as 16-byte words
template <int words>
__device__ __forceinline__ auto ac_elem(const ac_v4f *w, int k) {
    if constexpr (words == 2) {
        const ac_v4f q = w[k / 2];
        return (k & 1) ? ac_v2f{q.z, q.w} : ac_v2f{q.x, q.y};
    } else {
        return w[k / 4][k % 4];
    }
}

// the shapes of autocorr_kernel<T, ENERGY> and of whatever shares its front end
template <class T, bool ENERGY>
struct AcShape {
    static constexpr bool CPLX = sizeof(T) == 2 * sizeof(float);
    static constexpr int VW = (CPLX || ENERGY) ? 2 : 1;             // words of the main LDS element: P, or (P, E) of rrrf
    static constexpr bool SEP_E = CPLX && ENERGY;                   // E in an array of its own
    using X = std::conditional_t<CPLX, ac_v2f, float>;              // a sample
    using V = std::conditional_t<VW == 2, ac_v2f, float>;           // a main element
    static constexpr int kWordsV = kRows * (kR * VW + 4), kWordsE = SEP_E ? kRows * (kR + 4) : 0;
    static_assert((size_t)(kWordsV + kWordsE) * sizeof(float) == autocorr_lds_bytes(sizeof(T), ENERGY), "kernels.hpp");
};

// Lane tid's kR sums of the tile that starts at output t0 and holds cnt outputs: acc[r] is rxx (for rrrf with ENERGY,
// (rxx, energy)) and, for cccf with ENERGY, en[r] the energy of output t0 + tid kR + r.  s_lds holds kWordsV + kWordsE
// words.  The caller synchronises the workgroup before it reuses s_lds: the terms are being read until then.
template <class T, bool ENERGY>
__device__ __forceinline__ void ac_tile_sums(float *s_lds, const T *__restrict__ hist, T *__restrict__ hist_next,
                                             const T *__restrict__ x, size_t nb, int W, int d, size_t t0, int cnt,
                                             typename AcShape<T, ENERGY>::V (&acc)[kR],
                                             float (&en)[AcShape<T, ENERGY>::SEP_E ? kR : 1]) {
    using S = AcShape<T, ENERGY>;
    constexpr bool CPLX = S::CPLX, SEP_E = S::SEP_E;
    constexpr int VW = S::VW;
    using X = typename S::X;
    using V = typename S::V;
    float *const s_v = s_lds, *const s_e = s_lds + S::kWordsV;

    const int tid = (int)threadIdx.x;
    const int span = cnt + W - 1;                                   // position p is sample t0 + p - (W - 1)
    const long long H = (long long)W + (long long)d;                // hist = the H samples before x[0], oldest first
    const X *xe = reinterpret_cast<const X *>(x), *he = reinterpret_cast<const X *>(hist);

    {
        const long long first = (long long)t0 - (long long)(W - 1);
        X ua[kPerLane], ub[kPerLane];                               // a lane's loads are issued before the first is used
#pragma unroll
        for (int c = 0; c < kPerLane; ++c) {
            // every lane loads, past the span its last sample again, from an address picked without a branch
            const int p = std::min(tid + c * kWg, span - 1);
            const long long ga = first + p, gb = ga - (long long)d; // gb >= -(W - 1) - d > -H
            ua[c] = *(ga >= 0 ? xe + ga : he + (H + ga));
            ub[c] = *(gb >= 0 ? xe + gb : he + (H + gb));
        }
#pragma unroll
        for (int c = 0; c < kPerLane; ++c) {
            const int p = tid + c * kWg;
            if constexpr (CPLX) {
                const ac_v2f a = ua[c], b = ub[c];
                const float rr = a.x * b.x, ii = a.y * b.y, ir = a.y * b.x, ri = a.x * b.y;
                *reinterpret_cast<ac_v2f *>(s_v + ac_at<2>(p)) = ac_v2f{rr + ii, ir - ri};
                if constexpr (ENERGY) {
                    const float er = a.x * a.x, ei = a.y * a.y;
                    s_e[ac_at<1>(p)] = er + ei;
                }
            } else if constexpr (ENERGY) {
                *reinterpret_cast<ac_v2f *>(s_v + ac_at<2>(p)) = ac_v2f{ua[c] * ub[c], ua[c] * ua[c]};
            } else {
                s_v[ac_at<1>(p)] = ua[c] * ub[c];
            }
        }
    }
    // the history the call leaves: the last H samples of hist ++ x, shared among the first kHistWgs workgroups (the loop
    // is kept rolled: a runtime trip count would cost a division)
    if (blockIdx.x < (unsigned)kHistWgs) {
        X *hn = reinterpret_cast<X *>(hist_next);
        const int Hi = W + d, step = (int)std::min(gridDim.x, (unsigned)kHistWgs) * kWg;
#pragma unroll 1
        for (int j = (int)blockIdx.x * kWg + tid; j < Hi; j += step) {
            const long long g = (long long)nb - H + j;
            hn[j] = g >= 0 ? xe[g] : he[(long long)j + (long long)nb];
        }
    }
    __syncthreads();

    // the register windows, kept as the 16-byte words they are read as: element k of wv is ac_elem<VW>(wv, k)
    constexpr int kWv = (kR + kC) * VW / 4, kStepV = kC * VW / 4;   // words of a window, and of one step of it
    const float *rv = s_v + tid * (kR * VW + 4), *re_ = s_e + tid * (kR + 4);
    ac_v4f wv[kWv], we[SEP_E ? (kR + kC) / 4 : 1];
    // positions q .. q + 3 of the lane (q a multiple of 4) into step w of the windows: row q / R from its own, either half
    auto fetch = [&](int q, int w) {
#pragma unroll
        for (int v = 0; v < kStepV; ++v) wv[w * kStepV + v] = *reinterpret_cast<const ac_v4f *>(rv + ac_at<VW>(q) + 4 * v);
        if constexpr (SEP_E) we[w] = *reinterpret_cast<const ac_v4f *>(re_ + ac_at<1>(q));
    };
    // term t of all R outputs; rot = which of the window's three steps is its first
    auto terms = [&](int t, int rot) {
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const int k = ((r + t) / kC + rot) % 3 * kC + (r + t) % kC;
            acc[r] = acc[r] + ac_elem<VW>(wv, k);
            if constexpr (SEP_E) en[r] = en[r] + ac_elem<1>(we, k);
        }
    };
    // four terms of all R outputs: the next step of the window is read into the slot behind the two in use
    auto chunk = [&](int c, int rot) {
        fetch(kR + kC * c, (rot + 2) % 3);
#pragma unroll
        for (int t = 0; t < kC; ++t) terms(t, rot);
    };
    fetch(0, 0);
    fetch(kC, 1);
#pragma unroll
    for (int r = 0; r < kR; ++r) acc[r] = V(0.0f);
    if constexpr (SEP_E) {
#pragma unroll
        for (int r = 0; r < kR; ++r) en[r] = 0.0f;
    }

    const int full = W / kC, rem = W - full * kC;                   // the same for every lane
    int c = 0;
#pragma unroll 1
    for (; c + 3 <= full; c += 3) {                                 // three steps on, the window's slots are where they
        chunk(c, 0);                                                // were: no register is moved
        chunk(c + 1, 1);
        chunk(c + 2, 2);
    }
#pragma unroll 1
    for (; c < full; ++c) {
        chunk(c, 0);
#pragma unroll
        for (int v = 0; v < kWv - kStepV; ++v) wv[v] = wv[v + kStepV];
        if constexpr (SEP_E) {
            we[0] = we[1];
            we[1] = we[2];
        }
    }
    if (rem) {
        fetch(kR + kC * full, 2);
#pragma unroll
        for (int t = 0; t < kC - 1; ++t) {
            if (t < rem) terms(t, 0);
        }
    }
}

}  // namespace
}  // namespace yagi
