// autocorr_kernels.hip -- Autocorr (yagi_hip.h; src/filter/autocorr.rs is an empty file): over a block, for every sample
// n, rxx[n] = sum_i X[n-W+1+i] conj(X[n-W+1+i-d]) and energy[n] = sum_i |X[n-W+1+i]|^2, i = 0 .. W-1 in that order from
// +0.0, every product and every add rounded on its own -- the reference's Window and dotprod composed.
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
// autocorr_kernel<T, ENERGY>: a workgroup of 256 lanes owns kAutocorrTile consecutive outputs.  It reads the two spans
// of cnt + W - 1 samples the tile needs -- the current one, which starts W - 1 samples in front of the tile, and the
// same span d samples earlier, each sample from x or from the object's history in front of x[0] -- and stages their
// terms P (and E) in LDS.  Lane t owns the kAutocorrR consecutive outputs t R .. t R + R - 1 and slides a register
// window of R + 4 terms along them: four terms of all R outputs per 16-byte LDS read.  The terms lie in rows of R
// padded by 16 bytes, so that the 16 lanes a ds_read_b128 serves together, at consecutive rows, cover all 64 banks;
// every lane walks the same offsets from its own row, so that holds for every read of the loop.  The outputs go back
// through LDS and leave as contiguous stores.  Every workgroup also copies its share of the history the call leaves
// (the last W + d samples of history ++ x) into the other of the object's two buffers.
//
// LDS element per sample: cccf P as two floats and, with ENERGY, E in a second array; rrrf (P, E) as two floats with
// ENERGY, else P alone (autocorr_lds_bytes, kernels.hpp).
//
// Every global access is guarded by the block length: x is read in [0, nb), rxx / energy written in [0, nb), the
// history read and written in [0, W + d).
//
// The Makefile builds this file with -ffp-contract=off; tests/test_autocorr_isa_cpu.py checks that the kernels hold no
// f32 FMA and no scratch.
#pragma clang fp contract(off)

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

template <class T, bool ENERGY>
__global__ void __launch_bounds__(kWg) autocorr_kernel(const T *__restrict__ hist, T *__restrict__ hist_next,
                                                       const T *__restrict__ x, size_t nb, T *__restrict__ rxx,
                                                       float *__restrict__ energy, int W, int d) {
    constexpr bool CPLX = sizeof(T) == 2 * sizeof(float);
    constexpr int VW = (CPLX || ENERGY) ? 2 : 1;                    // words of the main LDS element: P, or (P, E) of rrrf
    constexpr bool SEP_E = CPLX && ENERGY;                          // E in an array of its own
    using X = std::conditional_t<CPLX, ac_v2f, float>;              // a sample
    using V = std::conditional_t<VW == 2, ac_v2f, float>;           // a main element
    constexpr int kWordsV = kRows * (kR * VW + 4), kWordsE = SEP_E ? kRows * (kR + 4) : 0;
    static_assert((size_t)(kWordsV + kWordsE) * sizeof(float) == autocorr_lds_bytes(sizeof(T), ENERGY), "kernels.hpp");
    __shared__ __attribute__((aligned(16))) float s_lds[kWordsV + kWordsE];
    float *const s_v = s_lds, *const s_e = s_lds + kWordsV;

    const int tid = (int)threadIdx.x;
    const size_t t0 = (size_t)blockIdx.x * kT;
    const int cnt = (int)std::min((size_t)kT, nb - t0);             // outputs of this tile
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
    V acc[kR];
    float en[SEP_E ? kR : 1];
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
