// fdelay_kernels.hip -- block forms of Fdelay (src/filter/fdelay.rs): a fixed delay over a block, and one delay per sample.
//
// Closed form.  The object pushes every input into a Window of nmax + 1 samples, reads index(w) of it (the sample
// D = nmax - w steps back) and pushes THAT into FirPfbFilter::default(npfb, m), whose branch f it executes.  With X the
// input stream (zero before the first sample after reset) and D[n], f[n] the lag and branch in force at step n:
//     V[n] = X[n - D[n]]                                         the bank's input: fixed by the lag AT step n
//     y[n] = (sum_{k < Ls} H[f[n]][k] V[n - (Ls - 1) + k]) scale   H[i][k] = h[i + (Ls - 1 - k) npfb], Ls = h_len div npfb
// Nothing feeds back, so every output of a call is independent.  The state a call leaves is the last nmax samples of X
// and the last Ls values of V (fdelay_state_kernel; the kernels read one buffer and write the other).  The sums run
// k = 0 .. Ls-1 from +0.0 with unfused f32 products and adds, and (D, f) of the track form repeat set_delay's f32 steps
// (:80-89), so every output word equals the reference's sequential loop.
//
// fdelay_block_kernel (uniform D, f): a workgroup owns kWg * R consecutive outputs (R = 8 real, 4 complex: 32 bytes).
// It stages V over the tile and its Ls - 1 halo in LDS -- one contiguous span of x read at offset -D, the object's two
// histories in front of it, so the cost does not depend on nmax -- and each lane slides a register window over its LDS
// row (two 16-byte LDS reads per R taps of R outputs).  The one tap row is wave-uniform and comes through the scalar
// cache.  The outputs leave through LDS as contiguous non-temporal stores.  Every staging loop issues its loads in batches
// (devmath.hpp: batched_for); a plain strided loop waited for each load and cost the block form 15-25 %.
// fdelay_track_kernel (delay per sample): a workgroup owns kFdTrackTile outputs.  It computes (D, f) of every sample of
// the tile and its halo, stages the span of x the lags can reach (nmax deep) in LDS when that fits kFdLdsBudget and
// gathers V from it, else gathers V from global memory through L2; it keeps V and f of the tile in LDS, and each lane
// gathers its output's tap row as firpfb_select_kernel does.
//
// The Makefile builds this file with -ffp-contract=off; tests/test_fdelay_isa_cpu.py checks that the kernels hold no
// f32 FMA and no scratch.
#pragma clang fp contract(off)

#include "devmath.hpp"
#include "kernels.hpp"

namespace yagi {
namespace {

typedef float fd_v4f __attribute__((ext_vector_type(4)));

constexpr int kWg = kFdWg;

// the reference's products and adds, one rounding each (oracle: MUL_TC(sample, tap), ADD_T)
__device__ __forceinline__ float fd_zero(float *) { return 0.0f; }
__device__ __forceinline__ cf32 fd_zero(cf32 *) { return cf32{0.0f, 0.0f}; }
__device__ __forceinline__ float fd_mul(float a, float b) { return a * b; }
__device__ __forceinline__ cf32 fd_mul(cf32 a, float b) { return cf32{a.re * b, a.im * b}; }
__device__ __forceinline__ cf32 fd_mul(cf32 a, cf32 b) {
    return cf32{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__device__ __forceinline__ float fd_add(float a, float b) { return a + b; }
__device__ __forceinline__ cf32 fd_add(cf32 a, cf32 b) { return cf32{a.re + b.re, a.im + b.im}; }

template <class K>
struct FdArgs {
    using T = typename K::T;
    using C = typename K::C;
    const T *xh;           // the last nmax samples of X before the call, oldest first
    const T *vh;           // the last Ls values of V before the call, oldest first
    const T *x;            // the call's n samples
    const float *delay;    // track form: n delays; block form: null
    const C *H;            // [npfb][Ls], row i against the window oldest first
    T *y;
    size_t n;
    int nmax, Ls, npfb;
    int D0, f0;            // block form: the lag and the branch
    C scale;
};

// set_delay :80-89 in f32: the lag D = nmax - w_index and the branch.  A delay that is not >= 0 counts as 0, one above
// nmax as nmax (the host form has validated its array; the device form documents the clamp).
__device__ __forceinline__ void fd_lag(float d, int nmax, int npfb, int &D, int &f) {
    const float fn = (float)nmax;
    if (!(d >= 0.0f)) d = 0.0f;
    if (d > fn) d = fn;
    const float offset = fn - d;
    const float ip = floorf(offset);
    const float frac = offset - ip;
    const float v = (float)npfb * frac;                  // >= 0: round half away from zero = floor, +1 from .5 up
    float r = floorf(v);
    if (v - r >= 0.5f) r = r + 1.0f;
    int w = (int)ip, fi = (int)r;
    while (fi >= npfb) { ++w; fi -= npfb; }
    if (w > nmax) w = nmax;                              // cannot happen for nmax <= 2^24 (create's limit): keeps reads in range
    D = nmax - w;
    f = fi;
}

template <class K>
__device__ __forceinline__ typename K::T fd_x(const FdArgs<K> &a, long long i) {      // X[i], i >= -nmax
    return i < 0 ? a.xh[a.nmax + i] : a.x[i];
}
// V[j], j >= -Ls: the stored history, else X at the lag of step j; zero past the call
template <class K, bool TRACK>
__device__ __forceinline__ typename K::T fd_v(const FdArgs<K> &a, long long j) {
    using T = typename K::T;
    if (j < 0) return a.vh[a.Ls + j];
    if ((size_t)j >= a.n) return fd_zero((T *)nullptr);
    int D = a.D0, f = 0;
    if (TRACK) fd_lag(a.delay[j], a.nmax, a.npfb, D, f);
    return fd_x(a, j - D);
}

template <class T> struct FdTile {
    static constexpr int R = 32 / (int)sizeof(T);        // consecutive outputs per lane: 32 bytes of LDS row
    static constexpr int N = kWg * R;                    // outputs per workgroup
};
// LDS row of the block kernel: the tile, the halo rounded up to whole chunks, and the slack the last chunk reads
template <class T>
__host__ __device__ constexpr int fd_row(int Ls) {
    return FdTile<T>::N + ((Ls + FdTile<T>::R - 1) / FdTile<T>::R) * FdTile<T>::R + FdTile<T>::R;
}

template <class T, int R>
__device__ __forceinline__ void fd_ld(T *dst, const T *src) {                         // R elements = 32 bytes, 16-byte aligned
    const fd_v4f a = *reinterpret_cast<const fd_v4f *>(src);
    const fd_v4f b = *(reinterpret_cast<const fd_v4f *>(src) + 1);
    __builtin_memcpy(dst, &a, 16);
    __builtin_memcpy(reinterpret_cast<char *>(dst) + 16, &b, 16);
}

// acc[r] += sum over taps k of row[r + k] * h[k], k ascending
template <class T, class C, int R>
__device__ __forceinline__ void fd_slide(const T *row, const C *__restrict__ h, int Ls, T (&acc)[R]) {
    T w[2 * R];
    fd_ld<T, R>(&w[0], row);
    const int full = Ls / R;
#pragma unroll 1
    for (int c = 0; c < full; ++c) {
        fd_ld<T, R>(&w[R], row + R * (c + 1));
        const C *hc = h + R * c;
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const C ht = hc[t];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = fd_add(acc[r], fd_mul(w[r + t], ht));
        }
#pragma unroll
        for (int e = 0; e < R; ++e) w[e] = w[R + e];
    }
    const int rem = Ls - full * R;                       // block-uniform
    if (rem) {
        fd_ld<T, R>(&w[R], row + R * (full + 1));
        const C *hc = h + R * full;
#pragma unroll
        for (int t = 0; t < R; ++t) {
            if (t < rem) {
                const C ht = hc[t];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fd_add(acc[r], fd_mul(w[r + t], ht));
            }
        }
    }
}

template <class K>
__global__ void __launch_bounds__(kWg) fdelay_block_kernel(FdArgs<K> a) {
    using T = typename K::T;
    using C = typename K::C;
    constexpr int R = FdTile<T>::R, N = FdTile<T>::N;
    extern __shared__ __align__(16) unsigned char fd_smem[];
    T *sV = reinterpret_cast<T *>(fd_smem);              // sV[t] = V[n0 - (Ls - 1) + t]
    const int tid = (int)threadIdx.x;
    const size_t n0 = (size_t)blockIdx.x * N;
    const int row = fd_row<T>(a.Ls);
    const long long j0 = (long long)n0 - (a.Ls - 1);
    const long long i0 = j0 - a.D0;                      // x index of sV[0]
    if (i0 >= 0 && (size_t)(i0 + row) <= a.n) {          // block-uniform: the whole row lies inside x
        const T *src = a.x + i0;                         // loads issued in batches before the LDS writes (devmath.hpp)
        batched_for<kWg>(row, [&](int t) { return ld_stream(src + t); }, [&](int t, T v) { sV[t] = v; });
    } else {
        batched_for<kWg>(row, [&](int t) { return fd_v<K, false>(a, j0 + t); }, [&](int t, T v) { sV[t] = v; });
    }
    __syncthreads();

    T acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = fd_zero((T *)nullptr);
    fd_slide<T, C, R>(sV + tid * R, a.H + (size_t)a.f0 * a.Ls, a.Ls, acc);
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = fd_mul(acc[r], a.scale);

    // the tile leaves through LDS: each lane's R outputs as 32 bytes, then contiguous stores
    __syncthreads();                                     // every lane is done with the staged span
    {
        fd_v4f o[2];
        __builtin_memcpy(o, acc, 32);
        fd_v4f *d = reinterpret_cast<fd_v4f *>(sV + tid * R);
        d[0] = o[0];
        d[1] = o[1];
    }
    __syncthreads();
    const size_t left = a.n - n0;
    const int nout = left < (size_t)N ? (int)left : N;
    T *yb = a.y + n0;
    if (nout == N && (reinterpret_cast<uintptr_t>(yb) & 15) == 0) {
        constexpr int V4 = N * (int)sizeof(T) / 16;
        for (int c = tid; c < V4; c += kWg)
            st_stream(reinterpret_cast<fd_v4f *>(yb) + c, reinterpret_cast<const fd_v4f *>(sV)[c]);
    } else {
        for (int t = tid; t < nout; t += kWg) yb[t] = sV[t];
    }
}

// XLDS: the span of x the tile's lags can reach is staged in LDS (it fits), else V is gathered from global memory
template <class K, bool XLDS>
__global__ void __launch_bounds__(kWg) fdelay_track_kernel(FdArgs<K> a) {
    using T = typename K::T;
    using C = typename K::C;
    constexpr int N = kFdTrackTile;
    extern __shared__ __align__(16) unsigned char fd_smem[];
    const int Ls = a.Ls, nmax = a.nmax;
    const int span = N + Ls - 1;
    T *sV = reinterpret_cast<T *>(fd_smem);              // sV[t] = V[n0 - (Ls - 1) + t]
    int *sF = reinterpret_cast<int *>(sV + span);        // sF[o] = branch of output n0 + o
    T *sX = reinterpret_cast<T *>(sF + N);               // XLDS: sX[u] = X[j0 - nmax + u], u < span + nmax
    const int tid = (int)threadIdx.x;
    const size_t n0 = (size_t)blockIdx.x * N;
    const long long j0 = (long long)n0 - (Ls - 1);
    if (XLDS) {
        const long long b = j0 - nmax;
        // below -nmax only where j < 0, which reads vh instead; loads issued in batches before the LDS writes
        batched_for<kWg>(span + nmax, [&](int u) {
            const long long i = b + u;
            return (i < -(long long)nmax || (i >= 0 && (size_t)i >= a.n)) ? fd_zero((T *)nullptr) : fd_x(a, i);
        }, [&](int u, T v) { sX[u] = v; });
        __syncthreads();
    }
    // the delays of the span in batches, then the lag, the branch and V of each sample
    batched_for<kWg>(span, [&](int t) {
        const long long j = j0 + t;
        return (j >= 0 && (size_t)j < a.n) ? a.delay[j] : 0.0f;
    }, [&](int t, float dl) {
        const long long j = j0 + t;
        T v = fd_zero((T *)nullptr);
        if (j < 0) {
            v = a.vh[Ls + j];
        } else if ((size_t)j < a.n) {
            int D, f;
            fd_lag(dl, nmax, a.npfb, D, f);
            v = XLDS ? sX[t + nmax - D] : fd_x(a, j - D);
            if (t >= Ls - 1) sF[t - (Ls - 1)] = f;
        }
        sV[t] = v;
    });
    __syncthreads();
    const size_t left = a.n - n0;
    const int nout = left < (size_t)N ? (int)left : N;
    for (int o = tid; o < nout; o += kWg) {
        const C *h = a.H + (size_t)sF[o] * Ls;
        T acc = fd_zero((T *)nullptr);
        for (int k = 0; k < Ls; ++k) acc = fd_add(acc, fd_mul(sV[o + k], h[k]));
        a.y[n0 + o] = fd_mul(acc, a.scale);
    }
}

// The histories the call leaves, thread p of nmax + Ls + 1: X[n - nmax + p], then V[n - Ls + p], then the delay in
// force after the call (the track's last one, clamped as fd_lag does), which the host reads back after a device track.
// It also covers a call shorter than either history: both streams continue into the old histories.
template <class K, bool TRACK>
__global__ void __launch_bounds__(256) fdelay_state_kernel(FdArgs<K> a, typename K::T *next, float delay0) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = (long long)a.n;
    if (g < a.nmax) {
        next[g] = fd_x(a, n - a.nmax + g);
    } else if (g < (long long)a.nmax + a.Ls) {
        next[g] = fd_v<K, TRACK>(a, n - a.Ls + (g - a.nmax));
    } else if (g == (long long)a.nmax + a.Ls) {
        float d = delay0;
        if (TRACK) {
            d = a.delay[a.n - 1];
            if (!(d >= 0.0f)) d = 0.0f;
            if (d > (float)a.nmax) d = (float)a.nmax;
        }
        *reinterpret_cast<float *>(next + g) = d;
    }
}

}  // namespace

template <class T>
size_t fdelay_state_bytes(int nmax, int Ls) {
    return ((size_t)nmax + (size_t)Ls + 1) * sizeof(T);
}
template size_t fdelay_state_bytes<float>(int, int);
template size_t fdelay_state_bytes<cf32>(int, int);

template <class K>
int launch_fdelay(const FdelayDims &dm, const typename K::C *H, typename K::C scale, const typename K::T *state,
                  typename K::T *state_next, int D, int f, float delay0, const float *delay, const typename K::T *x,
                  size_t n, typename K::T *y, hipStream_t st) {
    using T = typename K::T;
    if (n == 0) return YAGI_OK;
    if (dm.Ls > kFdMaxLs) return fail(YAGI_ERR_CONFIG, "fdelay: branch filters too long (%d taps)", dm.Ls);
    if (D < 0 || D > dm.nmax || f < 0 || f >= dm.npfb) return fail(YAGI_ERR_INTERNAL, "fdelay: lag out of range");
    FdArgs<K> a;
    a.xh = state;
    a.vh = state + dm.nmax;
    a.x = x;
    a.delay = delay;
    a.H = H;
    a.y = y;
    a.n = n;
    a.nmax = dm.nmax;
    a.Ls = dm.Ls;
    a.npfb = dm.npfb;
    a.D0 = D;
    a.f0 = f;
    a.scale = scale;
    const unsigned sblk = (unsigned)(((size_t)dm.nmax + dm.Ls + 1 + 255) / 256);
    if (delay == nullptr) {
        constexpr int N = FdTile<T>::N;
        const size_t tiles = (n + N - 1) / N;
        if (tiles > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
        fdelay_block_kernel<K><<<(unsigned)tiles, kWg, (size_t)fd_row<T>(dm.Ls) * sizeof(T), st>>>(a);
        YG_LAUNCH_CHECK();
        fdelay_state_kernel<K, false><<<sblk, 256, 0, st>>>(a, state_next, delay0);
    } else {
        constexpr int N = kFdTrackTile;
        const size_t tiles = (n + N - 1) / N;
        if (tiles > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
        const size_t span = (size_t)N + dm.Ls - 1;
        const size_t base = span * sizeof(T) + (size_t)N * sizeof(int);
        const size_t withx = base + (span + (size_t)dm.nmax) * sizeof(T);
        if (withx <= kFdLdsBudget) fdelay_track_kernel<K, true><<<(unsigned)tiles, kWg, withx, st>>>(a);
        else fdelay_track_kernel<K, false><<<(unsigned)tiles, kWg, base, st>>>(a);
        YG_LAUNCH_CHECK();
        fdelay_state_kernel<K, true><<<sblk, 256, 0, st>>>(a, state_next, delay0);
    }
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}
template int launch_fdelay<RRRF>(const FdelayDims &, const float *, float, const float *, float *, int, int, float,
                                 const float *, const float *, size_t, float *, hipStream_t);
template int launch_fdelay<CRCF>(const FdelayDims &, const float *, float, const cf32 *, cf32 *, int, int, float,
                                 const float *, const cf32 *, size_t, cf32 *, hipStream_t);
template int launch_fdelay<CCCF>(const FdelayDims &, const cf32 *, cf32, const cf32 *, cf32 *, int, int, float,
                                 const float *, const cf32 *, size_t, cf32 *, hipStream_t);

}  // namespace yagi
