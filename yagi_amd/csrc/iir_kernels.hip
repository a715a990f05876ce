// iir_kernels.hip -- IirFilter (src/filter/iir/iirfilt.rs) as a block-parallel chunked state scan (kernels.hpp).
//
// One lane owns one chunk of T consecutive samples and runs the reference's per-sample recurrence over it in f32, in
// the reference's operation order (products unfused, sums left to right): the transfer-function form is the DF2 step
// over the VecDeque (iirfilt.rs:359-374) with the two-slice dot product of dotprod/mod.rs:75-121, whose split point
// follows the deque's physical head; the second-order-section form is the cascade of IirFilterSos::execute_df2
// (iirfiltsos.rs:103-117).  Chunks start from states that come out of an f64 scan over the power tables
// P_k = A^(T 2^k); the only difference from the sequential f32 path is the rounding of each chunk's initial state.
//
// A workgroup is one wave (64 chunks), so the cross-lane scan is a Hillis-Steele scan on shuffles, and global x / y
// go through an LDS tile of 64 chunks x kTs samples: the loads and stores are runs of kTs consecutive samples.
// The Makefile builds this file with -ffp-contract=off (the project's -ffp-contract=fast would override the pragma and
// fuse the recurrence); tests/test_iir_isa_cpu.py checks that no f32 FMA is left in the chunk kernels.
#pragma clang fp contract(off)

#include <type_traits>

#include "kernels.hpp"

namespace yagi {
namespace {

constexpr int kTs = 16;    // samples per LDS time slice

// ---- f32 arithmetic of the reference, unfused ---------------------------------------------------------------------
template <class T> __device__ __forceinline__ T izero();
template <> __device__ __forceinline__ float izero<float>() { return 0.0f; }
template <> __device__ __forceinline__ cf32 izero<cf32>() { return cf32{0.0f, 0.0f}; }
__device__ __forceinline__ float iadd(float a, float b) { return a + b; }
__device__ __forceinline__ cf32 iadd(cf32 a, cf32 b) { return cf32{a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ float isub(float a, float b) { return a - b; }
__device__ __forceinline__ cf32 isub(cf32 a, cf32 b) { return cf32{a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ float imul(float a, float b) { return a * b; }
__device__ __forceinline__ cf32 imul(cf32 a, float b) { return cf32{a.re * b, a.im * b}; }
__device__ __forceinline__ cf32 imul(cf32 a, cf32 b) { return cf32{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ float isel(bool c, float a, float b) { return c ? a : b; }
__device__ __forceinline__ cf32 isel(bool c, cf32 a, cf32 b) { return cf32{c ? a.re : b.re, c ? a.im : b.im}; }

// ---- f64 combine -------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dmac(double &acc, double m, double v) { acc = fma(m, v, acc); }
__device__ __forceinline__ void dmac(dcplx &acc, double m, dcplx v) { acc.re = fma(m, v.re, acc.re); acc.im = fma(m, v.im, acc.im); }
__device__ __forceinline__ void dmac(dcplx &acc, dcplx m, dcplx v) {
    acc.re = fma(m.re, v.re, fma(-m.im, v.im, acc.re));
    acc.im = fma(m.re, v.im, fma(m.im, v.re, acc.im));
}
__device__ __forceinline__ double dzero(double *) { return 0.0; }
__device__ __forceinline__ dcplx dzero(dcplx *) { return dcplx{0.0, 0.0}; }
__device__ __forceinline__ double to64(float v, double *) { return (double)v; }
__device__ __forceinline__ dcplx to64(cf32 v, dcplx *) { return dcplx{(double)v.re, (double)v.im}; }
__device__ __forceinline__ float from64(double v) { return (float)v; }
__device__ __forceinline__ cf32 from64(dcplx v) { return cf32{(float)v.re, (float)v.im}; }
// value selects (a ?: between two struct lvalues selects their addresses and keeps the arrays out of registers)
__device__ __forceinline__ double dpick(bool c, double a, double b) { return c ? a : b; }
__device__ __forceinline__ dcplx dpick(bool c, dcplx a, dcplx b) { return dcplx{c ? a.re : b.re, c ? a.im : b.im}; }
__device__ __forceinline__ double shup(double v, int d) { return __shfl_up(v, (unsigned)d, kWave); }
__device__ __forceinline__ dcplx shup(dcplx v, int d) {
    return dcplx{__shfl_up(v.re, (unsigned)d, kWave), __shfl_up(v.im, (unsigned)d, kWave)};
}

// Large states (32 entries, or 16 complex ones) would need a fully unrolled MAC nest the
// compiler declines to unroll; the copy of the old vector then goes through LDS (`vb`: each lane its own column) and
// the j loop stays rolled.
template <int SC, class V> struct BigState { static constexpr bool value = SC * sizeof(V) >= 256; };
template <int SC, class V> constexpr int vbuf_len() { return BigState<SC, V>::value ? SC * kIirWg : 1; }

// one S x S matrix of the power table into LDS (every lane of the wave calls it: the matrices are wave-uniform, and a
// chain of dependent global loads per MAC row was what bounded the combine)
template <class M>
__device__ __forceinline__ void stage_mat(M *__restrict__ dst, const M *__restrict__ src, int S, int lane) {
    __syncthreads();
    for (int e = lane; e < S * S; e += kIirWg) dst[e] = src[e];
    __syncthreads();
}

// s = P s + add (P in LDS: S x S row-major; entries of s at or beyond S are left alone)
template <int SC, class V, class M>
__device__ __forceinline__ void matvec_add(V (&s)[SC], const M *P, int S, const V (&add)[SC], V *vb, int lane) {
    if constexpr (BigState<SC, V>::value) {
#pragma unroll
        for (int j = 0; j < SC; ++j) {
            vb[j * kIirWg + lane] = s[j];
            s[j] = add[j];
        }
#pragma unroll 1
        for (int j = 0; j < S; ++j) {
            const V o = vb[j * kIirWg + lane];
#pragma unroll
            for (int i = 0; i < SC; ++i)
                if (i < S) dmac(s[i], P[i * S + j], o);
        }
    } else {
        V o[SC];
#pragma unroll
        for (int j = 0; j < SC; ++j) o[j] = s[j];
#pragma unroll
        for (int i = 0; i < SC; ++i) {
            if (i < S) {
                V acc = add[i];
#pragma unroll
                for (int j = 0; j < SC; ++j)
                    if (j < S) dmac(acc, P[i * S + j], o[j]);
                s[i] = acc;
            }
        }
    }
}

// inclusive scan over the 64 lanes of the wave: lane j ends with the state after the units (j-64, j], where one lane's
// unit spans 2^k0 chunks of T samples (P_{k0 + k} = the transfer over 2^k units, staged level by level in pl)
template <int SC, class V, class M>
__device__ __forceinline__ void wave_scan(V (&s)[SC], int S, const M *__restrict__ ptab, int k0, int lane, M *pl,
                                          V *vb) {
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        const int d = 1 << k;
        stage_mat(pl, ptab + (size_t)(k0 + k) * S * S, S, lane);
        const M *P = pl;
        if constexpr (BigState<SC, V>::value) {
#pragma unroll
            for (int i = 0; i < SC; ++i) vb[i * kIirWg + lane] = shup(s[i], d);
            if (lane >= d) {
#pragma unroll 1
                for (int j = 0; j < S; ++j) {
                    const V o = vb[j * kIirWg + lane];
#pragma unroll
                    for (int i = 0; i < SC; ++i)
                        if (i < S) dmac(s[i], P[i * S + j], o);
                }
            }
        } else {
            V o[SC];
#pragma unroll
            for (int i = 0; i < SC; ++i) o[i] = shup(s[i], d);
            if (lane >= d) {
#pragma unroll
                for (int i = 0; i < SC; ++i) {
                    if (i < S) {
#pragma unroll
                        for (int j = 0; j < SC; ++j)
                            if (j < S) dmac(s[i], P[i * S + j], o[j]);
                    }
                }
            }
        }
    }
}

// ---- the per-sample recurrences ----------------------------------------------------------------------------------
// transfer function, n = S + 1 <= SC + 1.  s[i] = the deque's logical v[i] after the previous step (v[0] newest);
// head = its physical head.  Returns the unscaled output.
template <class K, int SC>
__device__ __forceinline__ typename K::T tf_step(typename K::T (&s)[SC], int n, int &head, const IirParams<K> &p,
                                                 typename K::T x) {
    using T = typename K::T;
    head = (head == 0) ? n - 1 : head - 1;              // rotate_right(1) (len == capacity == n)
    const int split = (head == 0) ? n : n - head;       // as_slices(): the first slice holds logical [0, split)
    // v[0] = 0 during the feedback sum
    T l = iadd(izero<T>(), imul(izero<T>(), p.a[0])), r = izero<T>();
#pragma unroll
    for (int i = 1; i <= SC; ++i) {
        if (i < n) {
            const T q = imul(s[i - 1], p.a[i]);
            const bool first = i < split;
            l = iadd(l, isel(first, q, izero<T>()));
            r = iadd(r, isel(first, izero<T>(), q));
        }
    }
    const T w = isub(x, iadd(l, r));
    l = iadd(izero<T>(), imul(w, p.b[0]));
    r = izero<T>();
#pragma unroll
    for (int i = 1; i <= SC; ++i) {
        if (i < n) {
            const T q = imul(s[i - 1], p.b[i]);
            const bool first = i < split;
            l = iadd(l, isel(first, q, izero<T>()));
            r = iadd(r, isel(first, izero<T>(), q));
        }
    }
#pragma unroll
    for (int i = SC - 1; i > 0; --i) s[i] = s[i - 1];
    if (SC > 0) s[0] = w;
    return iadd(l, r);
}

// second-order sections: s[2k] = v[0], s[2k + 1] = v[1] of section k after the previous step
template <class K, int SC>
__device__ __forceinline__ typename K::T sos_step(typename K::T (&s)[SC], int nsec, const IirParams<K> &p,
                                                  typename K::T x) {
    using T = typename K::T;
    T u = x;
#pragma unroll
    for (int k = 0; k < SC / 2; ++k) {
        if (k < nsec) {
            const T v2 = s[2 * k + 1], v1 = s[2 * k];
            const T v0 = isub(isub(u, imul(v1, p.a[3 * k + 1])), imul(v2, p.a[3 * k + 2]));
            u = iadd(iadd(imul(v0, p.b[3 * k]), imul(v1, p.b[3 * k + 1])), imul(v2, p.b[3 * k + 2]));
            s[2 * k] = v0;
            s[2 * k + 1] = v1;
        }
    }
    return u;
}

// ---- I/O policies ------------------------------------------------------------------------------------------------
// A policy says how filter step gi of the call obtains its input and where, if anywhere, its output goes.  load() fills
// the workgroup's LDS tile (64 chunks x kTs steps) for the time slice at t0, store() empties it; element e = lane + 64 r
// of the tile is row e / kTs (the chunk), column e % kTs, which is step wg0 + row T + t0 + column.
template <class K>
struct PlainPolicy {                     // IirFilter: step gi reads x[gi] and writes y[gi]
    using T = typename K::T;
    const T *__restrict__ x;
    T *__restrict__ y;
    __device__ __forceinline__ void load(T (*tile)[kTs + 1], uint64_t wg0, uint64_t Tl, int t0, int lane, uint64_t n) const {
#pragma unroll
        for (int r = 0; r < kTs; ++r) {
            const int e = lane + r * kIirWg, j = e / kTs, tt = e % kTs;
            const uint64_t gi = wg0 + (uint64_t)j * Tl + (uint64_t)(t0 + tt);
            tile[j][tt] = (gi < n) ? x[gi] : izero<T>();
        }
    }
    __device__ __forceinline__ void store(T (*tile)[kTs + 1], uint64_t wg0, uint64_t Tl, int t0, int lane, uint64_t n) const {
#pragma unroll
        for (int r = 0; r < kTs; ++r) {
            const int e = lane + r * kIirWg, j = e / kTs, tt = e % kTs;
            const uint64_t gi = wg0 + (uint64_t)j * Tl + (uint64_t)(t0 + tt);
            if (gi < n) y[gi] = tile[j][tt];
        }
    }
};

// IirDecim / IirInterp: the sparse side holds one sample per M steps, sample gi / M at the steps with gi % M == 0.
// A 64-bit division per element would bring f32 multiply-adds into the kernel, so the workgroup's first step is split
// once in 32-bit arithmetic, g W = ((g / M) W) M + (g % M) W with W = 64 T steps per workgroup, and the tile walk
// carries (quotient, remainder) along: one r step moves 4 rows = 4 T steps.  M <= 2^16 keeps (g % M) W + W < 2^31.
template <class K>
struct RatePolicy {
    using T = typename K::T;
    const T *x;
    T *y;
    uint32_t M, Tc;
    bool sparse_in, sparse_out;
    uint32_t off_wg, dq, dm;
    uint64_t base;
    __device__ __forceinline__ RatePolicy(const IirRateIo<K> &a, uint32_t g, uint32_t Tchunk)
        : x(a.x), y(a.y), M(a.M), Tc(Tchunk), sparse_in(a.sparse_in != 0), sparse_out(a.sparse_out != 0) {
        const uint32_t W = (uint32_t)kIirWg * Tchunk, rs = (uint32_t)(kIirWg / kTs) * Tchunk;
        off_wg = (g % M) * W;
        base = (uint64_t)(g / M) * W;
        dq = rs / M;
        dm = rs % M;
    }
    // f(row, column, step holds a sample and lies inside the call, index of that sample)
    template <class F>
    __device__ __forceinline__ void walk(uint64_t wg0, uint64_t Tl, int t0, int lane, uint64_t n, F &&f) const {
        const int j0 = lane / kTs, tt = lane % kTs;
        const uint32_t off = off_wg + (uint32_t)j0 * Tc + (uint32_t)(t0 + tt);
        uint32_t q = off / M, rm = off % M;
#pragma unroll
        for (int r = 0; r < kTs; ++r) {
            const int j = j0 + r * (kIirWg / kTs);
            const uint64_t gi = wg0 + (uint64_t)j * Tl + (uint64_t)(t0 + tt);
            f(j, tt, rm == 0 && gi < n, base + q);
            q += dq;
            rm += dm;
            if (rm >= M) { rm -= M; ++q; }
        }
    }
    __device__ __forceinline__ void load(T (*tile)[kTs + 1], uint64_t wg0, uint64_t Tl, int t0, int lane, uint64_t n) const {
        if (!sparse_in) return PlainPolicy<K>{x, y}.load(tile, wg0, Tl, t0, lane, n);
        // a step without a sample feeds +0.0 through the full recurrence (the reference calls execute(0.0))
        walk(wg0, Tl, t0, lane, n, [&](int j, int tt, bool has, uint64_t i) { tile[j][tt] = has ? x[i] : izero<T>(); });
    }
    __device__ __forceinline__ void store(T (*tile)[kTs + 1], uint64_t wg0, uint64_t Tl, int t0, int lane, uint64_t n) const {
        if (!sparse_out) return PlainPolicy<K>{x, y}.store(tile, wg0, Tl, t0, lane, n);
        walk(wg0, Tl, t0, lane, n, [&](int j, int tt, bool has, uint64_t i) { if (has) y[i] = tile[j][tt]; });
    }
};

// IirHilbertFilter: the reference's two real filters are one crcf filter over the complex stream u (re -> filt_0,
// im -> filt_1).  With k = (phase + gi) & 3 the input map turns x into u and the output map turns the filter output v
// into y (iirhilb.rs:55-164); negations are sign-bit flips and the factor 2 is exact.  Every chunk and every tile row
// starts at a multiple of 4 steps, so k follows from the column alone.
struct HilbPolicy {
    using T = cf32;
    const void *x;
    void *y;
    uint32_t ph;
    int im, om;
    __device__ __forceinline__ HilbPolicy(const IirHilbIo &a, uint32_t, uint32_t) : x(a.x), y(a.y), ph(a.phase), im(a.imode), om(a.omode) {}
    __device__ __forceinline__ void load(cf32 (*tile)[kTs + 1], uint64_t wg0, uint64_t Tl, int t0, int lane, uint64_t n) const {
#pragma unroll
        for (int r = 0; r < kTs; ++r) {
            const int e = lane + r * kIirWg, j = e / kTs, tt = e % kTs;
            const uint64_t gi = wg0 + (uint64_t)j * Tl + (uint64_t)(t0 + tt);
            const uint32_t k = (ph + (uint32_t)(t0 + tt)) & 3u;
            cf32 u{0.0f, 0.0f};
            if (im == kHilbInReal) {                        // r2c, decim: (x,0), (0,-x), (-x,0), (0,x)
                const float v = (gi < n) ? static_cast<const float *>(x)[gi] : 0.0f;
                const float s = (k == 1 || k == 2) ? -v : v;
                u = (k & 1u) ? cf32{0.0f, s} : cf32{s, 0.0f};
            } else if (im == kHilbInCplx) {                 // c2r: x, (im,-re), -x, (-im,re)
                const cf32 v = (gi < n) ? static_cast<const cf32 *>(x)[gi] : cf32{0.0f, 0.0f};
                u = (k == 0) ? v : (k == 1) ? cf32{v.im, -v.re} : (k == 2) ? cf32{-v.re, -v.im} : cf32{-v.im, v.re};
            } else if (im == kHilbInEven) {                 // interp: x at the even steps, (0,0) at the odd ones
                if (!(tt & 1) && gi < n) u = static_cast<const cf32 *>(x)[gi >> 1];
            } else {
                if (gi < n) u = static_cast<const cf32 *>(x)[gi];
            }
            tile[j][tt] = u;
        }
    }
    __device__ __forceinline__ void store(cf32 (*tile)[kTs + 1], uint64_t wg0, uint64_t Tl, int t0, int lane, uint64_t n) const {
#pragma unroll
        for (int r = 0; r < kTs; ++r) {
            const int e = lane + r * kIirWg, j = e / kTs, tt = e % kTs;
            const uint64_t gi = wg0 + (uint64_t)j * Tl + (uint64_t)(t0 + tt);
            const uint32_t k = (ph + (uint32_t)(t0 + tt)) & 3u;
            if (gi >= n) continue;
            const cf32 v = tile[j][tt];
            if (om == kHilbOutRot2) {                       // r2c: 2 (re,im), 2 (-im,re), 2 (-re,-im), 2 (im,-re)
                const float a = 2.0f * v.re, b = 2.0f * v.im;
                static_cast<cf32 *>(y)[gi] = (k == 0) ? cf32{a, b} : (k == 1) ? cf32{-b, a} : (k == 2) ? cf32{-a, -b} : cf32{b, -a};
            } else if (om == kHilbOutProj || om == kHilbOutProj2) {     // c2r: re, -im, -re, im; interp: twice that
                const float w = (k & 1u) ? v.im : v.re;
                const float s = (k == 1 || k == 2) ? -w : w;
                static_cast<float *>(y)[gi] = (om == kHilbOutProj2) ? 2.0f * s : s;
            } else if (om == kHilbOutEven2) {               // decim: 2 v at the even steps
                if (!(tt & 1)) static_cast<cf32 *>(y)[gi >> 1] = cf32{2.0f * v.re, 2.0f * v.im};
            } else {
                static_cast<cf32 *>(y)[gi] = v;
            }
        }
    }
};

// ---- phases A and C ---------------------------------------------------------------------------------------------
// OUT = false: phase A (zero start, z and the workgroup aggregate); OUT = true: phase C (exact start, y and the state)
// n = filter steps of the call
template <class K, bool SOS, int SC, bool OUT, class IO>
__device__ __forceinline__ void
iir_scan_pass(const IirParams<K> &p, const IO &io, size_t n, typename K::T *__restrict__ z,
              typename IirF64<K>::V *__restrict__ agg, const typename IirF64<K>::V *__restrict__ init,
              typename K::T *__restrict__ state, const typename IirF64<K>::M *__restrict__ ptab) {
    using T = typename K::T;
    using V = typename IirF64<K>::V;
    using M = typename IirF64<K>::M;
    __shared__ T tile[kIirWg][kTs + 1];
    __shared__ M pl[SC * SC];
    __shared__ V vb[vbuf_len<SC, V>()];
    const int lane = (int)threadIdx.x;
    const int S = p.S;
    const uint64_t Tl = (uint64_t)p.T;
    const uint64_t g = blockIdx.x;
    const uint64_t nc = (n + Tl - 1) >> __builtin_ctz((unsigned)p.T);    // T is a power of two
    const uint64_t c = g * kIirWg + (uint64_t)lane;
    const bool valid = c < nc;
    const uint64_t c0 = c * Tl;
    const uint64_t len = valid ? ((n - c0 < Tl) ? n - c0 : Tl) : 0;

    T s[SC];
#pragma unroll
    for (int i = 0; i < SC; ++i) s[i] = izero<T>();
    if (OUT) {
        // the chunk's initial state: seed lane 0 with P_0 init[g] + z_0, scan, shift by one lane
        V v[SC], seed[SC], zero[SC];
#pragma unroll
        for (int i = 0; i < SC; ++i) {
            zero[i] = dzero((V *)nullptr);
            seed[i] = zero[i];
            if (i < S) seed[i] = init[g * S + i];
            v[i] = zero[i];
            if (valid && i < S) v[i] = to64(z[c * S + i], (V *)nullptr);
        }
        stage_mat(pl, ptab, S, lane);
        if (lane == 0) {
            V t[SC];
#pragma unroll
            for (int i = 0; i < SC; ++i) t[i] = seed[i];
            matvec_add<SC>(t, pl, S, v, vb, lane);
#pragma unroll
            for (int i = 0; i < SC; ++i) v[i] = t[i];
        }
        wave_scan<SC>(v, S, ptab, 0, lane, pl, vb);
#pragma unroll
        for (int i = 0; i < SC; ++i) {
            const V e = shup(v[i], 1);
            s[i] = from64(dpick(lane == 0, seed[i], e));
        }
    }
    int head = 0;
    if (!SOS) {
        // (head0 - c T) mod n in 32-bit arithmetic (g < 2^31, n <= 33)
        const uint32_t nn = (uint32_t)p.n;
        const uint32_t cm = (((uint32_t)blockIdx.x % nn) * ((uint32_t)kIirWg % nn) + (uint32_t)lane) % nn;
        const uint32_t c0m = (cm * ((uint32_t)p.T % nn)) % nn;
        head = (int)((p.head0 + nn - c0m) % nn);
    }

    const uint64_t wg0 = g * kIirWg * Tl;
#pragma unroll 1
    for (int t0 = 0; t0 < p.T; t0 += kTs) {
        __syncthreads();
        io.load(tile, wg0, Tl, t0, lane, n);
        __syncthreads();
#pragma unroll 1
        for (int tt = 0; tt < kTs; ++tt) {
            if ((uint64_t)(t0 + tt) < len) {
                const T xv = tile[lane][tt];
                const T yv = SOS ? sos_step<K, SC>(s, p.n, p, xv) : tf_step<K, SC>(s, p.n, head, p, xv);
                if (OUT) tile[lane][tt] = imul(yv, p.scale);
            }
        }
        if (OUT) {
            __syncthreads();
            io.store(tile, wg0, Tl, t0, lane, n);
        }
    }

    if (!OUT) {
        V v[SC];
#pragma unroll
        for (int i = 0; i < SC; ++i) {
            if (valid && i < S) z[c * S + i] = s[i];
            v[i] = dzero((V *)nullptr);
            if (valid && i < S) v[i] = to64(s[i], (V *)nullptr);
        }
        wave_scan<SC>(v, S, ptab, 0, lane, pl, vb);
        if (lane == kIirWg - 1) {
#pragma unroll
            for (int i = 0; i < SC; ++i)
                if (i < S) agg[g * S + i] = v[i];
        }
    } else if (valid && c == nc - 1) {
#pragma unroll
        for (int i = 0; i < SC; ++i)
            if (i < S) state[i] = s[i];
    }
}

template <class K, bool SOS, int SC, bool OUT>
__global__ void __launch_bounds__(kIirWg)
iir_chunk_kernel(const IirParams<K> p, const typename K::T *__restrict__ x, size_t n, typename K::T *__restrict__ y,
                 typename K::T *__restrict__ z, typename IirF64<K>::V *__restrict__ agg,
                 const typename IirF64<K>::V *__restrict__ init, typename K::T *__restrict__ state,
                 const typename IirF64<K>::M *__restrict__ ptab) {
    iir_scan_pass<K, SOS, SC, OUT>(p, PlainPolicy<K>{x, y}, n, z, agg, init, state, ptab);
}

// the mapped forms: A = IirRateIo<K> (IirDecim, IirInterp) or IirHilbIo (IirHilbertFilter)
template <class K, class A> struct PolicyOf;
template <class K> struct PolicyOf<K, IirRateIo<K>> { using type = RatePolicy<K>; };
template <> struct PolicyOf<CRCF, IirHilbIo> { using type = HilbPolicy; };

template <class K, bool SOS, int SC, bool OUT, class A>
__global__ void __launch_bounds__(kIirWg)
iirmap_kernel(const IirParams<K> p, const A a, size_t n, typename K::T *__restrict__ z,
              typename IirF64<K>::V *__restrict__ agg, const typename IirF64<K>::V *__restrict__ init,
              typename K::T *__restrict__ state, const typename IirF64<K>::M *__restrict__ ptab) {
    const typename PolicyOf<K, A>::type io(a, (uint32_t)blockIdx.x, (uint32_t)p.T);
    iir_scan_pass<K, SOS, SC, OUT>(p, io, n, z, agg, init, state, ptab);
}

// ---- phase B: one wave scans the G - 1 workgroup aggregates, lane l owning 2^lc consecutive ones ------------------
template <class K, int SC>
__global__ void __launch_bounds__(kIirWg)
iir_phase_b(const typename IirF64<K>::V *__restrict__ agg, uint64_t G, int S, int lc, const typename K::T *__restrict__ state,
            typename IirF64<K>::V *__restrict__ init, const typename IirF64<K>::M *__restrict__ ptab) {
    using V = typename IirF64<K>::V;
    using M = typename IirF64<K>::M;
    const int lane = (int)threadIdx.x;
    const uint64_t cnt = (uint64_t)1 << lc;
    const uint64_t lo = (uint64_t)lane * cnt;
    const uint64_t na = G - 1;                           // aggregates that feed a later workgroup
    const uint64_t hi = (lo + cnt < na) ? lo + cnt : na;
    __shared__ M pw[SC * SC], pl[SC * SC];
    __shared__ V vb[vbuf_len<SC, V>()];
    stage_mat(pw, ptab + (size_t)6 * S * S, S, lane);    // transfer over one workgroup: A^(64 T)
    V seed[SC], r[SC], a[SC];
#pragma unroll
    for (int i = 0; i < SC; ++i) {
        seed[i] = dzero((V *)nullptr);
        if (i < S) seed[i] = to64(state[i], (V *)nullptr);
        r[i] = dpick(lane == 0, seed[i], dzero((V *)nullptr));
    }
#pragma unroll 1
    for (uint64_t k = lo; k < hi; ++k) {
#pragma unroll
        for (int i = 0; i < SC; ++i) {
            a[i] = dzero((V *)nullptr);
            if (i < S) a[i] = agg[k * S + i];
        }
        matvec_add<SC>(r, pw, S, a, vb, lane);
    }
    wave_scan<SC>(r, S, ptab, 6 + lc, lane, pl, vb);
#pragma unroll
    for (int i = 0; i < SC; ++i) {
        const V e = shup(r[i], 1);
        r[i] = dpick(lane == 0, seed[i], e);
        if (lo < G && i < S) init[lo * S + i] = r[i];
    }
#pragma unroll 1
    for (uint64_t k = lo; k < hi; ++k) {
#pragma unroll
        for (int i = 0; i < SC; ++i) {
            a[i] = dzero((V *)nullptr);
            if (i < S) a[i] = agg[k * S + i];
        }
        matvec_add<SC>(r, pw, S, a, vb, lane);
#pragma unroll
        for (int i = 0; i < SC; ++i)
            if (i < S) init[(k + 1) * S + i] = r[i];
    }
}

// A = PlainArgs<K> launches the plain chunk kernels, any other argument block the mapped ones; phase B is the same
template <class K> struct PlainArgs { const typename K::T *x; typename K::T *y; };

template <class K, bool SOS, int SC, class A>
int run_iir(const IirParams<K> &p, const A &a, size_t n, typename K::T *state, typename K::T *z, void *agg, void *init,
            const void *ptab, int levels, hipStream_t st) {
    using V = typename IirF64<K>::V;
    using M = typename IirF64<K>::M;
    const uint64_t Tl = (uint64_t)p.T;
    const uint64_t nc = (n + Tl - 1) / Tl;
    const uint64_t G = (nc + kIirWg - 1) / kIirWg;
    int lc = 0;
    while (((uint64_t)kIirWg << lc) < G - 1) ++lc;      // 64 lanes x 2^lc aggregates cover G - 1
    if (12 + lc > levels || G > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "iirfilt: block of %zu samples too long", n);
    const M *P = static_cast<const M *>(ptab);
    V *ag = static_cast<V *>(agg), *in = static_cast<V *>(init);
    if constexpr (std::is_same<A, PlainArgs<K>>::value)
        iir_chunk_kernel<K, SOS, SC, false><<<(unsigned)G, kIirWg, 0, st>>>(p, a.x, n, a.y, z, ag, in, state, P);
    else
        iirmap_kernel<K, SOS, SC, false, A><<<(unsigned)G, kIirWg, 0, st>>>(p, a, n, z, ag, in, state, P);
    YG_LAUNCH_CHECK();
    iir_phase_b<K, SC><<<1, kIirWg, 0, st>>>(ag, G, p.S, lc, state, in, P);
    YG_LAUNCH_CHECK();
    if constexpr (std::is_same<A, PlainArgs<K>>::value)
        iir_chunk_kernel<K, SOS, SC, true><<<(unsigned)G, kIirWg, 0, st>>>(p, a.x, n, a.y, z, ag, in, state, P);
    else
        iirmap_kernel<K, SOS, SC, true, A><<<(unsigned)G, kIirWg, 0, st>>>(p, a, n, z, ag, in, state, P);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

// the state cap of the filter picks the instantiation; TF = false leaves the transfer-function forms out (Hilbert)
template <class K, bool TF, class A>
int dispatch_iir(const IirParams<K> &p, const A &a, size_t n, typename K::T *state, typename K::T *z, void *agg,
                 void *init, const void *ptab, int levels, hipStream_t st) {
    if (n == 0) return YAGI_OK;
    if (p.T < kTs || (p.T & (p.T - 1)) || p.n < 1) return fail(YAGI_ERR_INTERNAL, "iirfilt: bad launch shape");
    if (p.sos) {
        if (p.n > kIirSosGroup || p.S != 2 * p.n) return fail(YAGI_ERR_INTERNAL, "iirfilt: bad section count");
        if (p.n <= 4) return run_iir<K, true, 8>(p, a, n, state, z, agg, init, ptab, levels, st);
        if (p.n <= 8) return run_iir<K, true, 16>(p, a, n, state, z, agg, init, ptab, levels, st);
        return run_iir<K, true, 2 * kIirSosGroup>(p, a, n, state, z, agg, init, ptab, levels, st);
    }
    if constexpr (TF) {
        if (p.n > kIirTfMaxN || p.S != p.n - 1) return fail(YAGI_ERR_INTERNAL, "iirfilt: bad filter length");
        if (p.S <= 4) return run_iir<K, false, 4>(p, a, n, state, z, agg, init, ptab, levels, st);
        if (p.S <= 8) return run_iir<K, false, 8>(p, a, n, state, z, agg, init, ptab, levels, st);
        if (p.S <= 16) return run_iir<K, false, 16>(p, a, n, state, z, agg, init, ptab, levels, st);
        return run_iir<K, false, kIirTfMaxN - 1>(p, a, n, state, z, agg, init, ptab, levels, st);
    }
    return fail(YAGI_ERR_INTERNAL, "iirfilt: this form runs second-order sections only");
}

}  // namespace

template <class K>
int launch_iir(const IirParams<K> &p, const typename K::T *x, size_t n, typename K::T *y, typename K::T *state,
               typename K::T *z, void *agg, void *init, const void *ptab, int levels, hipStream_t st) {
    return dispatch_iir<K, true>(p, PlainArgs<K>{x, y}, n, state, z, agg, init, ptab, levels, st);
}

template <class K>
int launch_iir_rate(const IirParams<K> &p, const IirRateIo<K> &io, size_t n, typename K::T *state, typename K::T *z,
                    void *agg, void *init, const void *ptab, int levels, hipStream_t st) {
    if (io.M < 2 || io.M > kIirMaxRate) return fail(YAGI_ERR_INTERNAL, "iirmap: bad rate");
    return dispatch_iir<K, true>(p, io, n, state, z, agg, init, ptab, levels, st);
}

int launch_iir_hilb(const IirParams<CRCF> &p, const IirHilbIo &io, size_t n, cf32 *state, cf32 *z, void *agg, void *init,
                    const void *ptab, int levels, hipStream_t st) {
    if (p.T % 4) return fail(YAGI_ERR_INTERNAL, "iirmap: the chunk length must be a multiple of 4");
    return dispatch_iir<CRCF, false>(p, io, n, state, z, agg, init, ptab, levels, st);
}

template int launch_iir<RRRF>(const IirParams<RRRF> &, const float *, size_t, float *, float *, float *, void *, void *,
                              const void *, int, hipStream_t);
template int launch_iir<CRCF>(const IirParams<CRCF> &, const cf32 *, size_t, cf32 *, cf32 *, cf32 *, void *, void *,
                              const void *, int, hipStream_t);
template int launch_iir<CCCF>(const IirParams<CCCF> &, const cf32 *, size_t, cf32 *, cf32 *, cf32 *, void *, void *,
                              const void *, int, hipStream_t);
template int launch_iir_rate<RRRF>(const IirParams<RRRF> &, const IirRateIo<RRRF> &, size_t, float *, float *, void *,
                                   void *, const void *, int, hipStream_t);
template int launch_iir_rate<CRCF>(const IirParams<CRCF> &, const IirRateIo<CRCF> &, size_t, cf32 *, cf32 *, void *,
                                   void *, const void *, int, hipStream_t);
template int launch_iir_rate<CCCF>(const IirParams<CCCF> &, const IirRateIo<CCCF> &, size_t, cf32 *, cf32 *, void *,
                                   void *, const void *, int, hipStream_t);

}  // namespace yagi
