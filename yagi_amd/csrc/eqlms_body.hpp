// eqlms_body.hpp -- the per-sample arithmetic of EqLms (push, execute, step and the desired symbol, eqlms.rs:125-192),
// shared by eqlms_kernels.hip and symtrack_kernels.hip.  Both files are built with -ffp-contract=off (Makefile): every
// product, add and quotient keeps its own rounding.  ring and w point at the lane's column; stride is the lane count.
#pragma once
#include <cmath>

#include "kernels.hpp"

namespace yagi {
namespace {

#define EQ_HD __host__ __device__ __forceinline__

// `one` is an exact 1.0 the compiler cannot see: it keeps the quotient an f64 expression (a sum with 0.0 would lose -0)
EQ_HD float eq_quot(float a, float b, double one) { return (float)(((double)a * one) / (double)b); }

// (x * x.conj()).re(), num-complex's product
EQ_HD float eq_norm(cf32 x) { return x.re * x.re - x.im * (-x.im); }

// f(i, slot) for i = 0 .. h_len - 1, slot = the ring slot of the i-th oldest sample
template <class F>
EQ_HD void eq_window(unsigned head, unsigned h_len, F f) {
    unsigned i = 0;
#pragma unroll 4
    for (unsigned sl = head; sl < h_len; ++sl, ++i) f(i, sl);
#pragma unroll 4
    for (unsigned sl = 0; sl < head; ++sl, ++i) f(i, sl);
}

// push (:125-129) without the count: ring[head] is the sample that leaves
EQ_HD void eq_push(cf32 *ring, unsigned stride, unsigned &head, unsigned h_len, cf32 x, float &x2_sum) {
    const cf32 old = ring[head * stride];
    const float x2_n = eq_norm(x), x2_0 = eq_norm(old);
    x2_sum = x2_sum + (x2_n - x2_0);
    ring[head * stride] = x;
    head = head + 1 == h_len ? 0 : head + 1;
}

// execute (:137-140)
EQ_HD cf32 eq_execute(const cf32 *ring, const cf32 *w, unsigned stride, unsigned head, unsigned h_len) {
    float yr = 0.0f, yi = 0.0f;
    eq_window(head, h_len, [&](unsigned i, unsigned sl) {
        const cf32 wv = w[i * stride], r = ring[sl * stride];
        const float ar = wv.re, ai = -wv.im;
        const float tr = ar * r.re - ai * r.im, ti = ar * r.im + ai * r.re;
        yr = yr + tr;
        yi = yi + ti;
    });
    return cf32{yr, yi};
}

// step (:179-186) behind the buf_full gate
EQ_HD void eq_step(const cf32 *ring, cf32 *w, unsigned stride, unsigned head, unsigned h_len, float mu, float x2_sum,
                   cf32 d, cf32 y, double one) {
    const float ar = d.re - y.re, ai = d.im - y.im;
    const float sr = mu * ar, si = mu * (-ai);
    eq_window(head, h_len, [&](unsigned i, unsigned sl) {
        const cf32 r = ring[sl * stride];
        const float pr = sr * r.re - si * r.im, pi = sr * r.im + si * r.re;
        cf32 wv = w[i * stride];
        wv.re = wv.re + eq_quot(pr, x2_sum, one);
        wv.im = wv.im + eq_quot(pi, x2_sum, one);
        w[i * stride] = wv;
    });
}

// d_hat / |d_hat| with the library's |.|
EQ_HD cf32 eq_unit(cf32 y, double one) {
    const double re = (double)y.re, im = (double)y.im;
    const float a = (float)sqrt(re * re + im * im);
    return cf32{eq_quot(y.re, a, one), eq_quot(y.im, a, one)};
}

// the first table entry at the least unfused squared distance; only a strictly smaller value replaces the best
EQ_HD cf32 eq_decide(cf32 y, const cf32 *table, unsigned M) {
    float dmin = INFINITY;
    unsigned s = 0;
#pragma unroll 4
    for (unsigned j = 0; j < M; ++j) {
        const cf32 t = table[j];
        const float er = y.re - t.re, ei = y.im - t.im;
        const float dd = er * er + ei * ei;
        if (dd < dmin) {
            dmin = dd;
            s = j;
        }
    }
    return table[s];
}

EQ_HD cf32 eq_desired(int mode, cf32 y, cf32 dk, const cf32 *table, unsigned M, double one) {
    if (mode == YAGI_EQLMS_TRAIN) return dk;
    if (mode == YAGI_EQLMS_BLIND) return eq_unit(y, one);
    return eq_decide(y, table, M);
}

}  // namespace
}  // namespace yagi
