// eqrls_body.hpp -- the per-symbol arithmetic of EqRls (execute and step, eqrls.rs:106-146), shared by the device kernel
// and the host form of eqrls_kernels.hip.  That file is built with -ffp-contract=off (Makefile): every product, add and
// quotient keeps its own rounding.
//
// One channel's step is run by a group of L lanes (the host form is the group of one lane, t = 0, L = 1, stride 1).  Every
// sum of the recursion is formed whole by one lane, in the order of the sequential loop: lane t owns the columns and the
// rows t, t + L, t + 2 L ...  Lanes hand finished values to each other through the arrays of RlsView and `sync()`; there
// is no cross-lane reduction.  Element e of an array of the view is at [e * stride].
#pragma once
#include "bank_lane.hpp"
#include "eqlms_body.hpp"     // eq_quot, eq_window, eq_desired

namespace yagi {
namespace {

struct RlsView {
    cf32 *P0, *P1;            // the recursion matrix and the buffer its successor is written to, [p][pp] each
    Ring<cf32> ring;          // the window, [p], at the arrays' stride
    cf32 *w;                  // w0, [p]
    cf32 *xp0, *g, *row;      // [p], [p] and two rows of gxl, [2][p]
    unsigned stride, p, pp;   // pp: the row pitch of P0 and P1 in elements
};

// num-complex's product and quotient: n = b.re b.re + b.im b.im is passed in, it is the same for every quotient by one b
EQ_HD cf32 rls_mul(cf32 a, cf32 b) { return cf32{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
EQ_HD cf32 rls_conj(cf32 a) { return cf32{a.re, -a.im}; }
EQ_HD float rls_norm_sqr(cf32 b) { return b.re * b.re + b.im * b.im; }
EQ_HD cf32 rls_quot(cf32 a, cf32 b, float n, double one) {
    const float re = a.re * b.re + a.im * b.im, im = a.im * b.re - a.re * b.im;
    return cf32{eq_quot(re, n, one), eq_quot(im, n, one)};
}

// execute (:106-110): y = sum_i w0[i] r[i], no conjugate, folded from Complex(0, 0); every lane forms it
EQ_HD cf32 rls_execute(const RlsView v) {
    float yr = 0.0f, yi = 0.0f;
    eq_window(v.ring.head, v.p, [&](unsigned i, unsigned sl) {
        const cf32 t = rls_mul(v.w[i * v.stride], v.ring.col[sl * v.stride]);
        yr = yr + t.re;
        yi = yi + t.im;
    });
    return cf32{yr, yi};
}

// step(d, d_hat) (:112-146).  On entry every lane of the group has finished rls_execute; on return P1 is the new matrix
// (the caller lets the two buffers change places, rls_swap), w the new weights, and every lane may read them.
template <class Sync>
EQ_HD void rls_step(const RlsView v, unsigned t, unsigned L, float lambda, cf32 d, cf32 y, double one, Sync sync) {
    const unsigned p = v.p, pp = v.pp, S = v.stride;
    const cf32 alpha{d.re - y.re, d.im - y.im};
    // xp0[c] = sum_r x[r] P0[r][c] for the lane's columns; the numerators of g for its rows
    for (unsigned c = t; c < p; c += L) {
        float sr = 0.0f, si = 0.0f, gr = 0.0f, gi = 0.0f;
        for (unsigned r = 0; r < p; ++r) {
            const cf32 xr = v.ring(r);
            const cf32 a = rls_mul(xr, v.P0[(r * pp + c) * S]);
            sr = sr + a.re;
            si = si + a.im;
            const cf32 b = rls_mul(v.P0[(c * pp + r) * S], rls_conj(xr));      // row c, column r
            gr = gr + b.re;
            gi = gi + b.im;
        }
        v.xp0[c * S] = cf32{sr, si};
        v.g[c * S] = cf32{gr, gi};
    }
    sync();
    // zeta = (sum_c xp0[c] conj(x[c])) + Complex(lambda, 0): p terms, formed by every lane
    float zr = 0.0f, zi = 0.0f;
    for (unsigned c = 0; c < p; ++c) {
        const cf32 a = rls_mul(v.xp0[c * S], rls_conj(v.ring(c)));
        zr = zr + a.re;
        zi = zi + a.im;
    }
    const cf32 zeta{zr + lambda, zi + 0.0f};
    const float zn = rls_norm_sqr(zeta);
    // g[r] = numerator / zeta and w1[r] = w0[r] + alpha g[r] for the lane's rows
    for (unsigned r = t; r < p; r += L) {
        const cf32 gr = rls_quot(v.g[r * S], zeta, zn, one);
        v.g[r * S] = gr;
        const cf32 a = rls_mul(alpha, gr), w = v.w[r * S];
        v.w[r * S] = cf32{w.re + a.re, w.im + a.im};
    }
    sync();
    // Row r of gxl = (g[r] x[i]) / Complex(lambda, 0) is formed once, its elements spread over the lanes, into one of two
    // row buffers; then P1[r][c] = P0[r][c] / Complex(lambda, 0) - sum_i gxl[r][i] P0[i][c] for the lane's columns.  A
    // buffer is written again two rows later, behind the sync of the row between.
    const cf32 lam{lambda, 0.0f};
    const float ln = rls_norm_sqr(lam);
    for (unsigned r = 0; r < p; ++r) {
        cf32 *row = v.row + (r & 1u) * p * S;
        const cf32 gr = v.g[r * S];
        for (unsigned i = t; i < p; i += L) row[i * S] = rls_quot(rls_mul(gr, v.ring(i)), lam, ln, one);
        sync();
        for (unsigned c = t; c < p; c += L) {
            float sr = 0.0f, si = 0.0f;
#pragma unroll 4
            for (unsigned i = 0; i < p; ++i) {
                const cf32 a = rls_mul(row[i * S], v.P0[(i * pp + c) * S]);
                sr = sr + a.re;
                si = si + a.im;
            }
            const cf32 q = rls_quot(v.P0[(r * pp + c) * S], lam, ln, one);
            v.P1[(r * pp + c) * S] = cf32{q.re - sr, q.im - si};
        }
    }
    sync();
}

// after a step the two buffers change places
EQ_HD void rls_swap(RlsView &v) {
    cf32 *const old = v.P0;
    v.P0 = v.P1;
    v.P1 = old;
}

}  // namespace
}  // namespace yagi
