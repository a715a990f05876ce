// modem_body.hpp -- the hard-decision arithmetic of Modem's schemes whose decision and x_hat are plain f32 arithmetic
// (BPSK, QPSK, OOK, ASK, QAM and Arb's first-minimum search), shared by modem_kernels.hip and symtrack_kernels.hip.
// Both files are built with -ffp-contract=off (Makefile): every subtract, product and add is one f32 rounding.
// md_linear<m> is the form unrolled at compile time; md_linear_rt runs the same statements for a bps known at run time
// and forms the same words.  md_hard is one sample of demodulate for a scheme chosen at run time (wave-uniform).
#pragma once
#include <cmath>

#include "kernels.hpp"

#define MD_HD __host__ __device__ __forceinline__

namespace yagi {
namespace {

constexpr float kPi = 3.14159274101257324f;        // std::f32::consts::PI
constexpr float kTwoPi = 6.28318548202514648f;     // 2.0 * PI
constexpr float kSqrt2 = 1.41421353816986084f;     // SQRT_2
constexpr float kRsqrt2 = 0.707106769084930420f;   // FRAC_1_SQRT_2

MD_HD unsigned md_gray_encode(unsigned s) { return s ^ (s >> 1); }

// demodulate_linear_array_ref :296-315
template <int m>
MD_HD unsigned md_linear(const float *ref, float v, float &res) {
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < m; ++k) {
        s <<= 1;
        if (v > 0.0f) {
            s |= 1;
            v -= ref[m - k - 1];
        } else {
            v += ref[m - k - 1];
        }
    }
    res = v;
    return s;
}
MD_HD unsigned md_linear_rt(const float *ref, int m, float v, float &res) {
    unsigned s = 0;
    for (int k = 0; k < m; ++k) {
        s <<= 1;
        if (v > 0.0f) {
            s |= 1;
            v -= ref[m - k - 1];
        } else {
            v += ref[m - k - 1];
        }
    }
    res = v;
    return s;
}

// One table entry of Arb's search for one sample (arb.rs:21-35 hard on squared distances, :37-74 soft with the bit of
// the running best index).
template <int BPS, bool SOFT>
MD_HD void md_arb_step(cf32 x, cf32 c, unsigned idx, float &dmin, unsigned &s, float *d0, float *d1) {
    const float er = x.re - c.re, ei = x.im - c.im;
    const float d = er * er + ei * ei;
    if (d < dmin) {
        dmin = d;
        s = idx;
    }
    if constexpr (SOFT) {
#pragma unroll
        for (int k = 0; k < BPS; ++k) {
            // as selects on values: a select between the two ADDRESSES would send both arrays to scratch
            const bool one = ((s >> (BPS - k - 1)) & 1u) != 0;
            const float m0 = d < d0[k] ? d : d0[k], m1 = d < d1[k] ? d : d1[k];
            d0[k] = one ? d0[k] : m0;
            d1[k] = one ? m1 : d1[k];
        }
    }
}

// demodulate of ask.rs:51-63, qam.rs:95-116, bpsk.rs:15-33, qpsk.rs:16-38, ook.rs:16-25 and arb.rs:21-35 for a kind and
// bps chosen at run time: the symbol, and x_hat in xh.  ref = reference[], map = the M points.
MD_HD unsigned md_hard(int kind, int bps, const float *ref, const cf32 *map, cf32 x, cf32 &xh) {
    unsigned s = 0;
    if (kind == MODEM_ASK) {
        float res;
        s = md_gray_encode(md_linear_rt(ref, bps, x.re, res));
        xh = map[s];
    } else if (kind == MODEM_QAM) {
        const int mi = (bps + 1) >> 1, mq = bps >> 1;
        float ri, rq;
        const unsigned si = md_gray_encode(md_linear_rt(ref, mi, x.re, ri));
        const unsigned sq = md_gray_encode(md_linear_rt(ref, mq, x.im, rq));
        s = (si << mq) + sq;
        xh = cf32{x.re - ri, x.im - rq};
    } else if (kind == MODEM_BPSK) {
        s = x.re > 0.0f ? 0u : 1u;
        xh = cf32{s == 0 ? 1.0f : -1.0f, 0.0f};
    } else if (kind == MODEM_QPSK) {
        s = (x.re > 0.0f ? 0u : 1u) + (x.im > 0.0f ? 0u : 2u);
        xh = cf32{(s & 1u) == 0 ? kRsqrt2 : -kRsqrt2, (s & 2u) == 0 ? kRsqrt2 : -kRsqrt2};
    } else if (kind == MODEM_OOK) {
        s = x.re > kRsqrt2 ? 0u : 1u;
        xh = cf32{s != 0 ? 0.0f : kSqrt2, 0.0f};
    } else {                                                                 // MODEM_ARB
        float dmin = INFINITY;
        const unsigned M = 1u << bps;
        for (unsigned idx = 0; idx < M; ++idx) md_arb_step<1, false>(x, map[idx], idx, dmin, s, nullptr, nullptr);
        xh = map[s];
    }
    return s;
}

}  // namespace
}  // namespace yagi
