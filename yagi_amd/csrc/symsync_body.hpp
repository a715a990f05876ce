// symsync_body.hpp -- the per-output arithmetic of SymSync (one iteration of step's while loop, symsync.rs:230-276),
// shared by symsync_kernels.hip and symtrack_kernels.hip.  Both files are built with -ffp-contract=off (Makefile): every
// product and add of the sums and of the loop filter keeps its own rounding.
#pragma once
#include <cmath>

#include "kernels.hpp"

namespace yagi {
namespace {

struct SsTap { float h, d; };

__host__ __device__ __forceinline__ float ss_quot(float a, float b, double zero) {
    return (float)(((double)a + zero) / (double)b);
}

// `bf.round() as usize`: half away from zero, saturating, negative and NaN give 0
__host__ __device__ __forceinline__ unsigned long long ss_round_usize(float bf) {
    const float t = truncf(bf);
    const float r = t + copysignf(fabsf(bf - t) >= 0.5f ? 1.0f : 0.0f, bf);
    if (!(r > 0.0f)) return 0ull;
    if (r >= 18446744073709551616.0f) return ~0ull;
    // r is an integer in [1, 2^64): shift its significand (the compiler's own f32 -> u64 conversion uses an f32 FMA)
    const unsigned w = __builtin_bit_cast(unsigned, r);
    const int e = (int)(w >> 23) - 127;
    const unsigned long long sig = (w & 0x7fffffu) | 0x800000u;
    return e >= 23 ? sig << (e - 23) : sig >> (23 - e);
}

// One iteration of step's while loop for a lane with b < npfb and room for the output: returns the word stored at y[ny].
// win(j) = the j-th oldest sample of the window, tap(j) = entry j of row b; z = slots the matched filter reads as +0.0.
template <bool Z, class Win, class Tap>
__host__ __device__ __forceinline__ cf32 ss_output(SymsyncChan &s, const SymsyncLoop &p, unsigned z, Win win, Tap tap,
                                                   double zero) {
    const bool upd = s.decim == p.k_out;
    float mr = 0.0f, mi = 0.0f, dr = 0.0f, di = 0.0f;
    if (upd && !p.locked) {
#pragma unroll 8
        for (unsigned j = 0; j < p.Ls; ++j) {
            const SsTap t = tap(j);
            const cf32 w = win(j);
            const cf32 wm = (Z && j < z) ? cf32{0.0f, 0.0f} : w;
            mr = mr + t.h * wm.re;
            mi = mi + t.h * wm.im;
            dr = dr + t.d * w.re;
            di = di + t.d * w.im;
        }
    } else {
#pragma unroll 8
        for (unsigned j = 0; j < p.Ls; ++j) {
            const SsTap t = tap(j);
            const cf32 w = win(j);
            const cf32 wm = (Z && j < z) ? cf32{0.0f, 0.0f} : w;
            mr = mr + t.h * wm.re;
            mi = mi + t.h * wm.im;
        }
    }
    // mf / Complex(k, 0), num-complex's division: (re k + im 0) / (k k + 0 0), (im k - re 0) / (k k + 0 0)
    cf32 y;
    y.re = ss_quot(mr * p.kf + mi * 0.0f, p.knorm, zero);
    y.im = ss_quot(mi * p.kf - mr * 0.0f, p.knorm, zero);
    if (upd) {
        s.decim = 0;
        if (!p.locked) {                                    // advance_internal_loop (:268-276)
            float q = mr * dr - (-mi) * di;                 // (mf.conj() * dmf).re()
            q = q < -1.0f ? -1.0f : (q > 1.0f ? 1.0f : q);   // clamp passes NaN
            s.q = q;
            s.v2 = s.v1;                                    // execute_df2
            s.v1 = s.v0;
            s.v0 = q - p.a1 * s.v1 - p.a2 * s.v2;
            s.q_hat = p.b0 * s.v0 + p.b1 * s.v1 + p.b2 * s.v2;
            s.rate = s.rate + p.rate_adj * s.q_hat;
            s.del = s.rate + s.q_hat;
            s.tau_decim = s.tau;
        }
        // a locked object repeats the iteration with decim_counter = 0: the same sum, the same word, then the lines below
    }
    s.decim += 1;
    s.tau = s.tau + s.del;
    s.bf = s.tau * p.npfbf;
    s.b = ss_round_usize(s.bf);
    return y;
}

}  // namespace
}  // namespace yagi
