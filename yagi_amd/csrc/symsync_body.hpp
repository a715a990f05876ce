// symsync_body.hpp -- SymSync's input row (step, symsync.rs:230-266: ss_row) and its per-output arithmetic (one iteration
// of step's while loop, :230-276: ss_output), shared by the kernels and the host forms of symsync_kernels.hip and
// symtrack_kernels.hip.  Both files are built with -ffp-contract=off (Makefile): every
// product and add of the sums and of the loop filter keeps its own rounding.
#pragma once
#include <cmath>

#include "bank_lane.hpp"
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

// One input row x of a channel: push, then every output that falls into this row, then the advance of tau, bf and b.
//   stall       the channel's stall code, 0 while it runs; a stalled channel's row does nothing but push (its column is dead)
//   room        outputs that still fit at the row's start: the loop is counted, 2 room + 1, so it ends whatever the state holds
//   any(m)      whether the select of ss_output<true> is needed: the host forms pass m through, a wave asks all of its lanes
//   full()      the capacity rule: an iteration about to store an output that does not fit does not run (stall = cap_code)
//   emit(y)     takes the output and returns 0, or the stall code that ends the channel's call behind this output
//   on_stall()  runs at the moment the channel stalls: the kernels write the window out, it is as the history has to keep it
template <class Stall, class Count, class Any, class Full, class Emit, class OnStall>
__host__ __device__ __forceinline__ void ss_row(SymsyncChan &s, const SymsyncLoop &p, Ring<cf32> &win, const SsTap *taps,
                                                cf32 x, Stall &stall, Stall cap_code, Count room, double zero, Any any,
                                                Full full, Emit emit, OnStall on_stall) {
    win.push(x);                                            // mf.push(x); dmf.push(x)
    if (!stall && s.since < p.Ls) s.since += 1;
    const unsigned z = p.Ls - s.since;
    const bool young = any(!stall && z != 0);
    Count budget = 2 * room + 1;
    while (!stall && s.b < p.npfb) {
        if (budget == 0 || full()) {                        // budget == 0 cannot happen
            stall = cap_code;
            on_stall();
            break;
        }
        --budget;
        const SsTap *row = taps + (size_t)s.b * p.Ls;
        auto tap = [&](unsigned j) { return row[j]; };
        const cf32 y = young ? ss_output<true>(s, p, z, win, tap, zero) : ss_output<false>(s, p, z, win, tap, zero);
        const Stall code = emit(y);
        if (code) {
            stall = code;
            on_stall();
            break;
        }
    }
    if (!stall) {
        s.tau = s.tau - 1.0f;
        s.bf = s.bf - p.npfbf;
        s.b -= p.npfb;
    }
}

}  // namespace
}  // namespace yagi
