// channel_body.hpp -- the per-sample arithmetic of Channel (yagi_hip.h, "Channel: the definition"), shared by the kernel
// and the host form of channel_kernels.hip.  The including file is built with -ffp-contract=off: every product and add
// below keeps its own rounding.
#pragma once
#include "channel_words.hpp"
#include "kernels.hpp"
#include "osc_mix.hpp"

namespace yagi {

// v = sum_{j < L} hrev[j] win[j], oldest sample first, sequential from 0, num-complex's product.  h and w are strided so
// that the kernel's [row][link] tiles and the host's plain arrays share the loop.
__host__ __device__ __forceinline__ float2 channel_fir(const cf32 *h, size_t h_stride, const cf32 *w, size_t w_stride,
                                                       unsigned L) {
    float ar = 0.0f, ai = 0.0f;
    for (unsigned j = 0; j < L; ++j) {
        const cf32 hv = h[(size_t)j * h_stride], xv = w[(size_t)j * w_stride];
        const float rr = hv.re * xv.re, ii = hv.im * xv.im, ri = hv.re * xv.im, ir = hv.im * xv.re;
        const float pr = rr - ii, pi = ri + ir;
        ar = ar + pr;
        ai = ai + pi;
    }
    return make_float2(ar, ai);
}

// carrier offset, gain and noise of the sample `at` samples after the words of k were taken.  Where nstd is zero and
// both scaled parts are nonzero, adding the noise term (a signed zero) changes no bit, so the draw is skipped.
template <int VCO>
__host__ __device__ __forceinline__ cf32 channel_finish(const typename OscEntry<VCO>::E *tab, const ChannelLink &k,
                                                        uint64_t seed_c, uint64_t at, float2 v) {
    const uint32_t theta = k.theta + (uint32_t)at * k.d_theta;
    const float2 w = osc_one<VCO, false>(tab, theta, v.x, v.y);
    const float gr = w.x * k.gamma, gi = w.y * k.gamma;
    if (k.nstd == 0.0f && gr != 0.0f && gi != 0.0f) return cf32{gr, gi};
    float nr, ni;
    chan_noise(seed_c, k.t + at, &nr, &ni);
    const float sr = k.nstd * nr, si = k.nstd * ni;
    return cf32{gr + sr, gi + si};
}

}  // namespace yagi
