// channel_words.hpp -- the words of Channel's noise and of set_awgn (yagi_hip.h, the Channel block).  Like agc_words.hpp:
// f32 roundings of f64 evaluations made of IEEE f64 + - * / (and one f64 root), each rounded on its own, integer
// operations and literals.  No libm, no ocml, no hardware approximation for cos and sin: the same source gives the same
// word on the host and on the device.  The including file must be built with contraction off; the operation sequence
// below is the definition and tests/channel_ref.py restates it.
#pragma once
#include <cmath>
#include <cstdint>

#include "agc_words.hpp"    // yg_ln64, yg_exp64, kAgcLn10
#include "splitmix.hpp"     // splitmix64_at

namespace yagi {

constexpr double kChanStep = 0x1.921fb54442d18p-22;     // fl64(2 pi) 2^-24: the angle of one count of k2
// E: |f64 evaluation - true| of chan_cos_sin64 for every k2.  The argument m kChanStep is off by at most 2^-52 (the
// literal's rounding and the product's, m kChanStep <= pi / 4 (1 + 2^-52)), the series are cut after x^15 / 15! and
// x^16 / 16! (below 2^-54 at pi / 4) and the Horner chains round to a few units of 2^-53 of values below 1: under
// 2^-50 in all.  The constant leaves room.
constexpr double kChanCosSinE = 0x1p-45;

// (cos, sin)(2 pi k2 / 2^24), k2 in [0, 2^24), in f64.  The octant is the top three bits of k2; inside an odd octant the
// count is reflected on the integer (m = 2^21 - r), so the argument is in [0, pi / 4] and is exact up to one product.
// k2 = 0, 2^22, 2^23, 3 2^22 give exactly (1, 0), (0, 1), (-1, 0), (0, -1): m = 0 makes the sine +0 and the cosine 1, and a
// sign is changed as 0 - v, which keeps +0.
YG_WORD_HD void chan_cos_sin64(uint32_t k2, double *c, double *s) {
    const uint32_t oct = k2 >> 21, r = k2 & 0x1fffffu;
    const bool odd = (oct & 1u) != 0;
    const uint32_t m = odd ? 0x200000u - r : r;
    const double x = (double)m * kChanStep;
    const double z = x * x;
    double p = -1.0 / 1307674368000.0;                      // -1 / 15!
    p = p * z + 1.0 / 6227020800.0;                         //  1 / 13!
    p = p * z + -1.0 / 39916800.0;                          // -1 / 11!
    p = p * z + 1.0 / 362880.0;                             //  1 / 9!
    p = p * z + -1.0 / 5040.0;                              // -1 / 7!
    p = p * z + 1.0 / 120.0;                                //  1 / 5!
    p = p * z + -1.0 / 6.0;                                 // -1 / 3!
    const double sn = x + (x * z) * p;
    double q = 1.0 / 20922789888000.0;                      //  1 / 16!
    q = q * z + -1.0 / 87178291200.0;                       // -1 / 14!
    q = q * z + 1.0 / 479001600.0;                          //  1 / 12!
    q = q * z + -1.0 / 3628800.0;                           // -1 / 10!
    q = q * z + 1.0 / 40320.0;                              //  1 / 8!
    q = q * z + -1.0 / 720.0;                               // -1 / 6!
    q = q * z + 1.0 / 24.0;                                 //  1 / 4!
    q = q * z + -0.5;                                       // -1 / 2!
    const double cs = 1.0 + z * q;
    const double ss = odd ? 0.0 - sn : sn;                  // the angle is quad pi / 2 +- mu
    const uint32_t quad = ((oct + 1u) >> 1) & 3u;
    if (quad == 0u) {
        *c = cs;
        *s = ss;
    } else if (quad == 1u) {
        *c = 0.0 - ss;
        *s = cs;
    } else if (quad == 2u) {
        *c = 0.0 - cs;
        *s = 0.0 - ss;
    } else {
        *c = ss;
        *s = 0.0 - cs;
    }
}

// R = (float)sqrt(-ln(k1 2^-24)), k1 in [1, 2^24]: an f64 root of an f64 logarithm.  k1 = 2^24 gives -0, which is kept.
YG_WORD_HD float chan_radius(uint32_t k1) {
    return (float)sqrt(-yg_ln64((double)k1 * 0x1p-24));
}

// the noise sample of sequence seed_c at counter t: (R C, R S), E|.|^2 = 1
YG_WORD_HD void chan_noise(uint64_t seed_c, uint64_t t, float *nr, float *ni) {
    const uint64_t a = splitmix64_at(seed_c, 2 * t), b = splitmix64_at(seed_c, 2 * t + 1);
    const uint32_t k1 = (uint32_t)(a >> 40) + 1u, k2 = (uint32_t)(b >> 40);
    const float R = chan_radius(k1);
    double c, s;
    chan_cos_sin64(k2, &c, &s);
    const float C = (float)c, S = (float)s;
    *nr = R * C;
    *ni = R * S;
}

// set_awgn's 10^t: (float)exp64((double)t ln 10), the word of Agc::set_rssi; a NaN stays
YG_WORD_HD float chan_p10(float t) {
    if (t != t) return t;
    return (float)yg_exp64((double)t * kAgcLn10);
}

}  // namespace yagi
