// agc_words.hpp -- the library's own ln, exp and log10 in f32 (yagi_hip.h, the Agc block): each is the f32 rounding of
// an f64 evaluation that uses nothing but IEEE f64 + - * /, each rounded on its own, integer and bit operations on the
// exponent, and f64 literals.  No libm, no ocml, no hardware approximation: the same source gives the same word on the
// host and on the device.  The including file must be built with contraction off; the operation sequence below is the
// definition and tests/agc_ref.py restates it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define YG_WORD_HD __host__ __device__ __forceinline__
#else
#define YG_WORD_HD inline
#endif

namespace yagi {

constexpr double kAgcLn2 = 0x1.62e42fefa39efp-1;        // fl64(ln 2)
constexpr double kAgcInvLn2 = 0x1.71547652b82fep+0;     // fl64(1 / ln 2)
constexpr double kAgcLn2Hi = 0x1.62e42feep-1;           // ln 2 = Hi + Lo, Hi of 32 bits: k Hi is exact
constexpr double kAgcLn2Lo = 0x1.a39ef35793c76p-33;
constexpr double kAgcLn10 = 0x1.26bb1bbb55516p+1;       // fl64(ln 10)
constexpr double kAgcInvLn10 = 0x1.bcb7b1526e50ep-2;    // fl64(1 / ln 10)
constexpr double kAgcSqrt2 = 0x1.6a09e667f3bcdp+0;      // fl64(sqrt 2)

YG_WORD_HD uint64_t agc_bits(double x) {
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    return u;
}
YG_WORD_HD double agc_from_bits(uint64_t u) {
    double x;
    __builtin_memcpy(&x, &u, 8);
    return x;
}

// ln x for a positive, finite, normal f64 (every positive finite f32 is one)
YG_WORD_HD double yg_ln64(double x) {
    const uint64_t u = agc_bits(x);
    int e = (int)((u >> 52) & 0x7ffu) - 1023;
    double m = agc_from_bits((u & 0x000fffffffffffffull) | 0x3ff0000000000000ull);     // [1, 2)
    if (m >= kAgcSqrt2) {                                                               // -> [sqrt 1/2, sqrt 2)
        m = m * 0.5;
        e = e + 1;
    }
    const double s = (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double p = 1.0 / 23.0;
    p = p * z + 1.0 / 21.0;
    p = p * z + 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    p = p * z + 1.0;
    return (double)e * kAgcLn2 + (2.0 * s) * p;
}

// exp x for a non-NaN f64, x clamped to [-110, 95] first: 2^k stays a normal f64, and the f32 rounding of the result is
// 0 below and inf above the clamp anyway
YG_WORD_HD double yg_exp64(double x) {
    x = x < -110.0 ? -110.0 : x;
    x = x > 95.0 ? 95.0 : x;
    const double t = x * kAgcInvLn2 + 0.5;
    int k = (int)t;                                         // toward zero, then down to the floor
    k = (double)k > t ? k - 1 : k;
    const double kd = (double)k;
    const double r = (x - kd * kAgcLn2Hi) - kd * kAgcLn2Lo;
    double p = 1.0 / 87178291200.0;                         // 1 / 14!
    p = p * r + 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return p * agc_from_bits((uint64_t)(k + 1023) << 52);
}

YG_WORD_HD float agc_nanf() {
    const uint32_t u = 0x7fc00000u;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
YG_WORD_HD float agc_inff() {
    const uint32_t u = 0x7f800000u;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// true: x is a special argument of ln and *special is the word
YG_WORD_HD bool agc_ln_special(float x, float *special) {
    if (x != x || x < 0.0f) {
        *special = agc_nanf();
        return true;
    }
    if (x == 0.0f) {                                        // either zero
        *special = -agc_inff();
        return true;
    }
    if (x == agc_inff()) {
        *special = x;
        return true;
    }
    return false;
}

YG_WORD_HD float yg_lnf(float x) {
    float sp;
    if (agc_ln_special(x, &sp)) return sp;
    return (float)yg_ln64((double)x);
}

YG_WORD_HD float yg_log10f(float x) {
    float sp;
    if (agc_ln_special(x, &sp)) return sp;
    return (float)(yg_ln64((double)x) * kAgcInvLn10);
}

YG_WORD_HD float yg_expf(float x) {
    if (x != x) return x;
    return (float)yg_exp64((double)x);
}

// set_rssi's 10^(-rssi / 20): t = -rssi / 20 in f32, then (float)exp64((double)t ln 10)
YG_WORD_HD float yg_exp10_rssi(float rssi) {
    const float t = -rssi / 20.0f;
    if (t != t) return t;
    return (float)yg_exp64((double)t * kAgcLn10);
}

}  // namespace yagi
