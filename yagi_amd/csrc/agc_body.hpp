// agc_body.hpp -- the per-sample arithmetic of Agc (execute and squelch_update_mode, agc.rs:71-89 and :212-248) and a
// channel's record in registers, shared by agc_kernels.hip and symtrack_kernels.hip.  Both files are built with
// -ffp-contract=off (Makefile); ln, exp and log10 are the library's own words (agc_words.hpp).
#pragma once
#include "agc_words.hpp"
#include "kernels.hpp"

namespace yagi {
namespace {

#define AGC_HD __host__ __device__ __forceinline__

AGC_HD float agc_scaled(float x, float s) { return x * s; }
AGC_HD cf32 agc_scaled(cf32 x, float s) { return cf32{x.re * s, x.im * s}; }
// (y * y.conj()).re(): num-complex's product for Complex32, y y for f32
AGC_HD float agc_norm(float y) { return y * y; }
AGC_HD float agc_norm(cf32 y) { return y.re * y.re - y.im * (-y.im); }

// a channel's record in registers: plain words, so that nothing of it is ever addressed
struct AgcRegs {
    float g, y2p;
    unsigned timer, mode, locked;
};
AGC_HD AgcRegs agc_unpack(const AgcChan &c) { return AgcRegs{c.g, c.y2p, c.timer, c.mode, c.locked}; }
AGC_HD AgcChan agc_pack(const AgcRegs &s) {
    AgcChan c{};
    c.g = s.g, c.y2p = s.y2p, c.timer = s.timer, c.mode = (uint8_t)s.mode, c.locked = (uint8_t)s.locked;
    return c;
}

// squelch_update_mode (:212-248)
AGC_HD void agc_squelch(AgcRegs &s, float threshold, unsigned timeout) {
    const bool hi = -20.0f * yg_log10f(s.g) > threshold;
    unsigned m = s.mode;
    switch (m) {
    case YAGI_AGC_SQUELCH_ENABLED: m = hi ? YAGI_AGC_SQUELCH_RISE : YAGI_AGC_SQUELCH_ENABLED; break;
    case YAGI_AGC_SQUELCH_RISE: m = hi ? YAGI_AGC_SQUELCH_SIGNALHI : YAGI_AGC_SQUELCH_FALL; break;
    case YAGI_AGC_SQUELCH_SIGNALHI: m = hi ? YAGI_AGC_SQUELCH_SIGNALHI : YAGI_AGC_SQUELCH_FALL; break;
    case YAGI_AGC_SQUELCH_FALL:
        s.timer = timeout;
        m = hi ? YAGI_AGC_SQUELCH_SIGNALHI : YAGI_AGC_SQUELCH_SIGNALLO;
        break;
    case YAGI_AGC_SQUELCH_SIGNALLO:
        s.timer = s.timer - 1u;
        m = s.timer == 0u ? YAGI_AGC_SQUELCH_TIMEOUT : hi ? YAGI_AGC_SQUELCH_SIGNALHI : YAGI_AGC_SQUELCH_SIGNALLO;
        break;
    case YAGI_AGC_SQUELCH_TIMEOUT: m = YAGI_AGC_SQUELCH_ENABLED; break;
    default: break;
    }
    s.mode = m;
}

// execute (:71-89)
template <bool SQUELCH, class T>
AGC_HD T agc_step(AgcRegs &s, T x, float alpha, float scale, float threshold, unsigned timeout) {
    const T y = agc_scaled(x, s.g);
    const float y2 = agc_norm(y);
    s.y2p = (1.0f - alpha) * s.y2p + alpha * y2;
    if (s.locked) return y;
    if (s.y2p > 1e-6f) s.g = s.g * yg_expf(-0.5f * alpha * yg_lnf(s.y2p));
    s.g = s.g < 1e6f ? s.g : 1e6f;                          // f32::min: a NaN becomes 1e6
    if (SQUELCH) agc_squelch(s, threshold, timeout);
    return agc_scaled(y, scale);
}

}  // namespace
}  // namespace yagi
