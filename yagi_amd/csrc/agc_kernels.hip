// agc_kernels.hip -- Agc: automatic gain control (src/agc/agc.rs) for a bank of independent channels.
//
// The object is a control loop along time: the gain of sample i + 1 depends on output i through g -> y -> y2' -> ln ->
// exp -> g, so a channel has no block form.  Across channels nothing is shared but the settings, and a channelizer's
// output is laid out [step][channel]: one lane runs one channel's sequential loop word for word (agc_step below, the
// definition of yagi_hip.h), and a wave's load of a row is one contiguous request.
//
// agc_kernel<T, SQUELCH, STATUS>: a workgroup is one wave of 64 channels and loops over all n rows of the call.  The
// state (g, y2', the squelch mode and timer, the locked bit) is one 16-byte AgcChan per channel, read once and written
// back once per call, and lives in registers in between.  Rows are requested a chunk of kAgcAhead ahead into registers,
// so a step never waits for a memory round trip; the chunk loop is unrolled, the registers are indexed statically: no
// LDS, no scratch (tests/test_agc_isa_cpu.py).  SQUELCH is object-uniform: without it log10 and the state machine are
// not compiled in and the mode stays Disabled.  With STATUS the lane writes the mode after each sample as one byte.
// ln, exp and log10 are the library's own words (agc_words.hpp): f64 + - * / only, one f64 division in ln.
// In place (y == x at the same pitch) is safe: a lane reads its sample of a row before it writes it, and touches no
// other lane's.  A bank of few channels uses few lanes of its one wave.  Accepted.
//
// The launch is bank_launch (bank_lane.hpp); the kernel keeps its own prefetch: on RowQueue the instances that write
// the status plane without squelch ran 4.5 % longer (profiles/r29_kbench_bank_lanes.txt).
// The host form lives here too, with the array forms of the words: host.cpp and capi.hip are built with contraction on.
#pragma clang fp contract(off)

#include <cmath>

#include "agc_body.hpp"       // agc_step and its helpers: shared with symtrack_kernels.hip
#include "agc_words.hpp"
#include "bank_lane.hpp"
#include "devmath.hpp"
#include "kernels.hpp"

namespace yagi {
namespace {

template <class T>
struct AgcArgs {
    AgcChan *state;
    const T *x;
    T *y;
    uint8_t *status;
    size_t C, x_pitch, y_pitch, status_pitch;
    unsigned n, timeout;
    float alpha, scale, threshold;
};

template <class T, bool SQUELCH, bool STATUS>
__global__ __launch_bounds__(kAgcWg) void agc_kernel(const AgcArgs<T> a) {
    const size_t c = (size_t)blockIdx.x * kAgcWg + threadIdx.x;
    if (c >= a.C) return;                                   // a lane beyond the last channel does nothing
    AgcRegs s = agc_unpack(a.state[c]);
    const T *xp = a.x + c;
    T *yp = a.y + c;
    uint8_t *sp = STATUS ? a.status + c : nullptr;
    const unsigned n = a.n;

    T xq[kAgcAhead];
#pragma unroll
    for (int u = 0; u < kAgcAhead; ++u) xq[u] = (unsigned)u < n ? ld_stream(xp + (size_t)u * a.x_pitch) : T{};

    for (unsigned s0 = 0; s0 < n; s0 += kAgcAhead) {
        T cur[kAgcAhead];
#pragma unroll
        for (int u = 0; u < kAgcAhead; ++u) cur[u] = xq[u];
#pragma unroll
        for (int u = 0; u < kAgcAhead; ++u) {
            const size_t ahead = (size_t)s0 + kAgcAhead + u;
            xq[u] = ahead < n ? ld_stream(xp + ahead * a.x_pitch) : T{};
        }
#pragma unroll
        for (int u = 0; u < kAgcAhead; ++u) {
            const size_t row = (size_t)s0 + u;
            if (row < n) {
                const T y = agc_step<SQUELCH>(s, cur[u], a.alpha, a.scale, a.threshold, a.timeout);
                st_stream(yp + row * a.y_pitch, y);
                if (STATUS) __builtin_nontemporal_store((uint8_t)s.mode, sp + row * a.status_pitch);
            }
        }
    }
    a.state[c] = agc_pack(s);
}

// init (:171-178): the f32 sum of |x|^2 in row order; the root and the quotient are the host's
template <class T>
__global__ __launch_bounds__(kAgcWg) void agc_init_kernel(const T *x, size_t x_pitch, unsigned n, size_t C, float *sum) {
    const size_t c = (size_t)blockIdx.x * kAgcWg + threadIdx.x;
    if (c >= C) return;
    float acc = 0.0f;
    for (unsigned i = 0; i < n; ++i) acc = acc + agc_norm(x[(size_t)i * x_pitch + c]);
    sum[c] = acc;
}

template <class T, bool SQUELCH, bool STATUS>
int agc_launch(const AgcArgs<T> &a, hipStream_t st) {
    return bank_launch(agc_kernel<T, SQUELCH, STATUS>, a.C, kAgcWg, kAgcWg, 0, st, a);
}

}  // namespace

template <class T>
int launch_agc(const AgcSettings &g, AgcChan *state, size_t C, const T *x, size_t x_pitch, size_t n, T *y, size_t y_pitch,
               uint8_t *status, size_t status_pitch, hipStream_t st) {
    AgcArgs<T> a{};
    a.state = state, a.x = x, a.y = y, a.status = status;
    a.C = C, a.x_pitch = x_pitch, a.y_pitch = y_pitch, a.status_pitch = status_pitch;
    a.n = (unsigned)n, a.timeout = g.timeout;
    a.alpha = g.alpha, a.scale = g.scale, a.threshold = g.threshold;
    if (g.squelch) return status ? agc_launch<T, true, true>(a, st) : agc_launch<T, true, false>(a, st);
    return status ? agc_launch<T, false, true>(a, st) : agc_launch<T, false, false>(a, st);
}
template int launch_agc<cf32>(const AgcSettings &, AgcChan *, size_t, const cf32 *, size_t, size_t, cf32 *, size_t, uint8_t *,
                              size_t, hipStream_t);
template int launch_agc<float>(const AgcSettings &, AgcChan *, size_t, const float *, size_t, size_t, float *, size_t,
                               uint8_t *, size_t, hipStream_t);

template <class T>
int launch_agc_init(const T *x, size_t x_pitch, size_t n, size_t C, float *sum, hipStream_t st) {
    return bank_launch(agc_init_kernel<T>, C, kAgcWg, kAgcWg, 0, st, x, x_pitch, (unsigned)n, C, sum);
}
template int launch_agc_init<cf32>(const cf32 *, size_t, size_t, size_t, float *, hipStream_t);
template int launch_agc_init<float>(const float *, size_t, size_t, size_t, float *, hipStream_t);

template <class T>
void agc_host(const AgcSettings &g, AgcChan *state, size_t C, const T *x, size_t x_pitch, size_t n, T *y, size_t y_pitch,
              uint8_t *status, size_t status_pitch) {
    for (size_t c = 0; c < C; ++c) {
        AgcRegs s = agc_unpack(state[c]);
        for (size_t row = 0; row < n; ++row) {
            const T v = x[row * x_pitch + c];
            y[row * y_pitch + c] = g.squelch ? agc_step<true>(s, v, g.alpha, g.scale, g.threshold, g.timeout)
                                             : agc_step<false>(s, v, g.alpha, g.scale, g.threshold, g.timeout);
            if (status) status[row * status_pitch + c] = (uint8_t)s.mode;
        }
        state[c] = agc_pack(s);
    }
}
template void agc_host<cf32>(const AgcSettings &, AgcChan *, size_t, const cf32 *, size_t, size_t, cf32 *, size_t, uint8_t *,
                             size_t);
template void agc_host<float>(const AgcSettings &, AgcChan *, size_t, const float *, size_t, size_t, float *, size_t,
                              uint8_t *, size_t);

template <class T>
void agc_init_host(const T *x, size_t x_pitch, size_t n, size_t C, float *sum) {
    for (size_t c = 0; c < C; ++c) {
        float acc = 0.0f;
        for (size_t i = 0; i < n; ++i) acc = acc + agc_norm(x[i * x_pitch + c]);
        sum[c] = acc;
    }
}
template void agc_init_host<cf32>(const cf32 *, size_t, size_t, size_t, float *);
template void agc_init_host<float>(const float *, size_t, size_t, size_t, float *);

float agc_level_gain(float sum, size_t n) {
    const float x2 = sqrtf(sum / (float)n) + 1e-16f;
    return 1.0f / x2;
}
float agc_rssi_gain(float rssi) {
    const float g = yg_exp10_rssi(rssi);
    return g >= 1e-16f ? g : 1e-16f;                        // f32::max: a NaN becomes 1e-16
}
float agc_rssi(float g) { return -20.0f * yg_log10f(g); }
void agc_words_host(int word, const float *x, size_t n, float *y) {
    for (size_t i = 0; i < n; ++i) y[i] = word == 0 ? yg_lnf(x[i]) : word == 1 ? yg_expf(x[i]) : yg_log10f(x[i]);
}

}  // namespace yagi
