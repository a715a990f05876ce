// eqrls_kernels.hip -- EqRls: the recursive-least-squares equalizer (src/equalization/eqrls.rs) for a bank of independent
// channels.
//
// Like EqLms the object is a loop along time with no block form, and across channels nothing is shared but the design.
// Unlike EqLms a step is O(p^3): gxlp0 = gxl P0 is a plain triple loop in the reference, and its words do not survive a
// regrouping.  One lane per channel would leave a small bank on a sliver of one CU and, from p = 12, would not fit 64
// matrices in LDS.  So a group of L lanes (a power of two, planned in kernels.hpp, overridable for tests) shares one
// channel's step, and a wave holds G = 64 / L channels.
//
// Every sum of the recursion is owned whole by one lane and runs in the sequential loop's order (eqrls_body.hpp): lane t of
// a group owns columns t, t + L, ... of xp0, gxlp0 and P1 and rows t, t + L, ... of g and w; zeta and y are p terms and are
// formed by every lane.  There is no cross-lane reduction.  Lanes exchange finished values through LDS; the workgroup
// is one wave, its LDS operations execute in issue order, so the exchange needs no s_barrier, only a fence that keeps the
// compiler from moving LDS accesses across it (rls_sync).  gxl is formed once per step, a row at a time, its p elements
// spread over the group, 4 f64 quotients each.  Column c of P1 needs all of column c of P0, so P1 is written to a second
// buffer and the two change places after the step; a step costs p + 3 syncs.
//
// LDS layout: every array is [element][channel-in-wave], and lane = t G + g (g the channel in the wave).  The lanes of a
// wave that read P0[i][c = t + j L] for one i and j then read 64 consecutive cf32, conflict free; values that a whole
// group reads (x[i], a gxl row, g[r]) are G consecutive cf32 with a broadcast inside each group.  [channel][element]
// would put the groups p pp elements apart, the same banks for every p pp that is a multiple of 32.  The one access that
// runs along rows, the numerators of g, has the lanes of a group p pp' G elements apart; the row pitch pp' = p | 1 is odd,
// so the L / 2 groups' worth of t inside a 32-lane half fall on different banks.  State is read from and written back to
// the object's [element][channel] arrays once per call.
//
// Input rows go through the bank kernels' row queue (bank_lane.hpp) in chunks of kEqrlsAhead, held and staged by each
// group's lane 0; the window is that header's Ring at stride G, written by lane 0 and advanced by every lane.  TRAIN's
// symbol is requested one symbol ahead by every lane of the group (one address per group), behind a step that
// is much longer than the round trip.  Control flow is uniform across the wave: a group beyond the last channel runs on
// zeros and stores nothing.
//
// The quotients are f32 roundings of f64 quotients (eq_quot), so the listing holds no f32 FMA (tests/test_eqrls_isa_cpu.py).
// The host form lives here too: host.cpp is built with contraction on.
#pragma clang fp contract(off)

#include <cmath>

#include "eqrls_body.hpp"
#include "kernels.hpp"

namespace yagi {
namespace {

struct RlsArgs {
    cf32 *P, *w0, *w1, *hist;
    const cf32 *x, *d, *table;
    cf32 *y;
    size_t C, x_pitch, d_pitch, y_pitch;
    unsigned n, k, p, M, lgL;
    float lambda;
    double one;        // an exact 1.0 the compiler cannot see (eq_quot)
};

// the exchange point of a group: all lanes of the wave are here together and LDS serves a wave in order
__device__ __forceinline__ void rls_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int MODE>
__global__ __launch_bounds__(kEqrlsWg) void eqrls_cccf_kernel(const RlsArgs a) {
    extern __shared__ __align__(16) unsigned char rls_smem[];
    const unsigned p = a.p, pp = (unsigned)eqrls_pitch(p), k = a.k, lane = threadIdx.x;
    const unsigned L = 1u << a.lgL, G = (unsigned)kEqrlsWg >> a.lgL;
    const unsigned g = lane & (G - 1), t = lane >> (6 - a.lgL);
    cf32 *base = reinterpret_cast<cf32 *>(rls_smem) + g;
    RlsView v;
    v.stride = G, v.p = p, v.pp = pp;
    v.P0 = base, base += (size_t)p * pp * G;
    v.P1 = base, base += (size_t)p * pp * G;
    v.ring = Ring<cf32>{base, G, p, 0}, base += (size_t)p * G;
    v.w = base, base += (size_t)p * G;
    v.xp0 = base, base += (size_t)p * G;
    v.g = base, base += (size_t)p * G;
    v.row = base, base += (size_t)2 * p * G;
    cf32 *stage = base;                                     // [row of the chunk][g], written and read by lane t = 0 alone
    base += (size_t)kEqrlsAhead * G;
    const cf32 *tl = base - g;
    if (MODE == YAGI_EQRLS_DECISION)
        for (unsigned i = lane; i < a.M; i += kEqrlsWg) (base - g)[i] = a.table[i];

    const size_t c = (size_t)blockIdx.x * G + g;
    const bool act = c < a.C, first = act && t == 0;
    for (unsigned r = 0; r < p; ++r)
        for (unsigned j = t; j < p; j += L) v.P0[(r * pp + j) * G] = act ? a.P[((size_t)r * p + j) * a.C + c] : cf32{0.0f, 0.0f};
    for (unsigned j = t; j < p; j += L) v.w[j * G] = act ? a.w0[(size_t)j * a.C + c] : cf32{0.0f, 0.0f};
    v.ring.fill(a.hist, a.C, c, act, t, L);
    unsigned dp = 0, sym = 0;                               // the row's place in its symbol, the symbol
    const unsigned nsym = a.n / k;

    auto load = [&](size_t row, bool in_range) { return first && in_range ? a.x[row * a.x_pitch + c] : cf32{0.0f, 0.0f}; };
    RowQueue<cf32, kEqrlsAhead> xq;                         // held by each group's lane 0
    xq.prime(a.n, load);
    cf32 dnext = MODE == YAGI_EQRLS_TRAIN && act && nsym ? a.d[c] : cf32{0.0f, 0.0f};
    rls_sync();

    for (unsigned s0 = 0; s0 < a.n; s0 += kEqrlsAhead) {
        const unsigned steps = xq.next(s0, a.n, lane_stage(stage, G, t == 0), load);
        for (unsigned u = 0; u < steps; ++u) {
            v.ring.push(stage[u * G], t == 0);              // the oldest sample leaves; lane 0 of the group writes
            rls_sync();
            if (dp == 0) {                                  // the symbol's first row: execute, then the update
                const cf32 yv = rls_execute(v);
                if (first) a.y[(size_t)sym * a.y_pitch + c] = yv;
                if (MODE != YAGI_EQRLS_NONE) {
                    const cf32 dk = dnext;
                    if (MODE == YAGI_EQRLS_TRAIN)
                        dnext = act && sym + 1 < nsym ? a.d[(size_t)(sym + 1) * a.d_pitch + c] : cf32{0.0f, 0.0f};
                    rls_sync();                             // every lane has its y before a lane writes w
                    rls_step(v, t, L, a.lambda, eq_desired(MODE, yv, dk, tl, a.M, a.one), yv, a.one,
                             [] { rls_sync(); });
                    rls_swap(v);
                }
                ++sym;
            }
            dp = dp + 1 == k ? 0u : dp + 1;
            rls_sync();                                     // the window is read out before the next push
        }
    }

    if (!act) return;
    for (unsigned r = 0; r < p; ++r)
        for (unsigned j = t; j < p; j += L) a.P[((size_t)r * p + j) * a.C + c] = v.P0[(r * pp + j) * G];
    const bool stepped = MODE != YAGI_EQRLS_NONE && nsym != 0;
    v.ring.store(a.hist, a.C, c, t, L);
    for (unsigned j = t; j < p; j += L) {
        const cf32 w = v.w[j * G];
        a.w0[(size_t)j * a.C + c] = w;
        if (stepped) a.w1[(size_t)j * a.C + c] = w;         // step leaves w1 = w0 (:140-143)
    }
}

template <int MODE>
int rls_launch(const RlsArgs &a, hipStream_t st) {
    const size_t L = (size_t)1 << a.lgL, G = kEqrlsWg / L;
    return bank_launch(eqrls_cccf_kernel<MODE>, a.C, G, kEqrlsWg, eqrls_lds_bytes(a.p, L), st, a);
}

}  // namespace

int launch_eqrls(int mode, size_t p, size_t L, float lambda, cf32 *P, cf32 *w0, cf32 *w1, cf32 *hist, size_t C, size_t k,
                 const cf32 *x, size_t x_pitch, size_t n, const cf32 *d, size_t d_pitch, const cf32 *table, size_t M, cf32 *y,
                 size_t y_pitch, hipStream_t st) {
    unsigned lgL = 0;
    while (((size_t)1 << lgL) < L) ++lgL;
    if (lgL > 6 || ((size_t)1 << lgL) != L || !(eqrls_admissible(p) >> lgL & 1u))
        return fail(YAGI_ERR_CONFIG, "eqrls: %zu lanes per channel are not admissible at p = %zu", L, p);
    RlsArgs a{};
    a.P = P, a.w0 = w0, a.w1 = w1, a.hist = hist, a.x = x, a.d = d, a.table = table, a.y = y;
    a.C = C, a.x_pitch = x_pitch, a.d_pitch = d_pitch, a.y_pitch = y_pitch;
    a.n = (unsigned)n, a.k = (unsigned)k, a.p = (unsigned)p, a.M = (unsigned)M, a.lgL = lgL;
    a.lambda = lambda;
    a.one = 1.0;
    switch (mode) {
    case YAGI_EQRLS_NONE: return rls_launch<YAGI_EQRLS_NONE>(a, st);
    case YAGI_EQRLS_TRAIN: return rls_launch<YAGI_EQRLS_TRAIN>(a, st);
    case YAGI_EQRLS_DECISION: return rls_launch<YAGI_EQRLS_DECISION>(a, st);
    }
    return fail(YAGI_ERR_CONFIG, "eqrls: unknown update mode %d", mode);
}

void eqrls_host(int mode, size_t p_, float lambda, cf32 *P, cf32 *w0, cf32 *w1, cf32 *hist, size_t C, size_t k_, const cf32 *x,
                size_t x_pitch, size_t n, const cf32 *d, size_t d_pitch, const cf32 *table, size_t M, cf32 *y,
                size_t y_pitch) {
    const unsigned p = (unsigned)p_, k = (unsigned)k_;
    std::vector<cf32> Pa((size_t)p * p), Pb((size_t)p * p), ring(p), wv(p), xp0(p), gv(p), row(2 * (size_t)p);
    for (size_t c = 0; c < C; ++c) {
        for (size_t e = 0; e < (size_t)p * p; ++e) Pa[e] = P[e * C + c];
        for (unsigned j = 0; j < p; ++j) wv[j] = w0[(size_t)j * C + c];
        RlsView v{Pa.data(), Pb.data(), Ring<cf32>{ring.data(), 1, p, 0}, wv.data(), xp0.data(), gv.data(), row.data(), 1, p, p};
        v.ring.fill(hist, C, c);
        bool stepped = false;
        for (size_t r = 0; r < n; ++r) {
            v.ring.push(x[r * x_pitch + c]);
            if (r % k != 0) continue;
            const size_t sym = r / k;
            const cf32 yv = rls_execute(v);
            y[sym * y_pitch + c] = yv;
            if (mode == YAGI_EQRLS_NONE) continue;
            const cf32 dk = mode == YAGI_EQRLS_TRAIN ? d[sym * d_pitch + c] : cf32{0.0f, 0.0f};
            rls_step(v, 0, 1, lambda, eq_desired(mode, yv, dk, table, (unsigned)M, 1.0), yv, 1.0, [] {});
            rls_swap(v);
            stepped = true;
        }
        for (size_t e = 0; e < (size_t)p * p; ++e) P[e * C + c] = v.P0[e];
        v.ring.store(hist, C, c);
        for (unsigned j = 0; j < p; ++j) {
            w0[(size_t)j * C + c] = wv[j];
            if (stepped) w1[(size_t)j * C + c] = wv[j];
        }
    }
}

}  // namespace yagi
