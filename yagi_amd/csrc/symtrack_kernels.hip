// symtrack_kernels.hip -- SymTrack: agc -> symsync -> nco -> eqlms -> modem with the carrier loop closed per symbol, for a
// bank of independent channels (yagi_hip.h, "SymTrack: the definition").
//
// The object is five control loops along time that feed one another: the decision of symbol i steers the oscillator that
// de-rotates the samples of symbol i + 1 in front of the equalizer, so a channel has no block form and the loop cannot be
// cut into launches.  Across channels nothing is shared but the design, and a channelizer's output is laid out
// [step][channel]: one lane carries all five states of its channel through each sample, and a wave's load of a row is
// contiguous.  The per-sample arithmetic is the standalone objects' own source (agc_body.hpp, symsync_body.hpp,
// osc_mix.hpp, eqlms_body.hpp, modem_body.hpp): every product, add and quotient is rounded on its own, the quotients are
// f32 roundings of f64 quotients, and the listing holds no f32 FMA (tests/test_symtrack_isa_cpu.py).
//
// symtrack_cccf_kernel<LDS_TAPS>: a workgroup is one wave of 64 channels and loops over all n rows of the call.
//   registers   the agc record, the synchroniser's scalars, theta / d_theta, sync_index, num_syms, x2_sum and count
//   LDS [.][lane]  the synchroniser's window (a ring with a wave-uniform head: every lane pushes on every row), the
//               equalizer's window (a ring with a head per lane: a lane pushes once per synchroniser output) and weights
//   LDS shared  the staged input rows, the oscillator table (NCO float2, VCO float4), the constellation with reference[],
//               and the interleaved (H, D) branch taps where they fit (else they stay in global memory)
// The two rings, the rows requested a chunk of kSymtrackAhead ahead and the launch are the bank kernels' scaffold
// (bank_lane.hpp); the synchroniser's row is ss_row (symsync_body.hpp) with st_after_sync behind it.  The oscillator
// scheme, the equalizer strategy and the modem's kind and bps are wave-uniform run-time branches; only LDS_TAPS, which
// sits in the tap loop, is a template parameter.  Lanes that emit on different rows serialise in the inner loop.  Accepted.
//
// Stalls: an iteration about to emit symbol number ycap does not run (CAPACITY); a pll_step whose argument reaches
// YAGI_SYMTRACK_PLL_ARG_MAX does not run, nor anything behind it in that iteration (PLL).  A stalled lane writes its
// synchroniser window out at once and does nothing more.  The inner loop is also counted, 2 (ycap - ny) + 1 per row.
//
// The host form lives here too: host.cpp is built with contraction on.
#pragma clang fp contract(off)

#include <cmath>

#include "agc_body.hpp"
#include "eqlms_body.hpp"
#include "kernels.hpp"
#include "modem_body.hpp"
#include "osc_mix.hpp"
#include "symsync_body.hpp"

namespace yagi {
namespace {

#define ST_HD __host__ __device__ __forceinline__

// constrain (osc.rs:191-201) for |theta| < YAGI_SYMTRACK_PLL_ARG_MAX or NaN: the reference's loops word for word (at most
// 41 turns, counted all the same), then `(theta / 2 pi * 2^32) as u32`, saturating, NaN -> 0
ST_HD uint32_t st_constrain(float theta, double zero) {
    for (int i = 0; i < 64 && theta >= kTwoPi; ++i) theta = theta - kTwoPi;
    for (int i = 0; i < 64 && theta < 0.0f; ++i) theta = theta + kTwoPi;
    const float v = ss_quot(theta, kTwoPi, zero) * 4294967296.0f;
    if (!(v > 0.0f)) return 0u;
    if (v >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)v;
}

ST_HD cf32 st_mix_down(int vco, const void *tab, uint32_t theta, cf32 s) {
    const float2 u = vco ? osc_one<1, true>(static_cast<const float4 *>(tab), theta, s.re, s.im)
                         : osc_one<0, true>(static_cast<const float2 *>(tab), theta, s.re, s.im);
    return cf32{u.x, u.y};
}

// a channel's scalars in registers
struct StRegs {
    AgcRegs ag;
    SymsyncChan ss;
    SymtrackChan st;
    float x2_sum;
    unsigned long long count;
};

// Everything of one iteration behind the synchroniser's output s: returns 0 where nothing is emitted (an odd output),
// 1 where (d_hat, sym) is, and -1 where the PLL rule stalls the channel.
ST_HD int st_after_sync(StRegs &r, const SymtrackLoop &p, const void *osc_tab, const float *ref, const cf32 *map,
                        Ring<cf32> &eq_ring, cf32 *eq_w, cf32 s, cf32 &d_hat, unsigned &sym, double zero, double one) {
    const cf32 u = st_mix_down((int)p.vco, osc_tab, r.st.theta, s);
    r.st.theta += r.st.d_theta;
    eq_push(eq_ring.col, eq_ring.stride, eq_ring.head, p.h_len, u, r.x2_sum);
    r.count += 1;
    const unsigned j = r.st.index;
    r.st.index = j + 1;
    if (j & 1u) return 0;
    d_hat = eq_execute(eq_ring.col, eq_w, eq_ring.stride, eq_ring.head, p.h_len);
    cf32 xh;
    sym = md_hard(p.kind, p.bps, ref, map, d_hat, xh);
    const float e = d_hat.re * (-xh.im) + d_hat.im * xh.re;             // (r * conj(x_hat)).im
    const float fa = e * p.pll_alpha, fb = e * p.pll_beta;
    if (fabsf(fa) >= YAGI_SYMTRACK_PLL_ARG_MAX || fabsf(fb) >= YAGI_SYMTRACK_PLL_ARG_MAX) return -1;
    r.st.d_theta += st_constrain(fa, zero);
    r.st.theta += st_constrain(fb, zero);
    if (r.st.num_syms > p.holdoff && p.strategy != YAGI_SYMTRACK_EQ_OFF && r.count >= p.h_len) {
        const cf32 d = p.strategy == YAGI_SYMTRACK_EQ_CM ? eq_unit(d_hat, one) : xh;
        eq_step(eq_ring.col, eq_w, eq_ring.stride, eq_ring.head, p.h_len, p.eq_mu, r.x2_sum, d, d_hat, one);
    }
    r.st.num_syms += 1;
    return 1;
}

struct StArgs {
    SymtrackLoop p;
    SymtrackState s;
    const SsTap *taps;
    const void *osc_tab;
    const cf32 *map;   // the M points, then reference[8] as floats
    const cf32 *x;
    cf32 *y;
    uint8_t *sym;
    unsigned *status;
    size_t C, x_pitch, y_pitch, sym_pitch;
    unsigned n, ycap;
    double zero, one;  // an exact 0.0 and 1.0 the compiler cannot see: they keep the quotients f64 expressions
};

template <bool LDS_TAPS>
__global__ __launch_bounds__(kSymtrackWg) void symtrack_cccf_kernel(const StArgs a) {
    extern __shared__ __align__(16) unsigned char st_smem[];
    constexpr unsigned S = kSymtrackWg;
    const SymtrackLoop &p = a.p;
    const SymsyncLoop ssl = a.p.ss;
    const unsigned Ls = ssl.Ls, L = p.h_len, lane = threadIdx.x;
    unsigned char *at = st_smem;
    Ring<cf32> win{reinterpret_cast<cf32 *>(at) + lane, S, Ls, 0};       // the synchroniser's window
    at += symsync_ring_bytes(Ls);
    Ring<cf32> eq_ring{reinterpret_cast<cf32 *>(at) + lane, S, L, 0};
    at += eqlms_taps_bytes(L);
    cf32 *eq_w = reinterpret_cast<cf32 *>(at) + lane;
    at += eqlms_taps_bytes(L);
    cf32 *stage = reinterpret_cast<cf32 *>(at) + lane;
    at += symtrack_stage_bytes();
    float *osc_l = reinterpret_cast<float *>(at);
    at += symtrack_osc_bytes(p.vco);
    cf32 *map_l = reinterpret_cast<cf32 *>(at);
    at += (size_t)p.M * sizeof(cf32);
    float *ref_l = reinterpret_cast<float *>(at);
    at += 8 * sizeof(float);
    SsTap *tl = reinterpret_cast<SsTap *>(at);

    const size_t c = (size_t)blockIdx.x * S + lane;
    const bool live = c < a.C;

    StRegs r{};
    r.st.stall = YAGI_SYMTRACK_STALL_CAPACITY;              // a lane beyond the last channel does nothing
    if (live) {
        r.ag = agc_unpack(a.s.agc[c]);
        r.ss = a.s.ss[c];
        r.st = a.s.st[c];
        const EqlmsChan e = a.s.eq[c];
        r.x2_sum = e.x2_sum;
        r.count = e.count;
    }
    const bool was_stalled = r.st.stall != 0;
    win.fill(a.s.ss_hist, a.C, c, live);
    for (unsigned j = 0; j < L; ++j) eq_w[j * S] = live ? a.s.eq_w[(size_t)j * a.C + c] : cf32{0.0f, 0.0f};
    eq_ring.fill(a.s.eq_hist, a.C, c, live);
    {
        const float *g = static_cast<const float *>(a.osc_tab);
        const unsigned words = (unsigned)(symtrack_osc_bytes(p.vco) / sizeof(float));
        for (unsigned i = lane; i < words; i += S) osc_l[i] = g[i];
        const float *gm = reinterpret_cast<const float *>(a.map);           // M points, then reference[8]
        float *ml = reinterpret_cast<float *>(map_l);
        for (unsigned i = lane; i < 2 * p.M + 8; i += S) ml[i] = gm[i];
        if (LDS_TAPS)
            for (unsigned i = lane; i < ssl.npfb * Ls; i += S) tl[i] = a.taps[i];
    }
    __syncthreads();

    unsigned ny = 0;
    const SsTap *taps = LDS_TAPS ? tl : a.taps;
    auto window_out = [&] { win.store(a.s.ss_hist, a.C, c); };          // a lane that stalls writes its window out at once
    auto any = [](bool m) { return __any(m) != 0; };
    auto full = [&] { return !(r.st.index & 1u) && ny >= a.ycap; };
    auto emit = [&](cf32 sv) -> uint32_t {
        cf32 d_hat{0.0f, 0.0f};
        unsigned sym = 0;
        const int got = st_after_sync(r, p, osc_l, ref_l, map_l, eq_ring, eq_w, sv, d_hat, sym, a.zero, a.one);
        if (got < 0) return YAGI_SYMTRACK_STALL_PLL;
        if (got > 0) {
            a.y[(size_t)ny * a.y_pitch + c] = d_hat;
            if (a.sym) a.sym[(size_t)ny * a.sym_pitch + c] = (uint8_t)sym;
            ++ny;
        }
        return 0u;
    };

    auto load = [&](size_t row, bool in_range) { return live && in_range ? a.x[row * a.x_pitch + c] : cf32{0.0f, 0.0f}; };
    RowQueue<cf32, kSymtrackAhead> xq;
    xq.prime(a.n, load);
    for (unsigned s0 = 0; s0 < a.n; s0 += kSymtrackAhead) {
        const unsigned steps = xq.next(s0, a.n, lane_stage(stage, S), load);
        for (unsigned u = 0; u < steps; ++u) {
            cf32 v = stage[u * S];
            if (!r.st.stall) v = agc_step<false>(r.ag, v, p.agc_alpha, p.agc_scale, 0.0f, 0u);
            ss_row(r.ss, ssl, win, taps, v, r.st.stall, (uint32_t)YAGI_SYMTRACK_STALL_CAPACITY, a.ycap - ny, a.zero, any, full,
                   emit, window_out);
        }
    }

    if (live) {
        if (!was_stalled) {
            r.ss.stalled = r.st.stall != 0;
            a.s.agc[c] = agc_pack(r.ag);
            a.s.ss[c] = r.ss;
            a.s.st[c] = r.st;
            EqlmsChan e{};
            e.x2_sum = r.x2_sum;
            e.count = r.count;
            a.s.eq[c] = e;
            if (!r.st.stall) window_out();
            eq_ring.store(a.s.eq_hist, a.C, c);
            for (unsigned j = 0; j < L; ++j) a.s.eq_w[(size_t)j * a.C + c] = eq_w[j * S];
        }
        a.status[c] = ny;
        a.status[a.C + c] = r.st.stall;
        a.status[2 * a.C + c] = (unsigned)r.st.num_syms;
    }
}

}  // namespace

size_t symtrack_lds_bytes(size_t Ls, size_t h_len, int vco, size_t M) {
    return symsync_ring_bytes(Ls) + 2 * eqlms_taps_bytes(h_len) + symtrack_stage_bytes() + symtrack_osc_bytes(vco) +
           M * sizeof(cf32) + 8 * sizeof(float);
}

int launch_symtrack(const SymtrackLoop &p, const float *taps, const void *osc_tab, const cf32 *map, const SymtrackState &s,
                    size_t C, const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch, uint8_t *sym,
                    size_t sym_pitch, size_t ycap, unsigned *status, hipStream_t st) {
    StArgs a{};
    a.p = p, a.s = s;
    a.taps = reinterpret_cast<const SsTap *>(taps);
    a.osc_tab = osc_tab, a.map = map, a.x = x, a.y = y, a.sym = sym, a.status = status;
    a.C = C, a.x_pitch = x_pitch, a.y_pitch = y_pitch, a.sym_pitch = sym_pitch;
    a.n = (unsigned)n, a.ycap = (unsigned)ycap;
    a.zero = 0.0, a.one = 1.0;
    const size_t fixed = symtrack_lds_bytes(p.ss.Ls, p.h_len, (int)p.vco, p.M);
    if (fixed > kSymtrackLdsMax) return fail(YAGI_ERR_CONFIG, "symtrack: %zu bytes of LDS are more than 160 KiB", fixed);
    const size_t with_taps = fixed + symsync_table_bytes(p.ss.npfb, p.ss.Ls);
    const bool lds_taps = with_taps <= kSymtrackLdsMax;
    const size_t need = lds_taps ? with_taps : fixed;
    return bank_launch(lds_taps ? symtrack_cccf_kernel<true> : symtrack_cccf_kernel<false>, C, kSymtrackWg, kSymtrackWg, need, st,
                       a);
}

void symtrack_host(const SymtrackLoop &p, const float *taps_, const void *osc_tab, const cf32 *map, const SymtrackState &s,
                   size_t C, const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch, uint8_t *sym,
                   size_t sym_pitch, size_t ycap, unsigned *status) {
    const SsTap *taps = reinterpret_cast<const SsTap *>(taps_);
    const SymsyncLoop &ssl = p.ss;
    const unsigned Ls = ssl.Ls, L = p.h_len;
    std::vector<cf32> wv(Ls), ev(L), eq_w(L);
    for (size_t c = 0; c < C; ++c) {
        StRegs r{};
        r.ag = agc_unpack(s.agc[c]);
        r.ss = s.ss[c];
        r.st = s.st[c];
        r.x2_sum = s.eq[c].x2_sum;
        r.count = s.eq[c].count;
        unsigned ny = 0;
        if (!r.st.stall) {
            Ring<cf32> win{wv.data(), 1, Ls, 0}, eq_ring{ev.data(), 1, L, 0};
            win.fill(s.ss_hist, C, c);
            eq_ring.fill(s.eq_hist, C, c);
            for (unsigned j = 0; j < L; ++j) eq_w[j] = s.eq_w[(size_t)j * C + c];
            auto full = [&] { return !(r.st.index & 1u) && ny >= ycap; };
            auto emit = [&](cf32 sv) -> uint32_t {
                cf32 d_hat{0.0f, 0.0f};
                unsigned sy = 0;
                const int got = st_after_sync(r, p, osc_tab, p.ref, map, eq_ring, eq_w.data(), sv, d_hat, sy, 0.0, 1.0);
                if (got < 0) return YAGI_SYMTRACK_STALL_PLL;
                if (got > 0) {
                    y[(size_t)ny * y_pitch + c] = d_hat;
                    if (sym) sym[(size_t)ny * sym_pitch + c] = (uint8_t)sy;
                    ++ny;
                }
                return 0u;
            };
            for (size_t row = 0; row < n && !r.st.stall; ++row) {
                const cf32 v = agc_step<false>(r.ag, x[row * x_pitch + c], p.agc_alpha, p.agc_scale, 0.0f, 0u);
                ss_row(r.ss, ssl, win, taps, v, r.st.stall, (uint32_t)YAGI_SYMTRACK_STALL_CAPACITY, ycap - ny, 0.0,
                       [](bool m) { return m; }, full, emit, [] {});
            }
            r.ss.stalled = r.st.stall != 0;
            win.store(s.ss_hist, C, c);
            eq_ring.store(s.eq_hist, C, c);
            for (unsigned j = 0; j < L; ++j) s.eq_w[(size_t)j * C + c] = eq_w[j];
            s.agc[c] = agc_pack(r.ag);
            s.ss[c] = r.ss;
            s.st[c] = r.st;
            EqlmsChan e{};
            e.x2_sum = r.x2_sum;
            e.count = r.count;
            s.eq[c] = e;
        }
        status[c] = ny;
        status[C + c] = r.st.stall;
        status[2 * C + c] = (unsigned)r.st.num_syms;
    }
}

}  // namespace yagi
