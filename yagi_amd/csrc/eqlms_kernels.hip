// eqlms_kernels.hip -- EqLms: the LMS equalizer (src/equalization/eqlms.rs) for a bank of independent channels.
//
// The object is a control loop along time: the weights of symbol i + 1 depend on output i, so a channel has no block
// form.  Across channels nothing is shared but the design, and a channelizer's output is laid out [step][channel]: one
// lane runs one channel's sequential loop word for word, and a wave's load of a row is contiguous.
//
// Per input row a lane pushes its sample (push :125-129: the window, then x2_sum += x2_n - x2_0, where x2_0 is recomputed
// from the sample that leaves the window, the same expression WDelay(h_len) would hand back) and then, depending on the
// call, forms y = sum conj(w0[i]) r[i] over the window oldest first (execute :137-140) and runs step (:170-187) or
// step_blind (:189-192).  Every product, add and quotient is rounded on its own.  The two quotients per tap of the
// weight update are the f32 roundings of f64 quotients (53 >= 2 24 + 2 bits: the double rounding cannot change the
// word), so the listing holds no f32 FMA at all (tests/test_eqlms_isa_cpu.py).  |y| of step_blind is the library's own
// word, (float)sqrt((double)re re + (double)im im) (yagi_hip.h).
//
// eqlms_cccf_kernel<CALL>: a workgroup is one wave of 64 channels and loops over all n rows of the call.  The window is
// an LDS ring [slot][lane] and the weights an LDS array [tap][lane], 512 bytes per tap each; the slot index is
// wave-uniform because every lane pushes on every row.  Both are filled from and written back to the object's [h_len][C]
// arrays once per call; x2_sum and count travel in one 16-byte EqlmsChan.  Input rows (and the rows of known symbols of
// TRAIN) are requested a chunk ahead into registers and staged in LDS; the DECISION table sits in LDS behind them.
// The weight update is a second pass over LDS, not fused into the next symbol's sum: fusing would save 16 of the 40 LDS
// bytes per tap and lane, 8 cycles per tap and wave, against the 158 VALU cycles of the two f64 quotients of that tap;
// the kernel sits against the VALU bound.  The tap loops are unrolled by four: measured faster
// than by one and no slower than by eight.
// count differs between lanes only after reset_channel(c); the buf_full gate and execute_block's update test are per
// lane for that reason and uniform otherwise.  A bank of few channels uses few lanes of its one wave.  Accepted.
//
// The launch is bank_launch and the host form fills and stores its window through Ring (bank_lane.hpp).  The kernel keeps
// its own prefetch and ring: on RowQueue alone DECISION ran 0.4 to 1 % longer (the other four up to 10 % shorter), on Ring
// alone NONE and DECISION 5 to 13 % longer (profiles/r29_kbench_bank_lanes.txt).
// The host form lives here too: host.cpp is built with contraction on.
#pragma clang fp contract(off)

#include <cmath>

#include "bank_lane.hpp"
#include "eqlms_body.hpp"     // eq_push .. eq_desired: shared with symtrack_kernels.hip
#include "kernels.hpp"

namespace yagi {
namespace {

struct EqArgs {
    cf32 *w, *hist;
    EqlmsChan *state;
    const cf32 *x, *d, *table;
    cf32 *y;
    size_t C, x_pitch, d_pitch, y_pitch;
    unsigned n, k, h_len, M;
    float mu;
    double one;        // an exact 1.0 the compiler cannot see (eq_quot)
};

// CALL: YAGI_EQLMS_NONE .. YAGI_EQLMS_DECISION = decim_block in that mode, kEqlmsExec = execute_block
template <int CALL>
__global__ __launch_bounds__(kEqlmsWg) void eqlms_cccf_kernel(const EqArgs a) {
    extern __shared__ __align__(16) unsigned char eq_smem[];
    const unsigned h_len = a.h_len, lane = threadIdx.x, k = a.k;
    cf32 *ring = reinterpret_cast<cf32 *>(eq_smem) + lane;
    cf32 *wl = reinterpret_cast<cf32 *>(eq_smem + eqlms_taps_bytes(h_len)) + lane;
    cf32 *stage = reinterpret_cast<cf32 *>(eq_smem + 2 * eqlms_taps_bytes(h_len)) + lane;
    cf32 *dstage = reinterpret_cast<cf32 *>(eq_smem + 2 * eqlms_taps_bytes(h_len) + eqlms_stage_bytes()) + lane;
    cf32 *tl = reinterpret_cast<cf32 *>(eq_smem + 2 * eqlms_taps_bytes(h_len) + eqlms_stage_bytes() + eqlms_dstage_bytes());
    constexpr unsigned S = kEqlmsWg;
    if (CALL == YAGI_EQLMS_DECISION) {
        for (unsigned i = lane; i < a.M; i += S) tl[i] = a.table[i];
        __syncthreads();
    }
    const size_t c = (size_t)blockIdx.x * S + lane;
    if (c >= a.C) return;                                   // a lane beyond the last channel does nothing

    EqlmsChan s = a.state[c];
    for (unsigned j = 0; j < h_len; ++j) {
        ring[j * S] = a.hist[(size_t)j * a.C + c];
        wl[j * S] = a.w[(size_t)j * a.C + c];
    }
    unsigned head = 0;                                      // the oldest slot, where the next sample goes
    // pushes until count >= h_len (the buf_full gate), and count mod k for execute_block's update test
    unsigned togo = s.count < h_len ? h_len - (unsigned)s.count : 0u;
    unsigned ph = 0;
    if (CALL == kEqlmsExec)                                 // count mod k by shift and subtract, k < 2^31: the compiler's
        for (int b = 63; b >= 0; --b) {                     // own u64 remainder runs through an f32 FMA
            ph = (ph << 1) | (unsigned)((s.count >> b) & 1ull);
            ph = ph >= k ? ph - k : ph;
        }
    const unsigned ph_upd = k == 1 ? 0u : 1u;               // (count + k - 1) % k == 0
    unsigned dp = 0, sym = 0;                               // decim_block: the row's place in its symbol, the symbol
    cf32 yv{0.0f, 0.0f};

    // The call's rows come in chunks of kEqlmsAhead: a chunk is requested into registers while the chunk before it is
    // worked through, and moves to its LDS stage when its turn comes, so a step never waits for a memory round trip.
    // TRAIN's known symbols do the same in chunks of kEqlmsAheadD symbols.
    cf32 xq[kEqlmsAhead], dq[kEqlmsAheadD];
#pragma unroll
    for (int u = 0; u < kEqlmsAhead; ++u)
        xq[u] = (unsigned)u < a.n ? a.x[(size_t)u * a.x_pitch + c] : cf32{0.0f, 0.0f};
    const unsigned nsym = CALL == YAGI_EQLMS_TRAIN ? a.n / k : 0u;
    unsigned d_end = 0;                                     // symbols [d_end - kEqlmsAheadD, d_end) are staged
    if (CALL == YAGI_EQLMS_TRAIN) {
#pragma unroll
        for (int u = 0; u < kEqlmsAheadD; ++u)
            dq[u] = (unsigned)u < nsym ? a.d[(size_t)u * a.d_pitch + c] : cf32{0.0f, 0.0f};
    }

    for (unsigned s0 = 0; s0 < a.n; s0 += kEqlmsAhead) {
#pragma unroll
        for (int u = 0; u < kEqlmsAhead; ++u) stage[u * S] = xq[u];
#pragma unroll
        for (int u = 0; u < kEqlmsAhead; ++u) {
            const size_t ahead = (size_t)s0 + kEqlmsAhead + u;
            xq[u] = ahead < a.n ? a.x[ahead * a.x_pitch + c] : cf32{0.0f, 0.0f};
        }
        const unsigned steps = a.n - s0 < (unsigned)kEqlmsAhead ? a.n - s0 : (unsigned)kEqlmsAhead;
        for (unsigned u = 0; u < steps; ++u) {
            eq_push(ring, S, head, h_len, stage[u * S], s.x2_sum);
            togo = togo ? togo - 1 : 0u;
            if (CALL == kEqlmsExec) {
                yv = eq_execute(ring, wl, S, head, h_len);
                a.y[(size_t)(s0 + u) * a.y_pitch + c] = yv;
                ph = ph + 1 == k ? 0u : ph + 1;
                if (ph == ph_upd && togo == 0)
                    eq_step(ring, wl, S, head, h_len, a.mu, s.x2_sum, eq_unit(yv, a.one), yv, a.one);
            } else {
                if (dp == 0) {
                    yv = eq_execute(ring, wl, S, head, h_len);
                    a.y[(size_t)sym * a.y_pitch + c] = yv;
                }
                dp = dp + 1 == k ? 0u : dp + 1;
                if (dp == 0) {                              // the symbol's last row: one update, then the next symbol
                    cf32 dk{0.0f, 0.0f};
                    if (CALL == YAGI_EQLMS_TRAIN) {
                        if (sym >= d_end) {
#pragma unroll
                            for (int v = 0; v < kEqlmsAheadD; ++v) dstage[v * S] = dq[v];
                            d_end += kEqlmsAheadD;
#pragma unroll
                            for (int v = 0; v < kEqlmsAheadD; ++v) {
                                const size_t ahead = (size_t)d_end + v;
                                dq[v] = ahead < nsym ? a.d[ahead * a.d_pitch + c] : cf32{0.0f, 0.0f};
                            }
                        }
                        dk = dstage[(sym - (d_end - kEqlmsAheadD)) * S];
                    }
                    if (CALL != YAGI_EQLMS_NONE && togo == 0)
                        eq_step(ring, wl, S, head, h_len, a.mu, s.x2_sum, eq_desired(CALL, yv, dk, tl, a.M, a.one), yv,
                                a.one);
                    ++sym;
                }
            }
        }
    }

    s.count += a.n;
    a.state[c] = s;
    for (unsigned j = 0; j < h_len; ++j) {                  // the window, oldest first, and the weights
        unsigned sl = head + j;
        sl = sl >= h_len ? sl - h_len : sl;
        a.hist[(size_t)j * a.C + c] = ring[sl * S];
        a.w[(size_t)j * a.C + c] = wl[j * S];
    }
}

template <int CALL>
int eq_launch(const EqArgs &a, hipStream_t st) {
    return bank_launch(eqlms_cccf_kernel<CALL>, a.C, kEqlmsWg, kEqlmsWg, eqlms_lds_bytes(a.h_len), st, a);
}

}  // namespace

int launch_eqlms(int call, size_t h_len, float mu, cf32 *w, cf32 *hist, EqlmsChan *state, size_t C, size_t k, const cf32 *x,
                 size_t x_pitch, size_t n, const cf32 *d, size_t d_pitch, const cf32 *table, size_t M, cf32 *y,
                 size_t y_pitch, hipStream_t st) {
    EqArgs a{};
    a.w = w, a.hist = hist, a.state = state, a.x = x, a.d = d, a.table = table, a.y = y;
    a.C = C, a.x_pitch = x_pitch, a.d_pitch = d_pitch, a.y_pitch = y_pitch;
    a.n = (unsigned)n, a.k = (unsigned)k, a.h_len = (unsigned)h_len, a.M = (unsigned)M;
    a.mu = mu;
    a.one = 1.0;
    switch (call) {
    case YAGI_EQLMS_NONE: return eq_launch<YAGI_EQLMS_NONE>(a, st);
    case YAGI_EQLMS_TRAIN: return eq_launch<YAGI_EQLMS_TRAIN>(a, st);
    case YAGI_EQLMS_BLIND: return eq_launch<YAGI_EQLMS_BLIND>(a, st);
    case YAGI_EQLMS_DECISION: return eq_launch<YAGI_EQLMS_DECISION>(a, st);
    case kEqlmsExec: return eq_launch<kEqlmsExec>(a, st);
    }
    return fail(YAGI_ERR_CONFIG, "eqlms: unknown update mode %d", call);
}

void eqlms_host(int call, size_t h_len_, float mu, cf32 *w, cf32 *hist, EqlmsChan *state, size_t C, size_t k_, const cf32 *x,
                size_t x_pitch, size_t n, const cf32 *d, size_t d_pitch, const cf32 *table, size_t M, cf32 *y,
                size_t y_pitch) {
    const unsigned h_len = (unsigned)h_len_, k = (unsigned)k_;
    std::vector<cf32> rv(h_len), wv(h_len);
    for (size_t c = 0; c < C; ++c) {
        EqlmsChan s = state[c];
        Ring<cf32> ring{rv.data(), 1, h_len, 0};
        ring.fill(hist, C, c);
        for (unsigned j = 0; j < h_len; ++j) wv[j] = w[(size_t)j * C + c];
        for (size_t row = 0; row < n; ++row) {
            eq_push(ring.col, 1, ring.head, h_len, x[row * x_pitch + c], s.x2_sum);
            s.count += 1;
            const bool full = s.count >= h_len;
            if (call == kEqlmsExec) {
                const cf32 yv = eq_execute(ring.col, wv.data(), 1, ring.head, h_len);
                y[row * y_pitch + c] = yv;
                if ((s.count + k - 1) % k == 0 && full)
                    eq_step(ring.col, wv.data(), 1, ring.head, h_len, mu, s.x2_sum, eq_unit(yv, 1.0), yv, 1.0);
            } else if (row % k == 0) {
                const size_t sym = row / k;
                const cf32 yv = eq_execute(ring.col, wv.data(), 1, ring.head, h_len);
                y[sym * y_pitch + c] = yv;
                for (unsigned u = 1; u < k; ++u) {          // the symbol's k - 1 trailing pushes, then one update
                    ++row;
                    eq_push(ring.col, 1, ring.head, h_len, x[row * x_pitch + c], s.x2_sum);
                    s.count += 1;
                }
                if (call != YAGI_EQLMS_NONE && s.count >= h_len) {
                    const cf32 dk = call == YAGI_EQLMS_TRAIN ? d[sym * d_pitch + c] : cf32{0.0f, 0.0f};
                    eq_step(ring.col, wv.data(), 1, ring.head, h_len, mu, s.x2_sum,
                            eq_desired(call, yv, dk, table, (unsigned)M, 1.0), yv, 1.0);
                }
            }
        }
        ring.store(hist, C, c);
        for (unsigned j = 0; j < h_len; ++j) w[(size_t)j * C + c] = wv[j];
        state[c] = s;
    }
}

}  // namespace yagi
