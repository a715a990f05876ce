// symsync_kernels.hip -- SymSync: symbol timing recovery (src/filter/symsync.rs) for a bank of independent channels.
//
// The object is a control loop along time: the branch of output i + 1 depends on output i, so a channel has no block
// form.  Across channels nothing is shared but the design, and a channelizer's output is laid out [step][channel]: one
// lane runs one channel's sequential loop word for word, and a wave's load of a row is contiguous.
//
// Per step (step, :230-266) a lane pushes its sample and then, while b < npfb, forms the matched sum of row b (and on
// the iterations that update the loop the derivative sum of the same row), stores mf / Complex(k, 0), runs the loop
// filter where decim_counter == k_out, and advances tau, bf, b.  Sums run oldest first from +0.0 with every product and
// add rounded on its own.  The iteration a locked object repeats (`continue` with decim_counter = 0) forms the same sum
// and stores the same word again, so it is folded into the iteration before it: no second pass.  The two quotients of an
// output are the f32 roundings of f64 quotients (53 >= 2 24 + 2 bits: the double rounding cannot change the word), and
// `bf.round() as usize` shifts the significand by hand, so the listing holds no f32 FMA at all (tests/test_symsync_isa_cpu.py).
//
// symsync_crcf_kernel: a workgroup is one wave of 64 channels and loops over all n steps of the call.  The last Ls rows
// sit in an LDS ring [slot][lane] whose index is wave-uniform (every lane pushes on every step; a stalled lane's column
// is dead).  The ring is filled from and written back to the object's [Ls][C] history; the per-channel scalars travel in
// one 64-byte SymsyncChan.  Input rows are requested a chunk of kSymsyncAhead steps ahead and staged in LDS.  The two
// banks are interleaved, (H, D) per entry, so one gather serves both sums; the table sits in LDS behind the ring where
// both fit, else in global memory.
// The matched filter's window alone is cleared by reset(): a lane counts its samples since reset and reads +0.0 for older
// slots (a uniform branch picks the loop with the select only while some lane of the wave is that young).
// Lanes that emit on different steps serialise in the inner loop; at k = 2 up to half the wave idles.  Accepted.
//
// Capacity: an iteration about to store output number ycap does not run; the lane stalls, writes its window out at once
// and does nothing more.  The inner loop is also counted, 2 (ycap - ny) + 1 per step, so it ends whatever the state holds.
//
// The ring, the row queue and the launch are bank_lane.hpp's, in the kernel and in the host form; the host form's row is
// ss_row (symsync_body.hpp).  The kernel spells its row out: on ss_row it ran 2 to 4 % longer
// (profiles/r29_kbench_bank_lanes.txt).
// The host form lives here too: host.cpp is built with contraction on.
#pragma clang fp contract(off)

#include <cmath>

#include "kernels.hpp"
#include "symsync_body.hpp"   // SsTap, ss_row, ss_output: shared with symtrack_kernels.hip

namespace yagi {
namespace {

struct SsArgs {
    SymsyncLoop p;
    const SsTap *taps;
    SymsyncChan *state;
    cf32 *hist;
    const cf32 *x;
    cf32 *y;
    unsigned *status;
    size_t C, x_pitch, y_pitch;
    unsigned n, ycap;
    double zero;       // an exact 0.0 the compiler cannot see: it keeps the quotients f64 expressions
};

template <bool LDS_TAPS>
__global__ __launch_bounds__(kSymsyncWg) void symsync_crcf_kernel(const SsArgs a) {
    extern __shared__ __align__(16) unsigned char ss_smem[];
    const SymsyncLoop p = a.p;
    const unsigned Ls = p.Ls, lane = threadIdx.x;
    cf32 *ring = reinterpret_cast<cf32 *>(ss_smem);
    SsTap *tl = reinterpret_cast<SsTap *>(ss_smem + symsync_ring_bytes(Ls));
    const size_t c = (size_t)blockIdx.x * kSymsyncWg + lane;
    const bool live = c < a.C;

    SymsyncChan s{};
    s.stalled = 1;                                          // a lane beyond the last channel does nothing
    if (live) s = a.state[c];
    const bool was_stalled = s.stalled != 0;
    Ring<cf32> win{ring + lane, kSymsyncWg, Ls, 0};
    win.fill(a.hist, a.C, c, live);
    if (LDS_TAPS)
        for (unsigned i = lane; i < p.npfb * Ls; i += kSymsyncWg) tl[i] = a.taps[i];
    __syncthreads();

    unsigned ny = 0;
    auto window_out = [&] { win.store(a.hist, a.C, c); };   // the lane's window, oldest first, to the object's history
    cf32 *stage = reinterpret_cast<cf32 *>(ss_smem + symsync_ring_bytes(Ls) + (LDS_TAPS ? symsync_table_bytes(p.npfb, Ls) : 0));
    auto load = [&](size_t row, bool in_range) { return live && in_range ? a.x[row * a.x_pitch + c] : cf32{0.0f, 0.0f}; };
    RowQueue<cf32, kSymsyncAhead> xq;
    xq.prime(a.n, load);
    for (unsigned s0 = 0; s0 < a.n; s0 += kSymsyncAhead) {
        const unsigned steps = xq.next(s0, a.n, lane_stage(stage + lane, kSymsyncWg), load);
        for (unsigned u = 0; u < steps; ++u) {
            win.push(stage[u * kSymsyncWg + lane]);         // mf.push(x); dmf.push(x)
            if (!s.stalled && s.since < Ls) s.since += 1;
            const unsigned z = Ls - s.since;
            const bool young = __any(!s.stalled && z != 0) != 0;
            unsigned budget = 2u * (a.ycap - ny) + 1u;
            while (!s.stalled && s.b < p.npfb) {
                if (budget == 0 || ny >= a.ycap) {          // the capacity rule; budget == 0 cannot happen
                    s.stalled = 1;
                    window_out();
                    break;
                }
                --budget;
                const SsTap *row = (LDS_TAPS ? tl : a.taps) + (size_t)s.b * Ls;
                auto tap = [&](unsigned j) { return row[j]; };
                const cf32 yv = young ? ss_output<true>(s, p, z, win, tap, a.zero)
                                      : ss_output<false>(s, p, z, win, tap, a.zero);
                a.y[(size_t)ny * a.y_pitch + c] = yv;
                ++ny;
            }
            if (!s.stalled) {
                s.tau = s.tau - 1.0f;
                s.bf = s.bf - p.npfbf;
                s.b -= p.npfb;
            }
        }
    }

    if (live) {
        if (!was_stalled) {
            a.state[c] = s;
            if (!s.stalled) window_out();
        }
        a.status[c] = ny;
        a.status[a.C + c] = s.stalled;
    }
}

}  // namespace

int symsync_design(size_t k, size_t npfb, const float *h, size_t h_len, std::vector<float> &taps, size_t *Ls_) {
    if (k < 2) return fail(YAGI_ERR_CONFIG, "samples/symbol must be at least 2");
    if (npfb == 0) return fail(YAGI_ERR_CONFIG, "number of filters must be greater than 0");
    if (h_len == 0) return fail(YAGI_ERR_CONFIG, "filter length must be greater than 0");
    if ((h_len - 1) % npfb != 0) return fail(YAGI_ERR_CONFIG, "filter length must be of the form: h_len = m*k + 1");
    if (!h) return fail(YAGI_ERR_CONFIG, "null pointer argument");
    const size_t Ls = h_len / npfb;
    if (k > ((size_t)1 << 20) || npfb > (size_t)YAGI_SYMSYNC_NPFB_MAX || Ls == 0 || Ls > (size_t)YAGI_SYMSYNC_LS_MAX ||
        h_len < 2)
        return fail(YAGI_ERR_CONFIG, "symsync: (k, npfb, taps per branch) = (%zu, %zu, %zu) out of range", k, npfb, Ls);
    std::vector<float> dh(h_len);
    float hdh_max = 0.0f;
    for (size_t i = 0; i < h_len; ++i) {
        if (i == 0) dh[i] = h[i + 1] - h[h_len - 1];
        else if (i == h_len - 1) dh[i] = h[0] - h[i - 1];
        else dh[i] = h[i + 1] - h[i - 1];
        if (std::fabs(h[i] * dh[i]) > hdh_max || i == 0) hdh_max = std::fabs(h[i] * dh[i]);
    }
    if (!std::isfinite(hdh_max) || hdh_max == 0.0f)
        return fail(YAGI_ERR_CONFIG, "symsync: max |h dh| must be finite and greater than zero");
    const float g = 0.06f / hdh_max;
    for (size_t i = 0; i < h_len; ++i) dh[i] *= g;
    taps.assign(npfb * Ls * 2, 0.0f);
    for (size_t b = 0; b < npfb; ++b)
        for (size_t n = 0; n < Ls; ++n) {                   // firpfb.rs:45-51: rows reversed
            const size_t e = (b * Ls + (Ls - n - 1)) * 2;
            taps[e] = h[b + n * npfb];
            taps[e + 1] = dh[b + n * npfb];
        }
    *Ls_ = Ls;
    return YAGI_OK;
}

int symsync_set_bw(float bw, SymsyncLoop *p) {
    if (!(bw >= 0.0f && bw <= 1.0f)) return fail(YAGI_ERR_CONFIG, "bandwidth must be in [0,1]");
    const float alpha = 1.0f - bw, beta = 0.22f * bw, a = 0.5f, b = 0.495f;
    const float bc[3] = {beta, 0.0f, 0.0f}, ac[3] = {1.0f - a * alpha, -b * alpha, 0.0f};
    const float a0 = ac[0];
    p->b0 = bc[0] / a0;
    p->b1 = bc[1] / a0;
    p->b2 = bc[2] / a0;
    p->a1 = ac[1] / a0;
    p->a2 = ac[2] / a0;
    p->rate_adj = 0.5f * bw;
    return YAGI_OK;
}

void symsync_reset_chan(SymsyncChan *s, size_t k, size_t k_out) {
    *s = SymsyncChan{};
    s->rate = (float)k / (float)k_out;
    s->del = s->rate;
}

int launch_symsync(const SymsyncLoop &p, const float *taps, SymsyncChan *state, cf32 *hist, size_t C, const cf32 *x,
                   size_t x_pitch, size_t n, cf32 *y, size_t y_pitch, size_t ycap, unsigned *status, hipStream_t st) {
    SsArgs a{};
    a.p = p;
    a.taps = reinterpret_cast<const SsTap *>(taps);
    a.state = state, a.hist = hist, a.x = x, a.y = y, a.status = status;
    a.C = C, a.x_pitch = x_pitch, a.y_pitch = y_pitch;
    a.n = (unsigned)n, a.ycap = (unsigned)ycap;
    a.zero = 0.0;
    const size_t ring = symsync_ring_bytes(p.Ls), both = ring + symsync_table_bytes(p.npfb, p.Ls);
    const bool lds_taps = both + symsync_stage_bytes() <= kSymsyncLdsMax;
    const size_t need = (lds_taps ? both : ring) + symsync_stage_bytes();
    return bank_launch(lds_taps ? symsync_crcf_kernel<true> : symsync_crcf_kernel<false>, C, kSymsyncWg, kSymsyncWg, need, st, a);
}

void symsync_host(const SymsyncLoop &p, const float *taps_, SymsyncChan *state, cf32 *hist, size_t C, const cf32 *x,
                  size_t x_pitch, size_t n, cf32 *y, size_t y_pitch, size_t ycap, unsigned *ny_, unsigned *stalled) {
    const SsTap *taps = reinterpret_cast<const SsTap *>(taps_);
    const unsigned Ls = p.Ls;
    std::vector<cf32> ring(Ls);
    for (size_t c = 0; c < C; ++c) {
        SymsyncChan s = state[c];
        unsigned ny = 0;
        if (!s.stalled) {
            Ring<cf32> win{ring.data(), 1, Ls, 0};
            win.fill(hist, C, c);
            auto full = [&] { return ny >= ycap; };
            auto emit = [&](cf32 yv) {
                y[(size_t)ny * y_pitch + c] = yv;
                ++ny;
                return 0u;
            };
            for (size_t step = 0; step < n && !s.stalled; ++step)
                ss_row(s, p, win, taps, x[step * x_pitch + c], s.stalled, 1u, ycap - ny, 0.0, [](bool m) { return m; }, full, emit,
                       [] {});
            win.store(hist, C, c);
            state[c] = s;
        }
        ny_[c] = ny;
        stalled[c] = s.stalled;
    }
}

}  // namespace yagi
