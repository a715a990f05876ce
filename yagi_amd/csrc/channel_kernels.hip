// channel_kernels.hip -- Channel: multipath, carrier offset and AWGN for a bank of independent links (yagi_hip.h).
//
// Per link the chain is an L-tap cccf inner product over a window, Osc's mix_up at phase theta + (u32)j d_theta, then
// y = w gamma + nstd n(seed, link, t + j).  Nothing feeds back along time, so the grid runs over tiles of links x steps
// and every output is whole in one lane, in the definition's order: the lane arrangement cannot change a word.
//
// channel_kernel<VCO, BCAST>: a workgroup of 256 lanes is cw links wide and 256 / cw steps deep (cw a power of two up to
// 64, so a single link and a wide bank both use every lane); a lane writes `rows` outputs, 256 / cw steps apart, so a
// wave's stores of one round are cw adjacent links of 64 / cw adjacent rows.  LDS holds Osc's table (8 KiB NCO, 16 KiB
// VCO), the tile's taps [L][cw] and its input rows [tile_steps + L - 1][cw]; rows before the call come from the carried
// window, loads are coalesced across links.  The broadcast form stages one row of tile_steps + L - 1 samples for all
// its links, plus the links' carried windows [L - 1][cw] in the tiles that still reach before the call.  The inner
// product reads LDS at consecutive 8-byte words across the links of a row (no bank conflict) and the taps likewise.
//
// The window the call leaves (its last L - 1 inputs per link, older ones from the old window where n < L - 1) goes to a
// second buffer that the host swaps in, written by the workgroups of the last step tile, so no workgroup of the launch
// reads what another writes.  The oscillator phase and the noise counter are closed forms of the sample index: the
// host advances them at the call.  A launch holds at most kChannelGridMax workgroups; where a call has more tiles a
// workgroup takes several step tiles of its links in turn.  No scratch, no f32 FMA (tests/test_channel_isa_cpu.py).
//
// The host form and the array forms of the words live here too: host.cpp and capi.hip are built with contraction on.
#pragma clang fp contract(off)

#include <cmath>
#include <vector>

#include "channel_body.hpp"
#include "channel_words.hpp"
#include "kernels.hpp"

namespace yagi {
namespace {

typedef float ch_v2f __attribute__((ext_vector_type(2)));

struct ChannelArgs {
    const void *osc_tab;
    const ChannelLink *link;
    const cf32 *taps, *win, *x;
    cf32 *win_next, *y;
    size_t C, x_pitch, y_pitch;
    unsigned long long seed, adv;
    unsigned n, L, lg_cw, rows, link_tiles, step_tiles, step_slots;
};

template <int VCO, bool BCAST>
__global__ __launch_bounds__(kChannelWg) void channel_kernel(const ChannelArgs a) {
    using E = typename OscEntry<VCO>::E;
    extern __shared__ __align__(16) unsigned char ch_smem[];
    E *tab = reinterpret_cast<E *>(ch_smem);
    cf32 *taps = reinterpret_cast<cf32 *>(tab + 1024);
    const unsigned tid = threadIdx.x, L = a.L, H = L - 1, n = a.n;
    const unsigned cw = 1u << a.lg_cw, depth = kChannelWg >> a.lg_cw, ts = depth * a.rows;
    cf32 *xs = taps + (size_t)L * cw;                       // BCAST: [ts + H]; else [ts + H][cw]
    cf32 *halo = xs + ts + H;                               // BCAST only: [H][cw]
    const E *tg = static_cast<const E *>(a.osc_tab);
    for (unsigned e = tid; e < 1024u; e += kChannelWg) tab[e] = tg[e];

    // a launch holds at most kChannelGridMax workgroups: beyond that a workgroup takes several step tiles in turn
    const unsigned lt = blockIdx.x % a.link_tiles, st0 = blockIdx.x / a.link_tiles;
    const size_t c0 = (size_t)lt * cw;
    for (unsigned e = tid; e < L * cw; e += kChannelWg) {
        const size_t c = c0 + (e & (cw - 1));
        taps[e] = c < a.C ? a.taps[(size_t)(e >> a.lg_cw) * a.C + c] : cf32{0.0f, 0.0f};
    }
#pragma unroll 1
    for (unsigned st = st0; st < a.step_tiles; st += a.step_slots) {
        if (st != st0) __syncthreads();                         // every lane is done with the previous tile's LDS
        const unsigned t0 = st * ts;                            // t0 < n < 2^31
        const bool before = t0 < H;                             // the tile reaches before the call: the carried window
        // local row i is step t0 - H + i of the call
        if (BCAST) {
            for (unsigned i = tid; i < ts + H; i += kChannelWg) {
                const long long s = (long long)t0 - H + i;
                xs[i] = s >= 0 && s < (long long)n ? a.x[s] : cf32{0.0f, 0.0f};
            }
            if (before)
                for (unsigned e = tid; e < H * cw; e += kChannelWg) {
                    const size_t c = c0 + (e & (cw - 1));
                    halo[e] = c < a.C ? a.win[(size_t)(e >> a.lg_cw) * a.C + c] : cf32{0.0f, 0.0f};
                }
        } else {
            for (unsigned e = tid; e < (ts + H) * cw; e += kChannelWg) {
                const unsigned i = e >> a.lg_cw;
                const size_t c = c0 + (e & (cw - 1));
                const long long s = (long long)t0 - H + i;
                cf32 v{0.0f, 0.0f};
                if (c < a.C) {
                    if (s < 0) v = a.win[(size_t)(s + H) * a.C + c];
                    else if (s < (long long)n) v = a.x[(size_t)s * a.x_pitch + c];
                }
                xs[e] = v;
            }
        }
        __syncthreads();

        const unsigned lc = tid & (cw - 1), ls = tid >> a.lg_cw;
        const size_t c = c0 + lc;
        if (c < a.C) {
            const ChannelLink k = a.link[c];
            const uint64_t seed_c = splitmix64_at(a.seed, c);
            for (unsigned r = 0; r < a.rows; ++r) {
                const unsigned sl = ls + r * depth, s = t0 + sl;
                if (s >= n) break;
                float2 v;
                if (!BCAST) {
                    v = channel_fir(taps + lc, cw, xs + (size_t)sl * cw + lc, cw, L);
                } else if (!before || s >= H) {                 // the whole window lies inside the call
                    v = channel_fir(taps + lc, cw, xs + sl, 1, L);
                } else {                                        // window entry j is step s - H + j
                    float ar = 0.0f, ai = 0.0f;
                    for (unsigned j = 0; j < L; ++j) {
                        const cf32 hv = taps[(size_t)j * cw + lc];
                        const cf32 xv = s + j < H ? halo[(size_t)(s + j) * cw + lc] : xs[sl + j];
                        const float rr = hv.re * xv.re, ii = hv.im * xv.im, ri = hv.re * xv.im, ir = hv.im * xv.re;
                        const float pr = rr - ii, pi = ri + ir;
                        ar = ar + pr;
                        ai = ai + pi;
                    }
                    v = make_float2(ar, ai);
                }
                const cf32 y = channel_finish<VCO>(tab, k, seed_c, a.adv + s, v);
                __builtin_nontemporal_store(ch_v2f{y.re, y.im}, reinterpret_cast<ch_v2f *>(a.y + (size_t)s * a.y_pitch + c));
            }
        }

        // the window the call leaves: entry i is step n - H + i, from the old window where that is before the call
        if (t0 + ts >= n) {
            for (unsigned e = tid; e < H * cw; e += kChannelWg) {
                const unsigned i = e >> a.lg_cw;
                const size_t cc = c0 + (e & (cw - 1));
                if (cc >= a.C) continue;
                const long long s = (long long)n - H + i;
                a.win_next[(size_t)i * a.C + cc] = s < 0 ? a.win[(size_t)(s + H) * a.C + cc]
                                                          : (BCAST ? a.x[s] : a.x[(size_t)s * a.x_pitch + cc]);
            }
        }
    }
}

template <int VCO, bool BCAST>
int channel_launch(const ChannelArgs &a, size_t lds, hipStream_t st) {
    auto fn = channel_kernel<VCO, BCAST>;
    if (lds > 64 * 1024)
        YG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(fn, dim3(a.link_tiles * a.step_slots), dim3(kChannelWg), lds, st, a);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

}  // namespace

bool channel_shape_ok(ChannelShape s) {
    const bool cw_ok = s.cw >= 1 && s.cw <= 64 && (s.cw & (s.cw - 1)) == 0;
    const bool rows_ok = s.rows >= 1 && s.rows <= kChannelRowsMax && (s.rows & (s.rows - 1)) == 0;
    return cw_ok && rows_ok;
}

// The arrangement measured fastest, or within 2 % of it, at every shape of tools/kb_channel.py (DESIGN section 4,
// "Channel").  Eight outputs per lane.  The row is as wide as the bank (the next power of two >= C, up to 64), narrowed
// until the workgroup is at least twice as deep as the taps are long (256 / cw >= 2 L) but not below 8 links, the 64
// contiguous bytes of a row that keep the loads and stores whole: the tile is then many times the halo and its LDS
// stays near 28 KiB, so several workgroups share a CU, which counted for more than wide rows (at L = 32, 8 links x 256
// steps ran twice as fast as 64 links x 64 steps).  A call shorter than the tile takes fewer outputs per lane.
ChannelShape channel_plan(size_t C, size_t L, size_t n) {
    ChannelShape s{1, 1};
    while (s.cw < 64 && s.cw < C) s.cw *= 2;
    while (s.cw > 8 && kChannelWg / s.cw < 2 * L) s.cw /= 2;
    const size_t depth = kChannelWg / s.cw;
    while (s.rows < 8 && depth * s.rows < n) s.rows *= 2;
    return s;
}

int launch_channel(ChannelShape s, int vco, bool bcast, const void *osc_tab, const ChannelLink *link, const cf32 *taps,
                   const cf32 *win, cf32 *win_next, uint64_t seed, uint64_t adv, size_t C, size_t L, const cf32 *x,
                   size_t x_pitch, size_t n, cf32 *y, size_t y_pitch, hipStream_t st) {
    if (n == 0) return YAGI_OK;
    if (!channel_shape_ok(s)) return fail(YAGI_ERR_CONFIG, "channel: the shape (%u links, %u rows) is not admissible", s.cw, s.rows);
    if (L < 1 || L > (size_t)YAGI_CHANNEL_TAPS_MAX || n >= ((size_t)1 << 31)) return fail(YAGI_ERR_CONFIG, "channel: bad launch");
    const size_t ts = channel_tile_steps(s);
    const size_t link_tiles = (C + s.cw - 1) / s.cw, step_tiles = (n + ts - 1) / ts;
    size_t slots = kChannelGridMax / link_tiles;              // link_tiles <= 2^20 = kChannelGridMax
    if (slots > step_tiles) slots = step_tiles;
    ChannelArgs a{};
    a.osc_tab = osc_tab, a.link = link, a.taps = taps, a.win = win, a.x = x, a.win_next = win_next, a.y = y;
    a.C = C, a.x_pitch = x_pitch, a.y_pitch = y_pitch, a.seed = seed, a.adv = adv;
    a.n = (unsigned)n, a.L = (unsigned)L, a.rows = s.rows, a.link_tiles = (unsigned)link_tiles, a.step_tiles = (unsigned)step_tiles, a.step_slots = (unsigned)slots;
    while ((1u << a.lg_cw) < s.cw) ++a.lg_cw;
    const size_t lds = channel_lds_bytes(s, L, vco, bcast);
    if (vco) return bcast ? channel_launch<1, true>(a, lds, st) : channel_launch<1, false>(a, lds, st);
    return bcast ? channel_launch<0, true>(a, lds, st) : channel_launch<0, false>(a, lds, st);
}

namespace {
template <int VCO>
void channel_host_t(bool bcast, const void *osc_tab, const ChannelLink *link, const cf32 *taps, uint64_t seed, size_t C,
                    size_t L, const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch) {
    using E = typename OscEntry<VCO>::E;
    const E *tab = static_cast<const E *>(osc_tab);
    std::vector<cf32> w(L - 1 + n, cf32{0.0f, 0.0f});       // the window's zeros, then the link's samples
    for (size_t c = 0; c < C; ++c) {
        for (size_t s = 0; s < n; ++s) w[L - 1 + s] = bcast ? x[s] : x[s * x_pitch + c];
        const uint64_t seed_c = splitmix64_at(seed, c);
        for (size_t s = 0; s < n; ++s) {
            const float2 v = channel_fir(taps + c, C, w.data() + s, 1, (unsigned)L);
            y[s * y_pitch + c] = channel_finish<VCO>(tab, link[c], seed_c, s, v);
        }
    }
}
}  // namespace

void channel_host(int vco, bool bcast, const void *osc_tab, const ChannelLink *link, const cf32 *taps, uint64_t seed, size_t C,
                  size_t L, const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch) {
    if (vco) channel_host_t<1>(bcast, osc_tab, link, taps, seed, C, L, x, x_pitch, n, y, y_pitch);
    else channel_host_t<0>(bcast, osc_tab, link, taps, seed, C, L, x, x_pitch, n, y, y_pitch);
}

void channel_awgn_words(float n0_db, float snr_db, float *gamma, float *nstd) {
    const float tn = n0_db / 20.0f, tg = (snr_db + n0_db) / 20.0f;
    *nstd = chan_p10(tn);
    *gamma = chan_p10(tg);
}
void channel_cos_sin_host(const uint32_t *k2, size_t n, double *c, double *s) {
    for (size_t i = 0; i < n; ++i) chan_cos_sin64(k2[i] & 0xffffffu, &c[i], &s[i]);
}
void channel_radius_host(const uint32_t *k1, size_t n, float *r) {
    for (size_t i = 0; i < n; ++i) r[i] = chan_radius(k1[i]);
}
void channel_noise_host(uint64_t seed, uint64_t link, uint64_t first, size_t n, cf32 *out) {
    const uint64_t seed_c = splitmix64_at(seed, link);
    for (size_t i = 0; i < n; ++i) chan_noise(seed_c, first + i, &out[i].re, &out[i].im);
}

}  // namespace yagi
