// convcode_kernels.hip -- ConvCode: convolutional encoder and Viterbi decoder for a bank of frames (yagi_hip.h).
//
// Everything is integer arithmetic, so every arrangement below gives the definition's words exactly.
//
// conv_encode_kernel: one lane per trellis step of a frame.  The shift register at step t is a K-bit window of the
// message bits, so there is no recurrence; the punctured write index comes from the per-period table (kernels.hpp).
//
// conv_decode_kernel<SPL, WIDE>: the trellis is serial along time and parallel across states and frames.  A lane holds SPL =
// max(1, S / 64) path metrics in registers; for S < 64 a wave holds fpw frames side by side, lane = frame S + state.
// Per step the two predecessor metrics come through ds_bpermute; the branch cost is a byte select between two
// expanded words and one v_sad_u8 that also adds the predecessor's metric; the survivor decisions of the step are the
// ballot of the compare, whose bit fields belong to the wave's frames, stored to the wave's decision array in LDS by
// lane 0 (or, where a step's decisions are fewer than 8 bytes, one byte per lane).
//
// Soft bytes are staged per wave, chunk = kConvStage / fpw steps at a time: first the aligned 4-byte words that hold a
// frame's bytes of the chunk (coalesced), then one lane per (frame, step) expands them through the puncture table into two
// words, A0 = the costs of the R outputs where the branch bit is 0 (s, or 0 where not kept) and A1 where it is 1
// (255 - s, or 0), a byte per output.  A lane's cost is then the bytes of A1 under its branch mask, those of A0 elsewhere.
//
// Traceback: lane j of a wave walks frame j's decisions in LDS from the end state, assembles the message bytes in a
// register and stores one per 8 steps, then the metric.  No scratch (tests/test_convcode_isa_cpu.py).
//
// The host forms are the definition's sequential loops and share nothing with the kernels but the table.
#include <vector>

#include "kernels.hpp"

namespace yagi {
namespace {

constexpr int kConvEncWg = 256;

__host__ __device__ inline unsigned cv_parity(unsigned v) { return (unsigned)__builtin_popcount(v) & 1u; }

struct ConvEncArgs {
    const uint32_t *tab;
    const uint8_t *msg;
    uint8_t *coded;
    size_t msg_pitch, coded_pitch;
    unsigned n, T, tiles, K, R, p, kp, g0, g1, g2, g3;
};

__global__ __launch_bounds__(kConvEncWg) void conv_encode_kernel(const ConvEncArgs a) {
    __shared__ uint32_t tab[kConvTableWords];
    if (threadIdx.x < kConvTableWords) tab[threadIdx.x] = a.tab[threadIdx.x];
    __syncthreads();
    const unsigned f = blockIdx.x / a.tiles, t = (blockIdx.x % a.tiles) * kConvEncWg + threadIdx.x;
    if (t >= a.T) return;
    const uint8_t *m = a.msg + (size_t)f * a.msg_pitch;
    unsigned sr = 0;                                        // bit k is message bit t - k; zero before the frame and in its tail
    for (unsigned k = 0; k < a.K; ++k)
        if (t >= k && t - k < a.n) {
            const unsigned i = t - k;
            sr |= ((m[i >> 3] >> (7u - (i & 7u))) & 1u) << k;
        }
    const unsigned j = t % a.p, q = t / a.p;
    const uint32_t off = tab[j], keep = tab[YAGI_CONVCODE_PERIOD_MAX + j];
    uint8_t *c = a.coded + (size_t)f * a.coded_pitch + (size_t)q * a.kp;
    const unsigned g[4] = {a.g0, a.g1, a.g2, a.g3};
#pragma unroll
    for (unsigned r = 0; r < 4; ++r)
        if ((keep >> r) & 1u) c[(off >> (8 * r)) & 0xffu] = (uint8_t)cv_parity(sr & g[r]);
}

struct ConvDecArgs {
    const uint32_t *tab;
    const uint8_t *soft;
    uint8_t *msg;
    uint32_t *metric;
    size_t soft_pitch, msg_pitch;
    unsigned n, T, F, K, R, p, kp, terminated, lg_fpw, W, dec_bytes, wave_bytes, g0, g1, g2, g3;
};

__device__ __forceinline__ unsigned cv_bperm(unsigned byte_addr, unsigned v) {
    return (unsigned)__builtin_amdgcn_ds_bpermute((int)byte_addr, (int)v);
}

// WIDE: a wave's step is whole 8-byte ballots (fpw S = 64 lanes, or SPL of them); else W = fpw S / 8 < 8 bytes
template <int SPL, bool WIDE>
__global__ __launch_bounds__(256) void conv_decode_kernel(const ConvDecArgs a) {
    extern __shared__ __align__(16) unsigned char cv_smem[];
    uint32_t *tab = reinterpret_cast<uint32_t *>(cv_smem);
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (unsigned e = tid; e < kConvTableWords; e += blockDim.x) tab[e] = a.tab[e];

    const unsigned K = a.K, S = 1u << (K - 1), fpw = 1u << a.lg_fpw, lg_ch = 8u - a.lg_fpw, CH = 1u << lg_ch, W = a.W;
    const unsigned T = a.T, p = a.p, kp = a.kp;
    unsigned char *dec = cv_smem + kConvTableWords * 4 + (size_t)wave * a.wave_bytes;
    uint2 *xs = reinterpret_cast<uint2 *>(dec + a.dec_bytes);          // [fpw][CH] expanded steps
    unsigned char *raw = reinterpret_cast<unsigned char *>(xs + kConvStage);
    const unsigned rawpitch = CH * 4 + 8;
    const size_t f0 = ((size_t)blockIdx.x * (blockDim.x >> 6) + wave) * fpw;     // the wave's first frame

    // the lane's states: SPL == 1: state s of frame grp; else states lane + 64 q of the wave's one frame
    const unsigned grp = SPL == 1 ? lane >> (K - 1) : 0u, s = lane & (S - 1);
    const unsigned gc = grp < fpw ? grp : fpw - 1;          // lanes beyond the wave's frames follow the last one; never stored
    const unsigned g[4] = {a.g0, a.g1, a.g2, a.g3};
    unsigned mm0[SPL], mm1[SPL], pm[SPL], src[SPL];
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
        const unsigned ns = SPL == 1 ? s : (unsigned)q * 64u + lane;
        mm0[q] = mm1[q] = 0;
#pragma unroll
        for (unsigned r = 0; r < 4; ++r)
            if (r < a.R) {
                const unsigned e0 = cv_parity(ns & g[r]), e1 = e0 ^ ((g[r] >> (K - 1)) & 1u);   // ((p << 1) | b) = ns, ns | 2^(K-1)
                mm0[q] |= e0 ? 0xffu << (8 * r) : 0u;
                mm1[q] |= e1 ? 0xffu << (8 * r) : 0u;
            }
        pm[q] = ns == 0 ? 0u : 1u << 30;
        // p0 = ns >> 1 sits in lane (grp S + (s >> 1)), or in slot q >> 1 at lane ((q & 1) << 5 | lane >> 1)
        src[q] = 4u * (SPL == 1 ? (grp << (K - 1)) + (s >> 1) : (((unsigned)q & 1u) << 5) | (lane >> 1));
    }
    const unsigned half = SPL == 1 ? 4u * (S >> 1) : 0u;    // p1 = p0 | 2^(K-2): S / 2 lanes on, or SPL / 2 slots on

#pragma unroll 1
    for (unsigned t0 = 0; t0 < T; t0 += CH) {
        const unsigned cn = T - t0 < CH ? T - t0 : CH, t1 = t0 + cn;
        __syncthreads();                                    // the table is in place; every lane is done with the last chunk
        const unsigned pos0 = t0 / p * kp + (tab[t0 % p] & 0xffu), len = t1 / p * kp + (tab[t1 % p] & 0xffu) - pos0;
        for (unsigned gi = 0; gi < fpw && f0 + gi < a.F; ++gi) {
            const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.soft + (f0 + gi) * a.soft_pitch + pos0);
            const uint32_t *from = reinterpret_cast<const uint32_t *>(a0 & ~(uintptr_t)3);
            const unsigned nd = ((unsigned)(a0 & 3) + len + 3u) >> 2;              // <= CH + 1 words
            uint32_t *to = reinterpret_cast<uint32_t *>(raw + gi * rawpitch);
            for (unsigned i = lane; i < nd; i += 64) to[i] = from[i];
        }
        __syncthreads();
        for (unsigned e = lane; e < kConvStage; e += 64) {
            const unsigned gi = e >> lg_ch, tl = e & (CH - 1);
            if (tl < cn && f0 + gi < a.F) {
                const unsigned t = t0 + tl, j = t % p, off = tab[j], keep = tab[YAGI_CONVCODE_PERIOD_MAX + j];
                const unsigned head = (unsigned)(reinterpret_cast<uintptr_t>(a.soft + (f0 + gi) * a.soft_pitch + pos0) & 3);
                const unsigned base = t / p * kp - pos0 + head;     // wraps where the period began before the chunk
                const unsigned char *rb = raw + gi * rawpitch;
                unsigned A0 = 0, A1 = 0;
#pragma unroll
                for (unsigned r = 0; r < 4; ++r)
                    if ((keep >> r) & 1u) {
                        const unsigned sv = rb[base + ((off >> (8 * r)) & 0xffu)];
                        A0 |= sv << (8 * r);
                        A1 |= (255u - sv) << (8 * r);
                    }
                xs[e] = make_uint2(A0, A1);
            }
        }
        __syncthreads();

        const uint2 *xg = xs + (gc << lg_ch);
        const auto forward = [&](unsigned tl) {             // one trellis step of the wave's frames
            const uint2 A = xg[tl];
            unsigned nm[SPL];
            unsigned long long w[SPL];
#pragma unroll
            for (int q = 0; q < SPL; ++q) {
                const unsigned o0 = cv_bperm(src[q], pm[SPL == 1 ? 0 : q >> 1]);
                const unsigned o1 = cv_bperm(src[q] + half, pm[SPL == 1 ? 0 : (q >> 1) + SPL / 2]);
                const unsigned m0 = __builtin_amdgcn_sad_u8((A.y & mm0[q]) | (A.x & ~mm0[q]), 0u, o0);
                const unsigned m1 = __builtin_amdgcn_sad_u8((A.y & mm1[q]) | (A.x & ~mm1[q]), 0u, o1);
                const bool d = m1 < m0;                     // strict: a tie keeps p0
                nm[q] = d ? m1 : m0;
                w[q] = __ballot(d);
            }
            const unsigned t = t0 + tl;
#pragma unroll
            for (int q = 0; q < SPL; ++q) {
                pm[q] = nm[q];
                if (WIDE) {
                    if (lane == 0) *reinterpret_cast<unsigned long long *>(dec + ((size_t)t * SPL + q) * 8) = w[q];
                } else if (lane < W) {
                    dec[(size_t)t * W + lane] = (unsigned char)(w[q] >> (8 * (lane & 7u)));
                }
            }
        };
        unsigned tl = 0;
#pragma unroll 1
        for (; tl + 4 <= cn; tl += 4) {
#pragma unroll
            for (unsigned u = 0; u < 4; ++u) forward(tl + u);
        }
#pragma unroll 1
        for (; tl < cn; ++tl) forward(tl);
    }

    // the end state: 0 where terminated, else the smallest metric, the lowest index on a tie
    unsigned long long key = ~0ull;
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
        const unsigned ns = SPL == 1 ? s : (unsigned)q * 64u + lane;
        const unsigned long long k = ((unsigned long long)pm[q] << 8) | ns;
        if ((!a.terminated || ns == 0) && k < key) key = k;
    }
    for (unsigned m = 1; m < (S < 64u ? S : 64u); m <<= 1) {
        const unsigned lo = __shfl_xor((unsigned)key, (int)m), hi = __shfl_xor((unsigned)(key >> 32), (int)m);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        if (o < key) key = o;
    }
    const int from = SPL == 1 && lane < fpw ? (int)(lane << (K - 1)) : 0;
    const unsigned klo = __shfl((unsigned)key, from), khi = __shfl((unsigned)(key >> 32), from);
    __syncthreads();                                        // the decisions of every lane are in LDS

    if (lane < fpw && f0 + lane < a.F) {
        const size_t f = f0 + lane;
        const unsigned gb = SPL == 1 ? lane << (K - 1) : 0u;
        unsigned e = klo & 0xffu, acc = 0, t = T;
        uint8_t *out = a.msg + f * a.msg_pitch;
        const auto back = [&](unsigned tt) {                // e = the state before step tt
            const unsigned bit = gb + e;
            const unsigned d = ((unsigned)dec[(size_t)tt * W + (bit >> 3)] >> (bit & 7u)) & 1u;
            e = (e >> 1) | (d << (K - 2));
        };
#pragma unroll 1
        while (t > a.n) back(--t);                          // the tail carries no message bit
#pragma unroll 1
        while (t & 7u) {                                    // the last byte where it is partial: pad bits stay zero
            --t;
            acc |= (e & 1u) << (7u - (t & 7u));
            back(t);
        }
        if (a.n & 7u) out[a.n >> 3] = (uint8_t)acc;
#pragma unroll 1
        while (t > 0) {                                     // whole bytes: bit t = e & 1 goes to position 7 - (t & 7)
            acc = 0;
#pragma unroll
            for (unsigned k = 0; k < 8; ++k) {
                --t;
                acc |= (e & 1u) << k;
                back(t);
            }
            out[t >> 3] = (uint8_t)acc;
        }
        if (a.metric) a.metric[f] = (klo >> 8) | (khi << 24);
    }
}

template <int SPL, bool WIDE>
int conv_decode_launch(const ConvDecArgs &a, unsigned blocks, unsigned waves, size_t lds, hipStream_t st) {
    auto fn = conv_decode_kernel<SPL, WIDE>;
    if (lds > 64 * 1024)
        YG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kConvLdsMax));
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(64 * waves), lds, st, a);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

}  // namespace

bool conv_shape_ok(int K, ConvShape s) {
    const bool fpw_ok = s.fpw >= conv_fpw_min(K) && s.fpw <= conv_fpw_max(K) && (s.fpw & (s.fpw - 1)) == 0;
    return fpw_ok && (s.waves == 1 || s.waves == 2 || s.waves == 4);
}

// Set from profiles/r27_kbench_convcode.txt ("ConvCode").  As many frames per wave as the states leave
// lanes for, halved (1) while the decisions of the wave's frames leave fewer than 8 waves resident on a CU: the frames a CU
// holds are set by their decision bytes either way, and more waves hide the latency of the serial chain better; (2) while
// the bank gives fewer than two waves to each of the chip's 1024 SIMDs.  Then 2 or 4 waves per workgroup while the bank
// has frames for them and the allocation stays under 64 KiB, so that at least two workgroups share a CU (the number of
// waves moves a call by 0 to 16 %, without a pattern a rule could follow).
ConvShape conv_plan(int K, size_t T, size_t F) {
    ConvShape s{conv_fpw_max(K), 1};
    const auto resident = [&](ConvShape v) { return kConvLdsMax / conv_lds_bytes(K, v, T); };
    while (s.fpw > conv_fpw_min(K) && (resident(s) < 8 || (F + s.fpw - 1) / s.fpw < 2048)) s.fpw /= 2;
    while (s.waves < 4 && (size_t)s.fpw * s.waves < F && conv_lds_bytes(K, ConvShape{s.fpw, s.waves * 2}, T) <= 64 * 1024)
        s.waves *= 2;
    return s;
}

void conv_table(const ConvCode &c, uint32_t *words) {
    for (int j = 0; j < YAGI_CONVCODE_PERIOD_MAX; ++j) {
        words[j] = c.off[j];
        words[YAGI_CONVCODE_PERIOD_MAX + j] = c.keep[j];
    }
}

int launch_conv_encode(const ConvCode &c, const uint32_t *tab, const uint8_t *msg, size_t msg_pitch, size_t n, size_t F,
                       uint8_t *coded, size_t coded_pitch, hipStream_t st) {
    if (F == 0) return YAGI_OK;
    if (n == 0 || n > c.nmax() || F > (size_t)YAGI_CONVCODE_FRAMES_MAX) return fail(YAGI_ERR_CONFIG, "convcode: bad launch");
    ConvEncArgs a{};
    a.tab = tab, a.msg = msg, a.coded = coded, a.msg_pitch = msg_pitch, a.coded_pitch = coded_pitch;
    a.n = (unsigned)n, a.T = (unsigned)c.steps(n), a.tiles = (a.T + kConvEncWg - 1) / kConvEncWg;
    a.K = (unsigned)c.K, a.R = (unsigned)c.R, a.p = (unsigned)c.p, a.kp = c.kp;
    a.g0 = c.g[0], a.g1 = c.g[1], a.g2 = c.g[2], a.g3 = c.g[3];
    hipLaunchKernelGGL(conv_encode_kernel, dim3((unsigned)(F * a.tiles)), dim3(kConvEncWg), 0, st, a);   // <= 2^20 x 2^8
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

int launch_conv_decode(const ConvCode &c, ConvShape s, const uint32_t *tab, const uint8_t *soft, size_t soft_pitch, size_t n,
                       size_t F, uint8_t *msg, size_t msg_pitch, uint32_t *metric, hipStream_t st) {
    if (F == 0) return YAGI_OK;
    if (n == 0 || n > c.nmax() || F > (size_t)YAGI_CONVCODE_FRAMES_MAX) return fail(YAGI_ERR_CONFIG, "convcode: bad launch");
    if (!conv_shape_ok(c.K, s))
        return fail(YAGI_ERR_CONFIG, "convcode: the shape (%u frames per wave, %u waves) is not admissible at K = %d", s.fpw, s.waves, c.K);
    const size_t T = c.steps(n), lds = conv_lds_bytes(c.K, s, T);
    if (lds > kConvLdsMax)
        return fail(YAGI_ERR_CONFIG, "convcode: %u frames per wave and %u waves of %zu steps need %zu bytes of LDS", s.fpw, s.waves, T, lds);
    ConvDecArgs a{};
    a.tab = tab, a.soft = soft, a.msg = msg, a.metric = metric, a.soft_pitch = soft_pitch, a.msg_pitch = msg_pitch;
    a.n = (unsigned)n, a.T = (unsigned)T, a.F = (unsigned)F, a.K = (unsigned)c.K, a.R = (unsigned)c.R, a.p = (unsigned)c.p;
    a.kp = c.kp, a.terminated = c.terminated ? 1u : 0u;
    while ((1u << a.lg_fpw) < s.fpw) ++a.lg_fpw;
    a.W = (unsigned)conv_step_bytes(c.K, s);
    a.dec_bytes = (unsigned)((T * a.W + 7) & ~(size_t)7);
    a.wave_bytes = (unsigned)conv_wave_bytes(c.K, s, T);
    a.g0 = c.g[0], a.g1 = c.g[1], a.g2 = c.g[2], a.g3 = c.g[3];
    const size_t per_wg = (size_t)s.fpw * s.waves;
    const unsigned blocks = (unsigned)((F + per_wg - 1) / per_wg);
    switch (conv_spl(c.K)) {
        case 1: return a.W >= 8 ? conv_decode_launch<1, true>(a, blocks, s.waves, lds, st)
                                : conv_decode_launch<1, false>(a, blocks, s.waves, lds, st);
        case 2: return conv_decode_launch<2, true>(a, blocks, s.waves, lds, st);
        default: return conv_decode_launch<4, true>(a, blocks, s.waves, lds, st);
    }
}

// ---- the definition on the host -------------------------------------------------------------------------------------
void conv_encode_host(const ConvCode &c, const uint8_t *msg, size_t msg_pitch, size_t n, size_t F, uint8_t *coded,
                      size_t coded_pitch) {
    const size_t T = c.steps(n);
    const unsigned mask = (1u << c.K) - 1;
    for (size_t f = 0; f < F; ++f) {
        const uint8_t *m = msg + f * msg_pitch;
        uint8_t *out = coded + f * coded_pitch;
        unsigned sr = 0;
        size_t w = 0;
        for (size_t t = 0; t < T; ++t) {
            const unsigned b = t < n ? (m[t >> 3] >> (7 - (t & 7))) & 1u : 0u;
            sr = ((sr << 1) | b) & mask;
            for (int r = 0; r < c.R; ++r)
                if ((c.keep[t % (size_t)c.p] >> r) & 1u) out[w++] = (uint8_t)cv_parity(sr & c.g[r]);
        }
    }
}

void conv_decode_host(const ConvCode &c, const uint8_t *soft, size_t soft_pitch, size_t n, size_t F, uint8_t *msg,
                      size_t msg_pitch, uint32_t *metric) {
    const size_t T = c.steps(n), S = c.states();
    std::vector<uint8_t> d(T * S);
    std::vector<uint32_t> pm(S), nx(S);
    for (size_t f = 0; f < F; ++f) {
        const uint8_t *in = soft + f * soft_pitch;
        size_t rd = 0;
        pm.assign(S, 1u << 30);
        pm[0] = 0;
        for (size_t t = 0; t < T; ++t) {
            unsigned sv[4] = {0, 0, 0, 0};
            const unsigned keep = c.keep[t % (size_t)c.p];
            for (int r = 0; r < c.R; ++r)
                if ((keep >> r) & 1u) sv[r] = in[rd++];
            for (size_t ns = 0; ns < S; ++ns) {
                const unsigned b = (unsigned)ns & 1u, p0 = (unsigned)ns >> 1, p1 = p0 | (1u << (c.K - 2));
                uint32_t c0 = 0, c1 = 0;
                for (int r = 0; r < c.R; ++r)
                    if ((keep >> r) & 1u) {
                        c0 += cv_parity(((p0 << 1) | b) & c.g[r]) ? 255u - sv[r] : sv[r];
                        c1 += cv_parity(((p1 << 1) | b) & c.g[r]) ? 255u - sv[r] : sv[r];
                    }
                const uint32_t m0 = pm[p0] + c0, m1 = pm[p1] + c1;
                d[t * S + ns] = m1 < m0;
                nx[ns] = m1 < m0 ? m1 : m0;
            }
            pm.swap(nx);
        }
        size_t e = 0;
        if (!c.terminated)
            for (size_t s = 1; s < S; ++s)
                if (pm[s] < pm[e]) e = s;
        if (metric) metric[f] = pm[e];
        uint8_t *out = msg + f * msg_pitch;
        for (size_t i = 0; i < (n + 7) / 8; ++i) out[i] = 0;
        for (size_t t = T; t-- > 0;) {
            if (t < n) out[t >> 3] |= (uint8_t)((e & 1u) << (7 - (t & 7)));
            e = (e >> 1) | ((size_t)d[t * S + e] << (c.K - 2));
        }
    }
}

}  // namespace yagi
