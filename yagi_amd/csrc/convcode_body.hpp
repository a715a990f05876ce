// convcode_body.hpp -- the Viterbi decoder of a wave's frames (convcode_kernels.hip describes the arrangement): the trellis
// step, the end-state search and the traceback of conv_decode_kernel as a body that leaves two things to the including
// kernel.  The Packetizer's decoder is built on it (packetizer_kernels.hip).  conv_decode_kernel itself keeps its own text
// for now: instantiated from this body with its word-staged source it computes the same bytes, but the compiler schedules
// it differently and it measured 0.5 to 2.4 % slower at K <= 7 (profiles/r28_convcode_unmoved.txt), and ConvCode may not
// move.  A change to the trellis step, the end-state search or the traceback goes into both.
//   Source  where a step's soft bytes come from.  stage(chunk) runs once per chunk on every lane, after the barrier that
//           ends the last chunk's reads (a word-staged source fills the wave's LDS behind xs there and ends with a barrier
//           of its own; the Packetizer does nothing); step(chunk, gi, t) says where the kept bytes of frame f0 + gi at step
//           t lie, and soft(at, o) returns the byte of the o-th kept bit of that step's period.  The one place that fills
//           xs[e] is here.
//   Sink    what the traceback lane of a frame does with the message: begin(f), then the bytes from the last to the first
//           (partial(i, v) for a last byte of fewer than 8 bits, byte(i, v) for whole ones, most significant bit first), then
//           end(f, metric).
#pragma once

#include "kernels.hpp"

namespace yagi {

__host__ __device__ inline unsigned cv_parity(unsigned v) { return (unsigned)__builtin_popcount(v) & 1u; }

struct ConvDecArgs {
    const uint32_t *tab;
    const uint8_t *soft;
    uint8_t *msg;
    uint32_t *metric;
    size_t soft_pitch, msg_pitch;
    unsigned n, T, F, K, R, p, kp, terminated, lg_fpw, W, dec_bytes, wave_bytes, g0, g1, g2, g3;
};

// what Source::stage sees of a chunk: steps t0 .. t1 - 1 of the frames f0 .. f0 + fpw - 1, whose kept bytes are the len
// coder-order positions from pos0 on; `after` is the wave's LDS behind its expanded steps
struct ConvChunk {
    unsigned t0, t1, pos0, len, lane, fpw, CH;
    size_t f0;
    unsigned char *after;
};

__device__ __forceinline__ unsigned cv_bperm(unsigned byte_addr, unsigned v) {
    return (unsigned)__builtin_amdgcn_ds_bpermute((int)byte_addr, (int)v);
}

// WIDE: a wave's step is whole 8-byte ballots (fpw S = 64 lanes, or SPL of them); else W = fpw S / 8 < 8 bytes
template <int SPL, bool WIDE, class Source, class Sink>
__device__ __forceinline__ void conv_decode_body(const ConvDecArgs &a, unsigned char *cv_smem, const unsigned nthreads, Source &source, Sink &sink) {
    uint32_t *tab = reinterpret_cast<uint32_t *>(cv_smem);
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (unsigned e = tid; e < kConvTableWords; e += nthreads) tab[e] = a.tab[e];

    const unsigned K = a.K, S = 1u << (K - 1), fpw = 1u << a.lg_fpw, lg_ch = 8u - a.lg_fpw, CH = 1u << lg_ch, W = a.W;
    const unsigned T = a.T, p = a.p, kp = a.kp;
    unsigned char *dec = cv_smem + kConvTableWords * 4 + (size_t)wave * a.wave_bytes;
    uint2 *xs = reinterpret_cast<uint2 *>(dec + a.dec_bytes);          // [fpw][CH] expanded steps
    const size_t f0 = ((size_t)blockIdx.x * (nthreads >> 6) + wave) * fpw;     // the wave's first frame

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
        const ConvChunk chunk{t0, t1, pos0, len, lane, fpw, CH, f0, reinterpret_cast<unsigned char *>(xs + kConvStage)};
        source.stage(chunk);
        for (unsigned e = lane; e < kConvStage; e += 64) {
            const unsigned gi = e >> lg_ch, tl = e & (CH - 1);
            if (tl < cn && f0 + gi < a.F) {
                const unsigned t = t0 + tl, j = t % p, off = tab[j], keep = tab[YAGI_CONVCODE_PERIOD_MAX + j];
                const auto at = source.step(chunk, gi, t);
                unsigned A0 = 0, A1 = 0;
#pragma unroll
                for (unsigned r = 0; r < 4; ++r)
                    if ((keep >> r) & 1u) {
                        const unsigned sv = source.soft(at, (off >> (8 * r)) & 0xffu);
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
        sink.begin(f);
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
        if (a.n & 7u) sink.partial(a.n >> 3, acc);
#pragma unroll 1
        while (t > 0) {                                     // whole bytes: bit t = e & 1 goes to position 7 - (t & 7)
            acc = 0;
#pragma unroll
            for (unsigned k = 0; k < 8; ++k) {
                --t;
                acc |= (e & 1u) << k;
                back(t);
            }
            sink.byte(t >> 3, acc);
        }
        sink.end(f, (klo >> 8) | (khi << 24));
    }
}

}  // namespace yagi
