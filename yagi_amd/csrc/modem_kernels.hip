// modem_kernels.hip -- Modem (src/modem/modem.rs, src/modem/modem/*.rs): block linear modulation and hard / soft
// demodulation, and the host forms of the same arithmetic (construction and the per-sample calls of the C ABI).
//
// The reference maps one symbol per call.  Every mapping is independent of its neighbours except DPSK's carried phase,
// so a block is one pass: 1 byte in / 8 out (modulate), 8 in / 1 (+ 8 for xhat, + bps soft bytes) out (demodulate).
// One set of __host__ __device__ functions (md_* below) holds the per-sample arithmetic -- the successive-approximation
// loop of demodulate_linear_array_ref with `>` as written, the sign tests of BPSK / QPSK / OOK and their soft formulas,
// the neighbour-table soft bits, Arb's first-minimum search and its soft loop with the reference's quirk -- and the
// kernels and the host mirror both call it.  Every operation is one f32 rounding: the Makefile builds this file with
// -ffp-contract=off, and tests/test_modem_isa_cpu.py checks that the decision and soft-bit kernels hold no f32 FMA
// (the PSK / DPSK kernels call the device library's atan2f / sincosf, whose own polynomials are fused; devmath.hpp has
// neither) and that no kernel uses scratch.
//
// modem_demod_kernel<KIND, BPS, SOFT>: a workgroup of 256 lanes owns kModemDemodTile = 2048 consecutive samples, lane t
// the samples t, t + 256, ... (coalesced 8-byte loads).  The map (<= 256 points) and the neighbour table live in LDS,
// reference[] and the other parameters in scalar registers (kernel arguments), and the loops over bps are unrolled at
// compile time.  Symbols and soft bytes are collected in LDS and leave as 16-byte stores at any byte alignment.  DPSK
// keeps atan2 of every sample of the tile in LDS, one slot in front for the sample before the tile (the object's phi
// for the first tile), and takes adjacent differences.  The lane that holds sample n - 1 writes the state the call
// leaves (r, x_hat, phi).
// modem_arb_kernel<BPS, SOFT>: the same tile; each lane runs the table loop over four samples at a time, so one LDS
// broadcast read of a point (every lane the same address) feeds four distance updates.  The soft loop tests the bits of
// the RUNNING best index, as arb.rs:52-63 does, so it stays ordered per sample.
// modem_modulate_kernel<DPSK>: a workgroup owns kModemModTile = 4096 symbols: one 16-byte load per lane at any byte
// alignment, through LDS, out as 16-byte stores of two points each.  modem_check_kernel runs first: a symbol >= M sets
// a flag that makes the other kernels return before they write and that the call reads back.  DPSK modulation is the
// exact integer running sum k_n = (k_{n-1} + gray_decode(s_n)) mod M: the check kernel leaves the sum of every tile,
// modem_scan_kernel (one workgroup) turns the sums into each tile's carry-in and writes the state, and the modulate
// kernel scans inside the workgroup.  No workgroup waits for another.
#pragma clang fp contract(off)

#include <cmath>
#include <type_traits>

#include "devmath.hpp"
#include "kernels.hpp"
#include "modem_body.hpp"     // md_linear, md_arb_step, the constants: shared with symtrack_kernels.hip

namespace yagi {
namespace {

constexpr int kWg = kModemWg;
struct __attribute__((packed, aligned(1))) md_b16 { unsigned v[4]; };     // 16 bytes at any byte address
struct __attribute__((packed, aligned(8))) md_f16 { float v[4]; };        // two points at a point's alignment

MD_HD unsigned md_gray_decode(unsigned s) {        // modem.rs:521-537 on 8 bits
    s ^= s >> 4;
    s ^= s >> 2;
    s ^= s >> 1;
    return s;
}
// `x.clamp(0.0, 255.0) as u8` (NaN -> 0)
MD_HD uint8_t md_soft_byte(float v) {
    if (!(v >= 0.0f)) v = 0.0f;
    if (v > 255.0f) v = 255.0f;
    return (uint8_t)(int)v;
}
MD_HD float md_atan2(float y, float x) { return atan2f(y, x); }
MD_HD cf32 md_polar1(float a) {                     // Complex32::from_polar(1.0, a)
    float s, c;
#if defined(__HIP_DEVICE_COMPILE__)
    sincosf(a, &s, &c);
#else
    s = sinf(a);
    c = cosf(a);
#endif
    return cf32{c, s};
}

template <int KIND, int BPS>
constexpr bool md_has_table() {
    return (KIND == MODEM_ASK && BPS >= 2 && BPS < 8) || (KIND == MODEM_PSK && BPS >= 3) || (KIND == MODEM_QAM && BPS >= 3);
}

// One sample of demodulate / demodulate_soft for every scheme but Arb.  theta: atan2 of the sample (PSK, DPSK);
// phi: DPSK's previous phase.  sb receives BPS soft bytes when SOFT.
template <int KIND, int BPS, bool SOFT>
MD_HD unsigned md_demod(const ModemParams &P, const cf32 *map, const uint8_t *nbr, cf32 x, float theta, float phi,
                        cf32 &xh, uint8_t *sb) {
    unsigned s = 0;
    if constexpr (KIND == MODEM_ASK) {                                       // ask.rs:51-63
        float res;
        s = md_gray_encode(md_linear<BPS>(P.ref, x.re, res));
        xh = map[s];
    } else if constexpr (KIND == MODEM_QAM) {                                // qam.rs:95-116
        constexpr int mi = (BPS + 1) >> 1, mq = BPS >> 1;
        float ri, rq;
        const unsigned si = md_gray_encode(md_linear<mi>(P.ref, x.re, ri));
        const unsigned sq = md_gray_encode(md_linear<mq>(P.ref, x.im, rq));
        s = (si << mq) + sq;
        xh = cf32{x.re - ri, x.im - rq};
    } else if constexpr (KIND == MODEM_PSK) {                                // psk.rs:60-74
        float t = theta - P.d_phi;
        if (t < -kPi) t += kTwoPi;
        float res;
        s = md_gray_encode(md_linear<BPS>(P.ref, t, res));
        xh = map[s];
    } else if constexpr (KIND == MODEM_DPSK) {                               // dpsk.rs:74-104
        float d = theta - phi;
        d -= P.d_phi;
        if (d > kPi) d -= kTwoPi;
        else if (d < -kPi) d += kTwoPi;
        float res;
        s = md_gray_encode(md_linear<BPS>(P.ref, d, res));
        xh = md_polar1(theta - res);
    } else if constexpr (KIND == MODEM_BPSK) {                               // bpsk.rs:15-33
        s = x.re > 0.0f ? 0u : 1u;
        xh = cf32{s == 0 ? 1.0f : -1.0f, 0.0f};
        if constexpr (SOFT) sb[0] = md_soft_byte(((-2.0f * x.re) * 4.0f) * 16.0f + 127.0f);
    } else if constexpr (KIND == MODEM_QPSK) {                               // qpsk.rs:16-38
        s = (x.re > 0.0f ? 0u : 1u) + (x.im > 0.0f ? 0u : 2u);
        xh = cf32{(s & 1u) == 0 ? kRsqrt2 : -kRsqrt2, (s & 2u) == 0 ? kRsqrt2 : -kRsqrt2};
        if constexpr (SOFT) {
            sb[0] = md_soft_byte(((-2.0f * x.im) * 5.8f) * 16.0f + 127.0f);
            sb[1] = md_soft_byte(((-2.0f * x.re) * 5.8f) * 16.0f + 127.0f);
        }
    } else {                                                                 // ook.rs:16-25
        s = x.re > kRsqrt2 ? 0u : 1u;
        xh = cf32{s != 0 ? 0.0f : kSqrt2, 0.0f};
    }
    if constexpr (SOFT && md_has_table<KIND, BPS>()) {                       // demodulate_soft_table :317-364
        float d0[BPS], d1[BPS];
        {
            const float er = x.re - xh.re, ei = x.im - xh.im;
            const float d = er * er + ei * ei;
#pragma unroll
            for (int k = 0; k < BPS; ++k) {
                const bool bit = (s >> (BPS - k - 1)) & 1u;
                d1[k] = bit ? d : 8.0f;
                d0[k] = bit ? 8.0f : d;
            }
        }
        const int p = P.p;
        for (int i = 0; i < p; ++i) {
            const unsigned nb = nbr[s * (unsigned)p + (unsigned)i];
            const cf32 c = map[nb];
            const float er = x.re - c.re, ei = x.im - c.im;
            const float d = er * er + ei * ei;
#pragma unroll
            for (int k = 0; k < BPS; ++k) {
                const bool bit = (nb >> (BPS - k - 1)) & 1u;
                if (bit) {
                    if (d < d1[k]) d1[k] = d;
                } else {
                    if (d < d0[k]) d0[k] = d;
                }
            }
        }
        constexpr float gamma = 1.2f * (float)(1 << BPS);
#pragma unroll
        for (int k = 0; k < BPS; ++k) sb[k] = md_soft_byte(((d0[k] - d1[k]) * gamma) * 16.0f + 127.0f);
    } else if constexpr (SOFT && KIND != MODEM_BPSK && KIND != MODEM_QPSK) {  // unpack_soft_bits :561-575
#pragma unroll
        for (int k = 0; k < BPS; ++k) sb[k] = ((s >> (BPS - k - 1)) & 1u) ? 255 : 0;
    }
    return s;
}

template <int BPS>
MD_HD void md_arb_soft(const ModemParams &P, const float *d0, const float *d1, uint8_t *sb) {
#pragma unroll
    for (int k = 0; k < BPS; ++k) sb[k] = md_soft_byte(((d0[k] - d1[k]) * P.gamma) * 16.0f + 127.0f);
}

// ---- device ------------------------------------------------------------------------------------------------------
// bytes [0, count) of an LDS tile to dst at any byte alignment: 16 bytes per store, then the odd bytes
__device__ __forceinline__ void md_store_bytes(uint8_t *dst, const uint8_t *lds, int count) {
    const int full = count >> 4;
    for (int c = threadIdx.x; c < full; c += kWg)
        *reinterpret_cast<md_b16 *>(dst + (size_t)c * 16) = *reinterpret_cast<const md_b16 *>(lds + c * 16);
    const int done = full << 4;
    if ((int)threadIdx.x < count - done) dst[done + threadIdx.x] = lds[done + threadIdx.x];
}

template <int BPS, bool SOFT>
__device__ __forceinline__ void md_emit(uint8_t *lsym, uint8_t *lsoft, int i, unsigned s, const uint8_t *sb) {
    lsym[i] = (uint8_t)s;
    if constexpr (SOFT) {
#pragma unroll
        for (int k = 0; k < BPS; ++k) lsoft[i * BPS + k] = sb[k];
    }
}

constexpr int kDemodR = kModemDemodTile / kWg;

template <int KIND, int BPS, bool SOFT>
__global__ __launch_bounds__(kWg) void modem_demod_kernel(ModemParams P, const cf32 *__restrict__ map,
                                                          const uint8_t *__restrict__ nbr, const ModemState *st,
                                                          ModemState *st_next, const cf32 *__restrict__ x, size_t n,
                                                          uint8_t *__restrict__ sym, cf32 *__restrict__ xhat,
                                                          uint8_t *__restrict__ soft) {
    constexpr int M = 1 << BPS;
    constexpr bool TABLE = md_has_table<KIND, BPS>();
    __shared__ cf32 lmap[M];
    __shared__ uint8_t lnbr[TABLE ? M * 4 : 16];
    __shared__ __attribute__((aligned(16))) uint8_t lsym[kModemDemodTile];
    __shared__ __attribute__((aligned(16))) uint8_t lsoft[SOFT ? kModemDemodTile * BPS : 16];
    __shared__ float lth[KIND == MODEM_DPSK ? kModemDemodTile + 1 : 1];
    const int tid = threadIdx.x;
    for (int i = tid; i < M; i += kWg) lmap[i] = map[i];
    if constexpr (TABLE)
        for (int i = tid; i < M * P.p; i += kWg) lnbr[i] = nbr[i];
    const size_t base = (size_t)blockIdx.x * kModemDemodTile;
    const int cnt = (int)(n - base < (size_t)kModemDemodTile ? n - base : (size_t)kModemDemodTile);
    cf32 xv[kDemodR];
#pragma unroll
    for (int j = 0; j < kDemodR; ++j) {
        const int i = j * kWg + tid;
        xv[j] = i < cnt ? x[base + i] : cf32{1.0f, 0.0f};
    }
    if constexpr (KIND == MODEM_DPSK) {
#pragma unroll
        for (int j = 0; j < kDemodR; ++j) lth[1 + j * kWg + tid] = md_atan2(xv[j].im, xv[j].re);
        if (tid == 0) {
            if (base == 0) {
                lth[0] = st->phi;
            } else {
                const cf32 xp = x[base - 1];
                lth[0] = md_atan2(xp.im, xp.re);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kDemodR; ++j) {
        const int i = j * kWg + tid;
        if (i < cnt) {
            float theta = 0.0f, phi = 0.0f;
            if constexpr (KIND == MODEM_PSK) theta = md_atan2(xv[j].im, xv[j].re);
            if constexpr (KIND == MODEM_DPSK) {
                theta = lth[1 + i];
                phi = lth[i];
            }
            cf32 xh;
            uint8_t sb[8];
            const unsigned s = md_demod<KIND, BPS, SOFT>(P, lmap, lnbr, xv[j], theta, phi, xh, sb);
            md_emit<BPS, SOFT>(lsym, lsoft, i, s, sb);
            if (xhat) xhat[base + i] = xh;
            if (base + i == n - 1) {
                ModemState o = *st;
                o.r = xv[j];
                o.x_hat = xh;
                if constexpr (KIND == MODEM_DPSK) o.phi = theta;
                *st_next = o;
            }
        }
    }
    __syncthreads();
    md_store_bytes(sym + base, lsym, cnt);
    if constexpr (SOFT) md_store_bytes(soft + base * BPS, lsoft, cnt * BPS);
}

constexpr int kArbR = 4;     // samples per lane and table pass

template <int BPS, bool SOFT>
__global__ __launch_bounds__(kWg) void modem_arb_kernel(ModemParams P, const cf32 *__restrict__ map, const ModemState *st,
                                                        ModemState *st_next, const cf32 *__restrict__ x, size_t n,
                                                        uint8_t *__restrict__ sym, cf32 *__restrict__ xhat,
                                                        uint8_t *__restrict__ soft) {
    constexpr int M = 1 << BPS;
    __shared__ cf32 lmap[M];
    __shared__ __attribute__((aligned(16))) uint8_t lsym[kModemDemodTile];
    __shared__ __attribute__((aligned(16))) uint8_t lsoft[SOFT ? kModemDemodTile * BPS : 16];
    const int tid = threadIdx.x;
    for (int i = tid; i < M; i += kWg) lmap[i] = map[i];
    const size_t base = (size_t)blockIdx.x * kModemDemodTile;
    const int cnt = (int)(n - base < (size_t)kModemDemodTile ? n - base : (size_t)kModemDemodTile);
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kDemodR / kArbR; ++g) {
        if (g * kArbR * kWg >= cnt) continue;                                // uniform
        cf32 xv[kArbR];
        float dmin[kArbR], d0[kArbR][BPS], d1[kArbR][BPS];
        unsigned s[kArbR];
#pragma unroll
        for (int r = 0; r < kArbR; ++r) {
            const int i = (g * kArbR + r) * kWg + tid;
            xv[r] = i < cnt ? x[base + i] : cf32{1.0f, 0.0f};
            dmin[r] = INFINITY;
            s[r] = 0;
#pragma unroll
            for (int k = 0; k < BPS; ++k) d0[r][k] = d1[r][k] = 4.0f;
        }
        for (int idx = 0; idx < M; ++idx) {
            const cf32 c = lmap[idx];                                        // one address per wave: broadcast
#pragma unroll
            for (int r = 0; r < kArbR; ++r) md_arb_step<BPS, SOFT>(xv[r], c, (unsigned)idx, dmin[r], s[r], d0[r], d1[r]);
        }
#pragma unroll
        for (int r = 0; r < kArbR; ++r) {
            const int i = (g * kArbR + r) * kWg + tid;
            if (i < cnt) {
                uint8_t sb[8];
                if constexpr (SOFT) md_arb_soft<BPS>(P, d0[r], d1[r], sb);
                md_emit<BPS, SOFT>(lsym, lsoft, i, s[r], sb);
                const cf32 xh = lmap[s[r]];
                if (xhat) xhat[base + i] = xh;
                if (base + i == n - 1) {
                    ModemState o = *st;
                    o.r = xv[r];
                    o.x_hat = xh;
                    *st_next = o;
                }
            }
        }
    }
    __syncthreads();
    md_store_bytes(sym + base, lsym, cnt);
    if constexpr (SOFT) md_store_bytes(soft + base * BPS, lsoft, cnt * BPS);
}

// a lane's 16 symbols of the tile; bytes beyond the tile's count read as 0
__device__ __forceinline__ void md_load16(const uint8_t *__restrict__ sym, int i0, int cnt, uint8_t *b) {
    if (i0 + 16 <= cnt) {
        const md_b16 q = *reinterpret_cast<const md_b16 *>(sym + i0);
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int e = 0; e < 4; ++e) b[w * 4 + e] = (uint8_t)(q.v[w] >> (8 * e));
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) b[e] = i0 + e < cnt ? sym[i0 + e] : (uint8_t)0;
    }
}

__device__ __forceinline__ unsigned md_wave_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// inclusive sum over the workgroup's 256 lanes; total receives the workgroup's sum.  lw: 4 words of LDS.
__device__ __forceinline__ unsigned md_wg_scan(unsigned v, unsigned *lw, unsigned &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned u = __shfl_up(v, off, 64);
        if (lane >= off) v += u;
    }
    __syncthreads();                       // lw may still be read from the previous round
    if (lane == 63) lw[wave] = v;
    __syncthreads();
    unsigned pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kWg / 64; ++w) {
        if (w < wave) pre += lw[w];
        tot += lw[w];
    }
    total = tot;
    return v + pre;
}

// Range check of every symbol (flag) and, for DPSK, the sum of gray_decode(s) over each tile (partials[tile]).
template <bool DPSK>
__global__ __launch_bounds__(kWg) void modem_check_kernel(int M, const uint8_t *__restrict__ sym, size_t n, int *flag,
                                                          unsigned *__restrict__ partials) {
    __shared__ unsigned lw[kWg / 64];
    const size_t base = (size_t)blockIdx.x * kModemModTile;
    const int cnt = (int)(n - base < (size_t)kModemModTile ? n - base : (size_t)kModemModTile);
    uint8_t b[16];
    md_load16(sym + base, threadIdx.x * 16, cnt, b);
    bool bad = false;
    unsigned sum = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        bad |= (int)b[e] >= M;
        sum += md_gray_decode(b[e]);
    }
    if (bad) atomicOr(flag, 1);
    if constexpr (DPSK) {
        sum = md_wave_sum(sum);
        if ((threadIdx.x & 63) == 0) lw[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned t = 0;
            for (int w = 0; w < kWg / 64; ++w) t += lw[w];
            partials[blockIdx.x] = t;
        }
    }
}

// One workgroup: partials[t] becomes the running index in front of tile t (the object's k included); the state the
// call leaves is k after the last symbol, and r the last output as modulate_dpsk leaves it (dpsk.rs:66).
__global__ __launch_bounds__(kWg) void modem_scan_kernel(int M, const cf32 *__restrict__ map, const ModemState *st,
                                                         ModemState *st_next, unsigned *partials, size_t tiles,
                                                         const int *flag) {
    __shared__ unsigned lw[kWg / 64];
    if (*flag) return;
    unsigned carry = st->k;
    for (size_t c = 0; c < tiles; c += kWg) {
        const size_t t = c + threadIdx.x;
        const unsigned v = t < tiles ? partials[t] : 0u;
        unsigned total;
        const unsigned incl = md_wg_scan(v, lw, total);
        if (t < tiles) partials[t] = carry + (incl - v);
        carry += total;
    }
    if (threadIdx.x == 0) {
        ModemState o = *st;
        o.k = carry & (unsigned)(M - 1);
        o.r = map[o.k];
        *st_next = o;
    }
}

template <bool DPSK>
__global__ __launch_bounds__(kWg) void modem_modulate_kernel(int M, const cf32 *__restrict__ map,
                                                             const unsigned *__restrict__ partials, const int *flag,
                                                             const uint8_t *__restrict__ sym, size_t n,
                                                             cf32 *__restrict__ y) {
    __shared__ cf32 lmap[256];
    __shared__ __attribute__((aligned(16))) uint8_t lsym[kModemModTile];
    __shared__ unsigned lw[kWg / 64];
    if (*flag) return;                                                       // uniform: nothing is written
    const int tid = threadIdx.x;
    for (int i = tid; i < M; i += kWg) lmap[i] = map[i];
    const size_t base = (size_t)blockIdx.x * kModemModTile;
    const int cnt = (int)(n - base < (size_t)kModemModTile ? n - base : (size_t)kModemModTile);
    uint8_t b[16];
    md_load16(sym + base, tid * 16, cnt, b);
    if constexpr (DPSK) {
        unsigned run = 0, loc[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            run += md_gray_decode(b[e]);
            loc[e] = run;
        }
        unsigned total;
        const unsigned incl = md_wg_scan(run, lw, total);
        const unsigned pre = partials[blockIdx.x] + (incl - run);
#pragma unroll
        for (int e = 0; e < 16; ++e) b[e] = (uint8_t)((pre + loc[e]) & (unsigned)(M - 1));
    }
    unsigned q[4];
#pragma unroll
    for (int w = 0; w < 4; ++w)
        q[w] = (unsigned)b[w * 4] | ((unsigned)b[w * 4 + 1] << 8) | ((unsigned)b[w * 4 + 2] << 16) | ((unsigned)b[w * 4 + 3] << 24);
    *reinterpret_cast<uint4 *>(lsym + tid * 16) = make_uint4(q[0], q[1], q[2], q[3]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kModemModTile / (2 * kWg); ++j) {
        const int i = 2 * (j * kWg + tid);
        if (i + 1 < cnt) {
            const cf32 a = lmap[lsym[i]], c = lmap[lsym[i + 1]];
            md_f16 o;
            o.v[0] = a.re;
            o.v[1] = a.im;
            o.v[2] = c.re;
            o.v[3] = c.im;
            *reinterpret_cast<md_f16 *>(y + base + i) = o;
        } else if (i < cnt) {
            y[base + i] = lmap[lsym[i]];
        }
    }
}

template <int KIND, int BPS>
int demod_launch(const ModemParams &P, const cf32 *map, const uint8_t *nbr, const ModemState *s, ModemState *sn,
                 const cf32 *x, size_t n, uint8_t *sym, cf32 *xhat, uint8_t *soft, hipStream_t st) {
    const dim3 grid((unsigned)((n + kModemDemodTile - 1) / kModemDemodTile));
    if constexpr (KIND == MODEM_ARB) {
        if (soft) hipLaunchKernelGGL((modem_arb_kernel<BPS, true>), grid, dim3(kWg), 0, st, P, map, s, sn, x, n, sym, xhat, soft);
        else hipLaunchKernelGGL((modem_arb_kernel<BPS, false>), grid, dim3(kWg), 0, st, P, map, s, sn, x, n, sym, xhat, soft);
    } else {
        if (soft)
            hipLaunchKernelGGL((modem_demod_kernel<KIND, BPS, true>), grid, dim3(kWg), 0, st, P, map, nbr, s, sn, x, n, sym, xhat, soft);
        else
            hipLaunchKernelGGL((modem_demod_kernel<KIND, BPS, false>), grid, dim3(kWg), 0, st, P, map, nbr, s, sn, x, n, sym, xhat, soft);
    }
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

template <int KIND, int BPS>
unsigned host_demod(const ModemParams &P, const cf32 *map, const uint8_t *nbr, cf32 x, ModemState &s, uint8_t *soft) {
    cf32 xh;
    uint8_t sb[8];
    unsigned sym;
    if constexpr (KIND == MODEM_ARB) {
        float dmin = INFINITY, d0[BPS], d1[BPS];
        for (int k = 0; k < BPS; ++k) d0[k] = d1[k] = 4.0f;
        sym = 0;
        for (int idx = 0; idx < (1 << BPS); ++idx) {
            if (soft) md_arb_step<BPS, true>(x, map[idx], (unsigned)idx, dmin, sym, d0, d1);
            else md_arb_step<BPS, false>(x, map[idx], (unsigned)idx, dmin, sym, d0, d1);
        }
        md_arb_soft<BPS>(P, d0, d1, sb);
        xh = map[sym];
    } else {
        float theta = 0.0f;
        if (KIND == MODEM_PSK || KIND == MODEM_DPSK) theta = md_atan2(x.im, x.re);
        if (soft) sym = md_demod<KIND, BPS, true>(P, map, nbr, x, theta, s.phi, xh, sb);
        else sym = md_demod<KIND, BPS, false>(P, map, nbr, x, theta, s.phi, xh, sb);
        if (KIND == MODEM_DPSK) s.phi = theta;
    }
    if (soft)
        for (int k = 0; k < BPS; ++k) soft[k] = sb[k];
    s.r = x;
    s.x_hat = xh;
    return sym;
}

// run f(kind, bps) as compile-time constants for the (kind, bps) pairs the constructor admits
template <int V> using md_ic = std::integral_constant<int, V>;
template <int KIND, int LO, class Fn>
bool md_bps(int bps, Fn &&f) {
    switch (bps) {
        case 1: if constexpr (LO <= 1) { f(md_ic<KIND>{}, md_ic<1>{}); return true; } break;
        case 2: if constexpr (LO <= 2) { f(md_ic<KIND>{}, md_ic<2>{}); return true; } break;
        case 3: f(md_ic<KIND>{}, md_ic<3>{}); return true;
        case 4: f(md_ic<KIND>{}, md_ic<4>{}); return true;
        case 5: f(md_ic<KIND>{}, md_ic<5>{}); return true;
        case 6: f(md_ic<KIND>{}, md_ic<6>{}); return true;
        case 7: f(md_ic<KIND>{}, md_ic<7>{}); return true;
        case 8: f(md_ic<KIND>{}, md_ic<8>{}); return true;
    }
    return false;
}
template <class Fn>
bool md_dispatch(const ModemParams &P, Fn &&f) {
    switch (P.kind) {
        case MODEM_PSK: return md_bps<MODEM_PSK, 1>(P.bps, f);
        case MODEM_DPSK: return md_bps<MODEM_DPSK, 1>(P.bps, f);
        case MODEM_ASK: return md_bps<MODEM_ASK, 1>(P.bps, f);
        case MODEM_QAM: return md_bps<MODEM_QAM, 2>(P.bps, f);
        case MODEM_ARB: return md_bps<MODEM_ARB, 1>(P.bps, f);
        case MODEM_BPSK: if (P.bps == 1) { f(md_ic<MODEM_BPSK>{}, md_ic<1>{}); return true; } break;
        case MODEM_QPSK: if (P.bps == 2) { f(md_ic<MODEM_QPSK>{}, md_ic<2>{}); return true; } break;
        case MODEM_OOK: if (P.bps == 1) { f(md_ic<MODEM_OOK>{}, md_ic<1>{}); return true; } break;
    }
    return false;
}

}  // namespace

unsigned modem_host_demod(const ModemParams &P, const cf32 *map, const uint8_t *nbr, cf32 x, ModemState &s, uint8_t *soft) {
    unsigned sym = 0;
    md_dispatch(P, [&](auto K, auto B) { sym = host_demod<decltype(K)::value, decltype(B)::value>(P, map, nbr, x, s, soft); });
    return sym;
}

unsigned modem_host_modulate_dpsk(const ModemParams &P, unsigned sym, unsigned k) {
    return (k + md_gray_decode(sym)) & (unsigned)(P.M - 1);
}

size_t modem_num_partials(size_t n) { return (n + kModemModTile - 1) / kModemModTile; }

int launch_modem_demod(const ModemParams &P, const cf32 *map, const uint8_t *nbr, const ModemState *s, ModemState *sn,
                       const cf32 *x, size_t n, uint8_t *sym, cf32 *xhat, uint8_t *soft, hipStream_t st) {
    if (n == 0) return YAGI_OK;
    int rc = YAGI_OK;
    if (md_dispatch(P, [&](auto K, auto B) {
            rc = demod_launch<decltype(K)::value, decltype(B)::value>(P, map, nbr, s, sn, x, n, sym, xhat, soft, st);
        }))
        return rc;
    return fail(YAGI_ERR_INTERNAL, "modem: no kernel for kind %d at %d bits/symbol", P.kind, P.bps);
}

int launch_modem_modulate(const ModemParams &P, const cf32 *map, const ModemState *s, ModemState *sn, const uint8_t *sym,
                          size_t n, cf32 *y, unsigned *partials, int *flag, hipStream_t st) {
    if (n == 0) return YAGI_OK;
    const size_t tiles = modem_num_partials(n);
    const dim3 grid((unsigned)tiles), wg(kWg);
    YG_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    if (P.kind == MODEM_DPSK) {
        hipLaunchKernelGGL((modem_check_kernel<true>), grid, wg, 0, st, P.M, sym, n, flag, partials);
        hipLaunchKernelGGL(modem_scan_kernel, dim3(1), wg, 0, st, P.M, map, s, sn, partials, tiles, (const int *)flag);
        hipLaunchKernelGGL((modem_modulate_kernel<true>), grid, wg, 0, st, P.M, map, (const unsigned *)partials,
                           (const int *)flag, sym, n, y);
    } else {
        hipLaunchKernelGGL((modem_check_kernel<false>), grid, wg, 0, st, P.M, sym, n, flag, partials);
        hipLaunchKernelGGL((modem_modulate_kernel<false>), grid, wg, 0, st, P.M, map, (const unsigned *)partials,
                           (const int *)flag, sym, n, y);
    }
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

// ---- construction (host) -------------------------------------------------------------------------------------------
// init_demod_soft_tab :465-511.  The reference's "empty" mark is `M as u8`, which is 0 at M = 256 and bars symbol 0
// from every list there; the mark here is out of range, so every list holds the p nearest other points.
static void modem_neighbours(const std::vector<cf32> &c, int p, std::vector<uint8_t> &nbr) {
    const int M = (int)c.size();
    std::vector<int> t((size_t)M * p, -1);
    for (int i = 0; i < M; ++i)
        for (int k = 0; k < p; ++k) {
            float dmin = 1e9f;
            for (int j = 0; j < M; ++j) {
                bool valid = i != j;
                for (int l = 0; l < p; ++l)
                    if (t[(size_t)i * p + l] == j) valid = false;
                const float d = std::hypot(c[i].re - c[j].re, c[i].im - c[j].im);
                if (d < dmin && valid) {
                    dmin = d;
                    t[(size_t)i * p + k] = j;
                }
            }
        }
    nbr.resize(t.size());
    for (size_t i = 0; i < t.size(); ++i) nbr[i] = (uint8_t)t[i];
}

int modem_design(int kind, int bps, const cf32 *table, ModemParams &P, std::vector<cf32> &map, std::vector<uint8_t> &nbr) {
    if (bps < 1 || bps > 8) return fail(YAGI_ERR_CONFIG, "modem: bits per symbol must be in 1..8");
    const int M = 1 << bps;
    P = ModemParams{};
    P.kind = kind;
    P.bps = bps;
    P.M = M;
    map.assign((size_t)M, cf32{0.0f, 0.0f});
    nbr.clear();
    float alpha = 0.0f;
    if (kind == MODEM_PSK || kind == MODEM_DPSK) {                           // psk.rs:25-45, dpsk.rs:31-46
        alpha = kPi / (float)M;
        P.d_phi = kPi * (1.0f - 1.0f / (float)M);
        for (int i = 0; i < M; ++i) {
            const unsigned sd = kind == MODEM_PSK ? md_gray_decode((unsigned)i) : (unsigned)i;
            map[i] = md_polar1((float)sd * 2.0f * alpha);
        }
        if (kind == MODEM_PSK && bps >= 3) P.p = 2;
    } else if (kind == MODEM_ASK) {                                          // ask.rs:10-50
        static const float e[8] = {1.0f, 5.0f, 21.0f, 85.0f, 341.0f, 1365.0f, 5461.0f, 21845.0f};
        alpha = bps == 1 ? 1.0f : 1.0f / std::sqrt(e[bps - 1]);
        for (int i = 0; i < M; ++i) map[i] = cf32{(float)(2 * (int)md_gray_decode((unsigned)i) - M + 1) * alpha, 0.0f};
        if (bps >= 2 && bps < 8) P.p = 2;
    } else if (kind == MODEM_QAM) {                                          // qam.rs:13-93
        if (bps < 2) return fail(YAGI_ERR_CONFIG, "modem: QAM needs at least 2 bits per symbol");
        static const float e[7] = {2.0f, 6.0f, 10.0f, 26.0f, 42.0f, 106.0f, 170.0f};
        alpha = 1.0f / std::sqrt(e[bps - 2]);
        const int mi = (bps + 1) >> 1, mq = bps >> 1;
        for (int i = 0; i < M; ++i) {
            const int si = (int)md_gray_decode((unsigned)i >> mq), sq = (int)md_gray_decode((unsigned)i & ((1u << mq) - 1));
            map[i] = cf32{(float)(2 * si - (1 << mi) + 1) * alpha, (float)(2 * sq - (1 << mq) + 1) * alpha};
        }
        P.p = bps == 3 ? 3 : bps >= 4 ? 4 : 0;
    } else if (kind == MODEM_BPSK && bps == 1) {
        map[0] = cf32{1.0f, 0.0f};
        map[1] = cf32{-1.0f, 0.0f};
    } else if (kind == MODEM_QPSK && bps == 2) {
        for (int i = 0; i < 4; ++i) map[i] = cf32{(i & 1) == 0 ? kRsqrt2 : -kRsqrt2, (i & 2) == 0 ? kRsqrt2 : -kRsqrt2};
    } else if (kind == MODEM_OOK && bps == 1) {
        map[0] = cf32{kSqrt2, 0.0f};
        map[1] = cf32{0.0f, 0.0f};
    } else if (kind == MODEM_ARB) {                                          // arb.rs:4-13, 76-94
        if (!table) return fail(YAGI_ERR_CONFIG, "null pointer argument");
        // the mean, the energy, the subtraction and the division in double, rounded to f32 once: every component is the
        // correctly rounded balanced and scaled point (the reference's f32 sums lose up to an ulp of the LARGEST point,
        // which is many ulps of a small component once the mean has cancelled)
        double sr = 0.0, si = 0.0;
        for (int i = 0; i < M; ++i) {
            sr += (double)table[i].re;
            si += (double)table[i].im;
        }
        const double mr = sr / M, mi = si / M;
        double energy = 0.0;
        for (int i = 0; i < M; ++i) {
            const double re = (double)table[i].re - mr, im = (double)table[i].im - mi;
            energy += re * re + im * im;
        }
        const double scale = std::sqrt(energy / M);
        if (!(scale > 0.0) || !std::isfinite(scale)) return fail(YAGI_ERR_CONFIG, "modem: table has no finite, non-zero energy");
        for (int i = 0; i < M; ++i)
            map[i] = cf32{(float)(((double)table[i].re - mr) / scale), (float)(((double)table[i].im - mi) / scale)};
        P.gamma = 1.2f * (float)bps;
    } else {
        return fail(YAGI_ERR_CONFIG, "modem: scheme not supported");
    }
    for (int k = 0; k < bps; ++k) P.ref[k] = (float)(1 << k) * alpha;
    if (P.p > 0) modem_neighbours(map, P.p, nbr);
    return YAGI_OK;
}

}  // namespace yagi
