// packetizer_kernels.hip -- Packetizer: CRC, ConvCode, block interleaver and scrambler for a bank of frames, one launch per
// direction (yagi_hip.h).  Everything is integer arithmetic, so every arrangement gives the definition's bytes exactly.
//
// pkt_decode_kernel<SPL, WIDE> is ConvCode's decoder, from convcode_body.hpp, with two things of its own:
//   - the lane that expands (frame, step) reads each kept byte at its transmit position pi(i) straight from the row, one
//     byte load and one multiplication by a reciprocal of C each, and turns it over where the scramble mask is set: no
//     staging of raw words, so nothing outside a row is read and the wave's LDS is the decisions and the expanded steps.
//     (Gathering a chunk's bytes into LDS first, where ConvCode lays its raw words, so that a chunk's loads are in flight
//     together, was measured too and is up to 5 % slower: profiles/r28_kbench_packetizer.txt.)
//   - the traceback lane meets the message from its last byte to its first: the CRC field comes first and stays in a
//     register, the n payload bytes are stored as they appear.  The CRC register is run BACKWARDS over them, from the
//     received field towards the start of the frame: one step is s = ((s' ^ T[i]) >> 8) | ((i ^ byte) << 24) with i the
//     table index whose entry ends in the low byte of s' (the polynomials are odd, so that byte names i), a single LDS
//     lookup in a 256-entry table of (T[i], i) that does not depend on the traceback's own chain of lookups.  The frame is
//     valid iff the walk ends at the scheme's init word I.  Where it ends at I' instead, the CRC of the decoded payload is
//     field + (I + I') x^(8n) mod P by linearity: one carry-less product with a constant of the object per frame.
//
// pkt_encode_kernel: a workgroup per frame.  Lane k runs the CRC register from zero over its slice of the payload and
// multiplies by x^(8 * bytes behind the slice) (a table of the object); the XOR of the 256 products and of I x^(8n) is the
// register.  Then a lane per output byte: each of its bps transmit bits j comes from coder-order bit i = pi^-1(j), through
// the inverse puncture table from (step, output), whose parity is taken on a K-bit window of payload || CRC in LDS.
//
// The host forms are the definition's loops around conv_encode_host / conv_decode_host.
#include <algorithm>
#include <vector>

#include "convcode_body.hpp"
#include "kernels.hpp"

namespace yagi {
namespace {

constexpr int kPktEncWg = 256;
constexpr uint32_t kScrambleWord = 0xCACC535Fu;            // scramble.rs :2-5, the first mask uppermost

// a(x) m(x) mod P on W-bit words (P without its x^W term)
__host__ __device__ inline uint32_t pkt_gfmul(uint32_t a, uint32_t m, unsigned W, uint32_t poly) {
    const uint32_t mask = W == 32 ? 0xffffffffu : (1u << W) - 1u;
    uint32_t r = 0;
    for (unsigned i = W; i-- > 0;) {
        const uint32_t top = (r >> (W - 1)) & 1u;
        r = ((r << 1) & mask) ^ (top ? poly : 0u);
        if ((a >> i) & 1u) r ^= m;
    }
    return r;
}

uint32_t pkt_xpow8(size_t nbytes, unsigned W, uint32_t poly) {      // x^(8 nbytes) mod P
    const uint32_t mask = W == 32 ? 0xffffffffu : (1u << W) - 1u;
    uint32_t r = 1;
    for (size_t i = 0; i < 8 * nbytes; ++i) {
        const uint32_t top = (r >> (W - 1)) & 1u;
        r = ((r << 1) & mask) ^ (top ? poly : 0u);
    }
    return r;
}

uint32_t pkt_reflect(uint32_t v, unsigned bits) {
    uint32_t r = 0;
    for (unsigned i = 0; i < bits; ++i) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}

// ---- decode ---------------------------------------------------------------------------------------------------------
struct PktDecArgs {
    ConvDecArgs c;          // msg = the payload plane; n = the 8 (n + w) message bits; tab = the object's table
    uint8_t *valid;
    uint32_t *crc;
    unsigned C, Cinv, q, r, smask, nbytes, w, sh, init, xorout, x8n, poly, reflected;
};

// soft byte of coder-order bit i: at transmit position pi(i) of the row, turned over where the mask is set
struct PktSource {
    const PktDecArgs &x;
    struct At {
        const uint8_t *row;
        unsigned i0;
    };
    __device__ __forceinline__ void stage(const ConvChunk &) const {}
    __device__ __forceinline__ At step(const ConvChunk &c, unsigned gi, unsigned t) const {
        return At{x.c.soft + (c.f0 + gi) * x.c.soft_pitch, t / x.c.p * x.c.kp};
    }
    __device__ __forceinline__ unsigned soft(const At &at, unsigned o) const {
        // i div C by the host's floor(2^32 / C) (2^32 - 1 at C = 1): the estimate is the quotient or one less
        const unsigned i = at.i0 + o, est = __umulhi(i, x.Cinv), rem = i - est * x.C;
        const unsigned rho = rem >= x.C ? est + 1u : est, col = rem >= x.C ? rem - x.C : rem;
        const unsigned j = col * x.q + (col < x.r ? col : x.r) + rho;          // < N: the row holds it
        const unsigned sv = at.row[j];
        return (x.smask >> (31u - (j & 31u))) & 1u ? 255u - sv : sv;
    }
};

struct PktSink {
    const PktDecArgs &x;
    const uint2 *rt;        // (T[i], i) by the byte of T[i] that a step leaves untouched
    uint8_t *out;
    unsigned s, field;
    __device__ __forceinline__ unsigned reg_of(unsigned f) const { return x.reflected ? __brev(f ^ x.xorout) : f ^ x.xorout; }
    __device__ __forceinline__ void begin(size_t f) {
        out = x.c.msg + f * x.c.msg_pitch;
        s = field = 0;
    }
    __device__ __forceinline__ void partial(unsigned, unsigned) {}               // the message is whole bytes
    __device__ __forceinline__ void byte(unsigned i, unsigned v) {
        if (i >= x.nbytes) {
            field |= v << (8u * (x.nbytes + x.w - 1u - i));
            if (i == x.nbytes) s = reg_of(field) << x.sh;
        } else {
            out[i] = (uint8_t)v;
            if (x.w) {
                const unsigned b = x.reflected ? __brev(v) >> 24 : v;
                const uint2 e = rt[(s >> x.sh) & 0xffu];
                s = ((s ^ e.x) >> 8) | ((e.y ^ b) << 24);
            }
        }
    }
    __device__ __forceinline__ void end(size_t f, unsigned metric) {
        unsigned ok = 1, val = 0;
        if (x.w) {
            const unsigned d = x.init ^ (s >> x.sh);
            ok = d == 0;
            const unsigned reg = reg_of(field) ^ pkt_gfmul(d, x.x8n, 32u - x.sh, x.poly);
            val = (x.reflected ? __brev(reg) : reg) ^ x.xorout;
        }
        x.valid[f] = (uint8_t)ok;
        if (x.crc) x.crc[f] = val;
        if (x.c.metric) x.c.metric[f] = metric;
    }
};

template <int SPL, bool WIDE>
__global__ __launch_bounds__(256) void pkt_decode_kernel(const PktDecArgs x) {
    extern __shared__ __align__(16) unsigned char pk_smem[];
    const unsigned waves = blockDim.x >> 6;
    uint32_t *rt = reinterpret_cast<uint32_t *>(pk_smem + kConvTableWords * 4 + (size_t)waves * x.c.wave_bytes);
    if (x.w) {
#pragma unroll 4
        for (unsigned e = threadIdx.x; e < kPktRevWords; e += blockDim.x) rt[e] = x.c.tab[kPktRevAt + e];    // visible after the body's first barrier
    }
    PktSource source{x};
    PktSink sink{x, reinterpret_cast<const uint2 *>(rt)};
    conv_decode_body<SPL, WIDE>(x.c, pk_smem, blockDim.x, source, sink);
}

template <int SPL, bool WIDE>
int pkt_decode_launch(const PktDecArgs &a, unsigned blocks, unsigned waves, size_t lds, hipStream_t st) {
    auto fn = pkt_decode_kernel<SPL, WIDE>;
    if (lds > 64 * 1024)
        YG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kConvLdsMax));
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(64 * waves), lds, st, a);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

// ---- encode ---------------------------------------------------------------------------------------------------------
struct PktEncArgs {
    const uint32_t *tab;
    const uint8_t *payload;
    uint8_t *tx;
    size_t payload_pitch, tx_pitch;
    unsigned n, w, N, nsym, bps, K, p, kp, g0, g1, g2, g3, C, q, r, smask, slice, sh, poly, initn, xorout, reflected;
};

__global__ __launch_bounds__(kPktEncWg) void pkt_encode_kernel(const PktEncArgs a) {
    extern __shared__ __align__(16) unsigned char pe_smem[];
    uint32_t *red = reinterpret_cast<uint32_t *>(pe_smem);             // [4] the waves' partial registers
    uint32_t *inv = red + 4;                                           // [kPktInvWords] coded index of a period -> step | output << 8
    uint8_t *m = reinterpret_cast<uint8_t *>(inv + kPktInvWords);      // 0, payload, crc, 0, 0: message byte i at m[1 + i]
    const unsigned tid = threadIdx.x, f = blockIdx.x;
    const uint8_t *pay = a.payload + (size_t)f * a.payload_pitch;
    if (tid < kPktInvWords) inv[tid] = a.tab[kPktInvAt + tid];

    // the lane's slice of the payload: into LDS, and through the CRC register from zero
    const unsigned lo = min(a.n, tid * a.slice), hi = min(a.n, lo + a.slice);
    const unsigned W = 32u - a.sh, poly32 = a.poly << a.sh;
    uint32_t reg = 0;
    for (unsigned i = lo; i < hi; ++i) {
        const unsigned v = pay[i];
        m[1 + i] = (uint8_t)v;
        reg ^= (a.reflected ? __brev(v) >> 24 : v) << 24;
#pragma unroll
        for (int k = 0; k < 8; ++k) reg = (reg << 1) ^ (reg & 0x80000000u ? poly32 : 0u);
    }
    uint32_t part = a.w && hi > lo ? pkt_gfmul(reg >> a.sh, a.tab[kPktZAt + tid], W, a.poly) : 0u;
    for (int d = 1; d < 64; d <<= 1) part ^= __shfl_xor(part, d);
    if ((tid & 63u) == 0) red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        const uint32_t total = red[0] ^ red[1] ^ red[2] ^ red[3] ^ a.initn;
        const uint32_t val = a.w ? (a.reflected ? __brev(total) : total) ^ a.xorout : 0u;
        m[0] = 0;
        for (unsigned k = 0; k < a.w; ++k) m[1 + a.n + k] = (uint8_t)(val >> (8u * (a.w - 1u - k)));
        m[1 + a.n + a.w] = m[2 + a.n + a.w] = 0;
    }
    __syncthreads();

    const unsigned head = a.r * (a.q + 1u), kmask = (1u << a.K) - 1u;
    uint8_t *out = a.tx + (size_t)f * a.tx_pitch;
    for (unsigned y = tid; y < a.nsym; y += kPktEncWg) {
        unsigned sym = 0;
        for (unsigned b = 0; b < a.bps; ++b) {
            const unsigned j = y * a.bps + b;
            if (j >= a.N) break;                                        // the missing bits of the last symbol are 0
            unsigned col, rho;
            if (j < head) {
                col = j / (a.q + 1u), rho = j - col * (a.q + 1u);
            } else {
                const unsigned jj = j - head, c1 = jj / a.q;
                col = a.r + c1, rho = jj - c1 * a.q;
            }
            const unsigned i = rho * a.C + col, per = i / a.kp, e = inv[i - per * a.kp];
            const unsigned t = per * a.p + (e & 0xffu), o = e >> 8;
            // message bits t - K + 1 .. t lie in bytes (t >> 3) - 1 and t >> 3; bit k of sr is message bit t - k
            const unsigned hb = t >> 3, word = ((unsigned)m[hb] << 8) | m[hb + 1];
            const unsigned sr = (word >> (7u - (t & 7u))) & kmask;
            const unsigned g = o == 0 ? a.g0 : o == 1 ? a.g1 : o == 2 ? a.g2 : a.g3;
            const unsigned bit = cv_parity(sr & g) ^ ((a.smask >> (31u - (j & 31u))) & 1u);
            sym |= bit << (a.bps - 1u - b);
        }
        out[y] = (uint8_t)sym;
    }
}

}  // namespace

bool crc_params(int scheme, CrcParams *out) {
    static const CrcParams k[5] = {{0, 0, 0, 0, false},
                                   {8, 0x07u, 0x00u, 0x00u, false},
                                   {16, 0x1021u, 0xFFFFu, 0x0000u, false},
                                   {24, 0x864CFBu, 0xB704CEu, 0x000000u, false},
                                   {32, 0x04C11DB7u, 0xFFFFFFFFu, 0xFFFFFFFFu, true}};
    if (scheme < 0 || scheme > 4) return false;
    *out = k[scheme];
    return true;
}

// the Rocksoft model bit by bit
uint32_t crc_host(const CrcParams &c, const uint8_t *data, size_t n) {
    if (c.width == 0) return 0;
    const unsigned W = (unsigned)c.width;
    const uint32_t mask = W == 32 ? 0xffffffffu : (1u << W) - 1u, top = 1u << (W - 1);
    uint32_t reg = c.init;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t b = c.reflected ? pkt_reflect(data[i], 8) : data[i];
        reg ^= b << (W - 8);
        for (int k = 0; k < 8; ++k) reg = reg & top ? ((reg << 1) ^ c.poly) & mask : (reg << 1) & mask;
    }
    if (c.reflected) reg = pkt_reflect(reg, W);
    return reg ^ c.xorout;
}

void pkt_permutation(size_t N, size_t C, uint32_t *pi) {
    const size_t q = N / C, r = N % C;
    for (size_t i = 0; i < N; ++i) pi[i] = (uint32_t)((i % C) * q + std::min(i % C, r) + i / C);
}

void scramble_data_host(uint8_t *x, size_t n) {                       // scramble.rs :7-29
    static const uint8_t mask[4] = {0xCA, 0xCC, 0x53, 0x5F};
    for (size_t i = 0; i < n; ++i) x[i] ^= mask[i & 3];
}

void unscramble_soft_host(uint8_t *x, size_t n) {                     // scramble.rs :37-53: whole groups of eight only
    for (size_t j = 0; j < (n & ~(size_t)7); ++j)
        if ((kScrambleWord >> (31 - (j & 31))) & 1u) x[j] = (uint8_t)(255 - x[j]);
}

void pkt_table(const Packetizer &k, uint32_t *words) {
    std::fill(words, words + kPktTableWords, 0u);
    conv_table(k.code, words);
    for (int j = 0; j < k.code.p; ++j)
        for (int r = 0; r < k.code.R; ++r)
            if ((k.code.keep[j] >> r) & 1u) words[kPktInvAt + ((k.code.off[j] >> (8 * r)) & 0xffu)] = (uint32_t)j | ((uint32_t)r << 8);
    if (k.crc.width == 0) return;
    const unsigned W = (unsigned)k.crc.width, sh = 32 - W;
    const size_t slice = pkt_slice(k.n);
    for (size_t lane = 0; lane < (size_t)kPktEncWg; ++lane) {
        const size_t hi = std::min(k.n, std::min(k.n, lane * slice) + slice);
        words[kPktZAt + lane] = pkt_xpow8(k.n - hi, W, k.crc.poly);
    }
    const uint32_t poly32 = k.crc.poly << sh;
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t t = i << 24;
        for (int b = 0; b < 8; ++b) t = (t << 1) ^ (t & 0x80000000u ? poly32 : 0u);
        const uint32_t low = (t >> sh) & 0xffu;                      // distinct for distinct i: P is odd
        words[kPktRevAt + 2 * low] = t;
        words[kPktRevAt + 2 * low + 1] = i;
    }
}

int launch_pkt_encode(const Packetizer &k, const uint32_t *tab, const uint8_t *payload, size_t payload_pitch, size_t F,
                      unsigned bps, uint8_t *tx, size_t tx_pitch, hipStream_t st) {
    if (F == 0) return YAGI_OK;
    if (bps < 1 || bps > 8 || F > (size_t)YAGI_CONVCODE_FRAMES_MAX || k.n == 0 || k.msg_bits() > k.code.nmax())
        return fail(YAGI_ERR_CONFIG, "packetizer: bad launch");
    const size_t N = k.N(), C = k.cols();
    const unsigned W = (unsigned)k.crc.width;
    PktEncArgs a{};
    a.tab = tab, a.payload = payload, a.tx = tx, a.payload_pitch = payload_pitch, a.tx_pitch = tx_pitch;
    a.n = (unsigned)k.n, a.w = (unsigned)k.w(), a.N = (unsigned)N, a.nsym = (unsigned)k.nsym(bps), a.bps = bps;
    a.K = (unsigned)k.code.K, a.p = (unsigned)k.code.p, a.kp = k.code.kp;
    a.g0 = k.code.g[0], a.g1 = k.code.g[1], a.g2 = k.code.g[2], a.g3 = k.code.g[3];
    a.C = (unsigned)C, a.q = (unsigned)(N / C), a.r = (unsigned)(N % C), a.smask = k.scramble ? kScrambleWord : 0u;
    a.slice = (unsigned)pkt_slice(k.n), a.sh = W ? 32 - W : 0, a.poly = k.crc.poly, a.xorout = k.crc.xorout;
    a.reflected = k.crc.reflected ? 1u : 0u;
    a.initn = W ? pkt_gfmul(k.crc.init, pkt_xpow8(k.n, W, k.crc.poly), W, k.crc.poly) : 0u;
    const size_t lds = (4 + kPktInvWords) * 4 + ((k.n + k.w() + 3 + 3) & ~(size_t)3);     // <= 16 + 512 + 8 KiB + 12
    hipLaunchKernelGGL(pkt_encode_kernel, dim3((unsigned)F), dim3(kPktEncWg), lds, st, a);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

int launch_pkt_decode(const Packetizer &k, ConvShape s, const uint32_t *tab, const uint8_t *soft, size_t soft_pitch, size_t F,
                      uint8_t *payload, size_t payload_pitch, uint8_t *valid, uint32_t *crc, uint32_t *metric, hipStream_t st) {
    if (F == 0) return YAGI_OK;
    const ConvCode &c = k.code;
    const size_t n = k.msg_bits();
    if (k.n == 0 || n > c.nmax() || F > (size_t)YAGI_CONVCODE_FRAMES_MAX) return fail(YAGI_ERR_CONFIG, "packetizer: bad launch");
    if (!conv_shape_ok(c.K, s))
        return fail(YAGI_ERR_CONFIG, "packetizer: the shape (%u frames per wave, %u waves) is not admissible at K = %d", s.fpw, s.waves, c.K);
    const size_t T = c.steps(n), lds = pkt_lds_bytes(c.K, s, T, k.crc.width != 0);
    if (lds > kConvLdsMax)
        return fail(YAGI_ERR_CONFIG, "packetizer: %u frames per wave and %u waves of %zu steps need %zu bytes of LDS", s.fpw, s.waves, T, lds);
    const size_t N = k.N(), C = k.cols();
    const unsigned W = (unsigned)k.crc.width;
    PktDecArgs x{};
    ConvDecArgs &a = x.c;
    a.tab = tab, a.soft = soft, a.msg = payload, a.metric = metric, a.soft_pitch = soft_pitch, a.msg_pitch = payload_pitch;
    a.n = (unsigned)n, a.T = (unsigned)T, a.F = (unsigned)F, a.K = (unsigned)c.K, a.R = (unsigned)c.R, a.p = (unsigned)c.p;
    a.kp = c.kp, a.terminated = c.terminated ? 1u : 0u;
    while ((1u << a.lg_fpw) < s.fpw) ++a.lg_fpw;
    a.W = (unsigned)conv_step_bytes(c.K, s);
    a.dec_bytes = (unsigned)((T * a.W + 7) & ~(size_t)7);
    a.wave_bytes = (unsigned)pkt_wave_bytes(c.K, s, T);
    a.g0 = c.g[0], a.g1 = c.g[1], a.g2 = c.g[2], a.g3 = c.g[3];
    x.valid = valid, x.crc = crc;
    x.C = (unsigned)C, x.q = (unsigned)(N / C), x.r = (unsigned)(N % C), x.smask = k.scramble ? kScrambleWord : 0u;
    x.Cinv = C == 1 ? 0xffffffffu : (unsigned)(((uint64_t)1 << 32) / C);
    x.nbytes = (unsigned)k.n, x.w = (unsigned)k.w(), x.sh = W ? 32 - W : 0, x.init = k.crc.init, x.xorout = k.crc.xorout;
    x.poly = k.crc.poly, x.reflected = k.crc.reflected ? 1u : 0u;
    x.x8n = W ? pkt_xpow8(k.n, W, k.crc.poly) : 0u;
    const size_t per_wg = (size_t)s.fpw * s.waves;
    const unsigned blocks = (unsigned)((F + per_wg - 1) / per_wg);
    switch (conv_spl(c.K)) {
        case 1: return a.W >= 8 ? pkt_decode_launch<1, true>(x, blocks, s.waves, lds, st)
                                : pkt_decode_launch<1, false>(x, blocks, s.waves, lds, st);
        case 2: return pkt_decode_launch<2, true>(x, blocks, s.waves, lds, st);
        default: return pkt_decode_launch<4, true>(x, blocks, s.waves, lds, st);
    }
}

// ---- the definition on the host -------------------------------------------------------------------------------------
void pkt_encode_host(const Packetizer &k, const uint8_t *payload, size_t payload_pitch, size_t F, unsigned bps, uint8_t *tx,
                     size_t tx_pitch) {
    const size_t n = k.n, w = k.w(), N = k.N(), nsym = k.nsym(bps);
    std::vector<uint8_t> msg(n + w), coded(N), sent(nsym * bps);
    std::vector<uint32_t> pi(N);
    pkt_permutation(N, k.columns, pi.data());
    for (size_t f = 0; f < F; ++f) {
        const uint8_t *in = payload + f * payload_pitch;
        std::copy(in, in + n, msg.begin());
        const uint32_t v = crc_host(k.crc, in, n);
        for (size_t i = 0; i < w; ++i) msg[n + i] = (uint8_t)(v >> (8 * (w - 1 - i)));
        conv_encode_host(k.code, msg.data(), n + w, k.msg_bits(), 1, coded.data(), N);
        std::fill(sent.begin(), sent.end(), (uint8_t)0);
        for (size_t i = 0; i < N; ++i) sent[pi[i]] = coded[i];
        if (k.scramble)
            for (size_t j = 0; j < N; ++j) sent[j] ^= (uint8_t)((kScrambleWord >> (31 - (j & 31))) & 1u);
        uint8_t *out = tx + f * tx_pitch;
        for (size_t y = 0; y < nsym; ++y) {
            unsigned sym = 0;
            for (unsigned b = 0; b < bps; ++b) sym = (sym << 1) | sent[y * bps + b];
            out[y] = (uint8_t)sym;
        }
    }
}

void pkt_decode_host(const Packetizer &k, const uint8_t *soft, size_t soft_pitch, size_t F, uint8_t *payload,
                     size_t payload_pitch, uint8_t *valid, uint32_t *crc, uint32_t *metric) {
    const size_t n = k.n, w = k.w(), N = k.N();
    std::vector<uint8_t> msg(n + w), ordered(N);
    std::vector<uint32_t> pi(N);
    pkt_permutation(N, k.columns, pi.data());
    for (size_t f = 0; f < F; ++f) {
        const uint8_t *in = soft + f * soft_pitch;
        for (size_t i = 0; i < N; ++i) {
            const size_t j = pi[i];
            const bool m = k.scramble && ((kScrambleWord >> (31 - (j & 31))) & 1u);
            ordered[i] = m ? (uint8_t)(255 - in[j]) : in[j];
        }
        uint32_t pm = 0;
        conv_decode_host(k.code, ordered.data(), N, k.msg_bits(), 1, msg.data(), n + w, &pm);
        std::copy(msg.begin(), msg.begin() + n, payload + f * payload_pitch);
        const uint32_t v = crc_host(k.crc, msg.data(), n);
        uint32_t field = 0;
        for (size_t i = 0; i < w; ++i) field = (field << 8) | msg[n + i];
        valid[f] = v == field;
        if (crc) crc[f] = v;
        if (metric) metric[f] = pm;
    }
}

}  // namespace yagi
