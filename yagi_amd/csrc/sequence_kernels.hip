// sequence_kernels.hip -- MSequence and BSequence (src/sequence/msequence.rs, bsequence.rs): the LFSR generator's block
// forms and the sliding bit correlator.  Everything here is integer arithmetic, so every output equals the reference's
// sequential loop bit for bit.
//
// MSequence.  advance() (msequence.rs:116-122) is  b = parity(state & g); state = ((state << 1) | b) & n,  which is
// linear over GF(2) on the 32-bit state word whatever m, g and the state hold: T(a ^ b) == T(a) ^ T(b).  T is kept as
// 32 column words (column j = T(1 << j)), applying it is the xor of the columns of the state's set bits, and
// T^(2^(b+1)) is T^(2^b) applied to its own columns.  The object holds T^(2^b) for b = 0 .. 63 (msequence_tables), so
// the state after any number k of steps is reached by the matrices of k's set bits (msequence_skip): O(log k).
//
// msequence_gen_kernel<BPS>: a workgroup of 256 lanes owns kMseqTile consecutive symbols of BPS bits, a lane
// kMseqRun consecutive ones.  The steps in front of a wave's first symbol are the same for its 64 lanes, so that jump
// runs on wave-uniform values (scalar registers, the matrices through scalar loads).  A lane then adds its own
// lane * kMseqRun * BPS steps with the six per-object, per-BPS lane-stride matrices T^(kMseqRun * BPS * 2^b): every
// lane applies all six and keeps the result where bit b of its lane number is set.  Only the columns that can be set
// are visited: after the first step a state has m bits, so `cols` is m unless the start state has bits above m - 1.
// From there the lane steps serially, packs its symbols into words and leaves them in LDS; the tile goes out as 16-byte
// stores where y allows and byte by byte otherwise (an unaligned y, the last tile).
//
// BSequence.  push_correlate_block is a sliding XNOR-popcount over a bit stream: q's window followed by the bits of the
// new symbols, MSB first.  The stream is packed into 32-bit words with the earlier bit in the higher position, which
// is the reference's own word layout (word 0 oldest, the newest bit at bit 0 of the top word).  With 32 W - N zero
// bits in front (W = the word count), packed words 0 .. W-1 ARE q's words and symbol i sits at bits
// [32 W + i bps, 32 W + (i + 1) bps).  The window after symbol i ends (exclusive) at e = 32 W + (i + 1) bps; with
// a = e / 32 and r = e % 32 its word j is the funnel shift  (packed[a - W + j] : packed[a - W + j + 1]) << r  (upper
// half), and word 0 is masked with q's top-word mask.  rxy = sum of popcount(~(ref[j] ^ window[j])) - (32 -
// ref.num_bits_msb), bsequence.rs:137-150 with ref as the receiver.
//
// bsequence_corr_kernel: a workgroup of 256 lanes owns kBseqTile consecutive outputs.  It stages the symbol bytes its
// packed words are made of in LDS (aligned 32-bit loads inside the block, single bytes at its ends), a lane then packs
// whole words (q's words below W, symbols above), and consecutive lanes take consecutive outputs: one LDS read, one
// funnel shift, one xor and one bit count per 32 window bits, ref's words through wave-uniform (scalar) loads.  The
// last workgroup writes the window the call leaves into the other of q's two state buffers.
//
// Every global access is guarded: sym is read in [0, n), y / rxy written in [0, n), the state words in [0, W).
#include <algorithm>
#include <cstdint>

#include "kernels.hpp"

namespace yagi {

// the matrix (32 column words) applied to s; only columns below `cols` are visited
__host__ __device__ __forceinline__ unsigned mseq_apply(const unsigned *__restrict__ M, unsigned s, int cols) {
    unsigned acc = 0u;
    for (int j = 0; j < cols; ++j) acc ^= (0u - ((s >> j) & 1u)) & M[j];
    return acc;
}

namespace {

constexpr int kMW = kMseqWg;
constexpr int kMT = kMseqTile;
constexpr int kMR = kMseqRun;
static_assert(kMT == kMW * kMR && kMW == 256 && kMR % 16 == 0, "a lane leaves whole uint4; four waves of 64 lanes");

template <int BPS>
__global__ void __launch_bounds__(kMW) msequence_gen_kernel(const unsigned *__restrict__ pow,
                                                            const unsigned *__restrict__ stride, unsigned s0,
                                                            unsigned g, unsigned nmask, int cols, size_t n,
                                                            uint8_t *__restrict__ y) {
    __shared__ __attribute__((aligned(16))) unsigned s_out[kMT / 4];

    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const size_t t0 = (size_t)blockIdx.x * kMT;
    const int cnt = (int)std::min((size_t)kMT, n - t0);

    // the steps in front of this wave's first symbol: wave-uniform
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned long long off = ((unsigned long long)t0 + (unsigned long long)wave * (64u * kMR)) * (unsigned)BPS;
    unsigned s = s0;
    for (int b = 0; off != 0; ++b, off >>= 1)
        if (off & 1u) s = mseq_apply(pow + 32 * b, s, cols);
    // the lane's own lane * kMR * BPS steps
#pragma unroll
    for (int b = 0; b < kMseqStrides; ++b) {
        const unsigned t = mseq_apply(stride + 32 * b, s, cols);
        s = ((lane >> b) & 1) ? t : s;
    }

    unsigned w[kMR / 4];
#pragma unroll
    for (int i = 0; i < kMR; ++i) {
        unsigned sym = 0u;
#pragma unroll
        for (int k = 0; k < BPS; ++k) {
            const unsigned bit = (unsigned)__popc(s & g) & 1u;
            s = ((s << 1) | bit) & nmask;
            sym = (sym << 1) | bit;
        }
        w[i / 4] = (i % 4 == 0) ? sym : (w[i / 4] | (sym << (8 * (i % 4))));
    }
    {
        uint4 *row = reinterpret_cast<uint4 *>(s_out + tid * (kMR / 4));
#pragma unroll
        for (int v = 0; v < kMR / 16; ++v) row[v] = make_uint4(w[4 * v], w[4 * v + 1], w[4 * v + 2], w[4 * v + 3]);
    }
    __syncthreads();

    uint8_t *yt = y + t0;
    if (cnt == kMT && (reinterpret_cast<uintptr_t>(yt) & 15u) == 0) {
        const uint4 *src = reinterpret_cast<const uint4 *>(s_out);
        uint4 *dst = reinterpret_cast<uint4 *>(yt);
        for (int q = tid; q < kMT / 16; q += kMW) dst[q] = src[q];
    } else {
        const uint8_t *src = reinterpret_cast<const uint8_t *>(s_out);
        for (int i = tid; i < cnt; i += kMW) yt[i] = src[i];
    }
}

constexpr int kBW = kBseqWg;
constexpr int kBT = kBseqTile;

__device__ __forceinline__ unsigned bseq_funnel(unsigned hi, unsigned lo, unsigned r) {      // ((hi : lo) << r) >> 32
    return __funnelshift_l(lo, hi, r);
}

__global__ void __launch_bounds__(kBW) bsequence_corr_kernel(const unsigned *__restrict__ cur,
                                                             unsigned *__restrict__ next,
                                                             const unsigned *__restrict__ ref,
                                                             const uint8_t *__restrict__ sym, size_t n, int bps, int W,
                                                             unsigned qmask, int corr, int *__restrict__ rxy,
                                                             unsigned tile0, unsigned last_tile) {
    __shared__ unsigned s_pk[kBseqPackedWords];
    __shared__ __attribute__((aligned(4))) uint8_t s_sym[kBseqSymBytes];

    const int tid = (int)threadIdx.x;
    const size_t tile = (size_t)blockIdx.x + tile0;
    const size_t t0 = tile * kBT;
    const int cnt = (int)std::min((size_t)kBT, n - t0);
    const size_t ubps = (size_t)bps, uW = (size_t)W;

    // packed words [wlo, whi] of the padded stream serve this tile's windows
    const size_t wlo = ((t0 + 1) * ubps) >> 5;
    const size_t whi = uW + (((t0 + (size_t)cnt) * ubps) >> 5);
    const int nw = (int)(whi - wlo) + 1;
    // the symbols under the words at and above W
    const size_t g0 = std::max(wlo, uW) - uW;
    const size_t s_lo = std::min(n, (g0 * 32) / ubps);
    const size_t s_hi = std::min(n, ((whi - uW + 1) * 32 + ubps - 1) / ubps);
    const uint8_t *p = sym + s_lo;
    const int nb = (int)(s_hi - s_lo);
    const int mis = (int)(reinterpret_cast<uintptr_t>(p) & 3u);     // s_sym[mis + i] = p[i]: aligned words stay aligned
    {
        const int total = mis + nb;
        const int jlo = (mis + 3) >> 2, jhi = total >> 2;           // the aligned words that lie inside [p, p + nb)
        if (jhi > jlo) {
            const unsigned *pw = reinterpret_cast<const unsigned *>(p - mis);
            unsigned *sw = reinterpret_cast<unsigned *>(s_sym);
            for (int j = jlo + tid; j < jhi; j += kBW) sw[j] = pw[j];
            for (int i = mis + tid; i < 4 * jlo; i += kBW) s_sym[i] = p[i - mis];
            for (int i = 4 * jhi + tid; i < total; i += kBW) s_sym[i] = p[i - mis];
        } else {
            for (int i = mis + tid; i < total; i += kBW) s_sym[i] = p[i - mis];
        }
    }
    __syncthreads();

    const unsigned smask = (1u << bps) - 1u;
    for (int k = tid; k < nw; k += kBW) {
        const size_t gw = wlo + (size_t)k;
        unsigned word;
        if (gw < uW) {
            word = cur[gw];
        } else {
            // a 64-bit accumulator over the stream positions [sb0 - 16, sb0 + 48): the symbol whose first bit is at
            // sb0 + pos, -bps < pos < 32, lands with its last bit at bit 48 - pos - bps
            const size_t sb0 = (gw - uW) * 32;
            size_t i = sb0 / ubps;
            int pos = (int)((long long)(i * ubps) - (long long)sb0);
            unsigned long long acc = 0ull;
            for (; pos < 32 && i < s_hi; ++i, pos += bps)
                acc |= (unsigned long long)(s_sym[mis + (int)(i - s_lo)] & smask) << (48 - pos - bps);
            word = (unsigned)(acc >> 16);
        }
        s_pk[k] = word;
    }
    __syncthreads();

    if (rxy != nullptr) {
        for (int o = tid; o < cnt; o += kBW) {
            const size_t e = uW * 32 + (t0 + (size_t)o + 1) * ubps;
            const unsigned r = (unsigned)(e & 31u);
            const int kb = (int)((e >> 5) - uW - wlo);              // window word j = s_pk[kb + j] : s_pk[kb + j + 1]
            unsigned hi = s_pk[kb], lo = s_pk[kb + 1];
            int diff = __popc((bseq_funnel(hi, lo, r) & qmask) ^ ref[0]);
            hi = lo;
#pragma unroll 4
            for (int j = 1; j < W; ++j) {
                lo = s_pk[kb + j + 1];
                diff += __popc(bseq_funnel(hi, lo, r) ^ ref[j]);
                hi = lo;
            }
            rxy[t0 + (size_t)o] = corr - diff;
        }
    }
    // the window the call leaves
    if (tile == (size_t)last_tile) {
        const size_t e = uW * 32 + n * ubps;
        const unsigned r = (unsigned)(e & 31u);
        const int kb = (int)((e >> 5) - uW - wlo);
        for (int j = tid; j < W; j += kBW) {
            const unsigned w = bseq_funnel(s_pk[kb + j], s_pk[kb + j + 1], r);
            next[j] = j == 0 ? (w & qmask) : w;
        }
    }
}

}  // namespace

void msequence_tables(unsigned g, unsigned nmask, unsigned *pow, unsigned *stride) {
    for (int j = 0; j < 32; ++j) {                                  // T itself: advance() on every unit vector
        const unsigned s = 1u << j;
        pow[j] = ((s << 1) | ((unsigned)__builtin_popcount(s & g) & 1u)) & nmask;
    }
    for (int b = 1; b < kMseqPowers; ++b)
        for (int j = 0; j < 32; ++j) pow[32 * b + j] = mseq_apply(pow + 32 * (b - 1), pow[32 * (b - 1) + j], 32);
    for (int bps = 1; bps <= 8; ++bps)
        for (int b = 0; b < kMseqStrides; ++b) {
            unsigned *S = stride + 32 * ((bps - 1) * kMseqStrides + b);
            for (int j = 0; j < 32; ++j) S[j] = msequence_skip(pow, 1u << j, (uint64_t)(kMR * bps) << b);
        }
}

unsigned msequence_skip(const unsigned *pow, unsigned s, uint64_t k) {
    for (int b = 0; k != 0; ++b, k >>= 1)
        if (k & 1u) s = mseq_apply(pow + 32 * b, s, 32);
    return s;
}

int launch_msequence_gen(const unsigned *pow, const unsigned *stride, unsigned s0, unsigned g, unsigned nmask, int m,
                         int bps, size_t n, uint8_t *y, hipStream_t st) {
    if (n == 0) return YAGI_OK;
    if (bps < 1 || bps > 8) return fail(YAGI_ERR_INTERNAL, "msequence: bps out of range");
    const size_t tiles = (n + kMT - 1) / kMT;
    if (tiles > 0x7fffffffu) return fail(YAGI_ERR_CONFIG, "msequence: block too long (%zu symbols)", n);
    const int cols = (m < 32 && (s0 >> m) != 0u) ? 32 : m;          // a start state with bits above m - 1 reaches them
    const unsigned *S = stride + 32 * ((bps - 1) * kMseqStrides);
    switch (bps) {
#define YG_MSEQ(B) case B: msequence_gen_kernel<B><<<(unsigned)tiles, kMW, 0, st>>>(pow, S, s0, g, nmask, cols, n, y); break;
        YG_MSEQ(1) YG_MSEQ(2) YG_MSEQ(3) YG_MSEQ(4) YG_MSEQ(5) YG_MSEQ(6) YG_MSEQ(7) YG_MSEQ(8)
#undef YG_MSEQ
    }
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

int launch_bsequence_corr(const unsigned *cur, unsigned *next, const unsigned *ref, int W, unsigned qmask,
                          int ref_bits_msb, const uint8_t *sym, size_t n, int bps, int *rxy, hipStream_t st) {
    if (n == 0) return YAGI_OK;
    if (bps < 1 || bps > 8 || W < 1 || W > kBseqNmax / 32) return fail(YAGI_ERR_INTERNAL, "bsequence: (bps, words) out of range");
    const size_t tiles = (n + kBT - 1) / kBT;
    if (tiles > 0x7fffffffu) return fail(YAGI_ERR_CONFIG, "bsequence: block too long (%zu symbols)", n);
    const int corr = 32 * W - (32 - ref_bits_msb);
    const unsigned last = (unsigned)(tiles - 1);
    // without rxy only the last tile has anything to do: the window the call leaves
    const unsigned tile0 = rxy ? 0u : last;
    bsequence_corr_kernel<<<(unsigned)tiles - tile0, kBW, 0, st>>>(cur, next, ref, sym, n, bps, W, qmask, corr, rxy, tile0, last);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

}  // namespace yagi
