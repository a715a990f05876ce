// ordfilt_kernels.hip -- OrdFilt (src/filter/ordfilt.rs): the rank-k sample of every window of n samples over a block.
//
// The reference sorts a copy of its window for every sample (stable sort under partial_cmp) and returns element k.  A
// block needs no sort: under a total order with ties broken by age, sample s of a window has the rank
//     #{l older than s : key[l] <= key[s]}  +  #{l newer than s : key[l] < key[s]},
// which is a permutation of 0 .. n-1 over the window, so exactly one sample has rank k.  When the window slides by one
// sample, the rank of a sample that stays changes by one compare against the sample that leaves (always older: `<=`)
// and one against the sample that enters (always newer: `<`).
//
// The order (ordfilt_key): the f32 bits mapped to a u32 that is monotone in the value -- negative floats bit-inverted,
// non-negative ones with the top bit set -- after -0.0 is folded onto +0.0, which compare equal in the reference too.
// For windows without NaN this is partial_cmp exactly, signed zeros and their age order included.  NaN, which the
// reference leaves unspecified, sorts above +inf with the sign bit clear and below -inf with it set (yagi_hip.h).
//
// ordfilt_rank_kernel: a workgroup of 256 lanes owns kOrdfiltTile consecutive outputs.  It stages the keys of those
// samples and of the n - 1 before them (from x, or from the object's history in front of x[0]) in LDS, plus one bit per
// sample that says "this was -0.0", the only thing the key does not keep.  Lane t then takes the candidates t, t + 256,
// ...: n - 1 compares give the candidate's rank in the first window of the tile that holds it, and it walks the at most
// n windows that hold it with two compares each; where its rank is k it writes its own bits into the tile's output slot
// in LDS.  Lanes at consecutive candidates read consecutive LDS words in every step, so no access has a bank conflict;
// one candidate per window matches, so no slot is written twice and none is left out.  The tile leaves as 16-byte
// stores where y allows, and the last workgroup writes the window the call leaves (the last n samples of history + x)
// into the other of the object's two history buffers.
//
// ordfilt_reg_kernel<N> (2 <= N <= kOrdfiltRegNmax) is the register-resident form of the same scheme, described at the
// kernel; launch_ordfilt takes it up to kOrdfiltRegCrossover (kernels.hpp) unless a form is forced.  Both forms give the
// same bits (tests/test_gpu_ordfilt.py).
//
// Every global access is guarded by the block length: x is read in [0, n_block), y written in [0, n_block).
#include <algorithm>
#include <cstdint>

#include "kernels.hpp"

namespace yagi {
namespace {

constexpr int kWg = kOrdfiltWg;
constexpr int kT = kOrdfiltTile;
constexpr int kStage = kT + kOrdfiltNmax - 1;          // samples a tile can need: its outputs and the halo in front
constexpr int kPerLane = kStage / kWg;                  // staged samples per lane
static_assert(kStage % kWg == 0 && kWg % 64 == 0 && kT % (4 * kWg) == 0,
              "whole waves stage the samples (one -0.0 bit each); the tile leaves as uint4");

__host__ __device__ __forceinline__ unsigned ordfilt_key(unsigned u) {
    if (u == 0x80000000u) u = 0u;                       // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the bits a key came from, up to the sign of a zero
__device__ __forceinline__ unsigned ordfilt_unkey(unsigned key) {
    return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
}

__global__ void __launch_bounds__(kWg) ordfilt_rank_kernel(const unsigned *__restrict__ hist,
                                                           unsigned *__restrict__ hist_next,
                                                           const unsigned *__restrict__ x, size_t nb,
                                                           unsigned *__restrict__ y, int n, int k) {
    __shared__ unsigned s_key[kStage];
    __shared__ __attribute__((aligned(16))) unsigned s_out[kT];
    __shared__ unsigned s_negz[kStage / 32];

    const int tid = (int)threadIdx.x;
    const size_t t0 = (size_t)blockIdx.x * kT;
    const int cnt = (int)std::min((size_t)kT, nb - t0);             // outputs of this tile
    const int halo = n - 1;
    const int W = cnt + halo;                                       // staged samples; sample p is x[t0 + p - halo]

    // all of a lane's loads are issued before the first is used
    unsigned u[kPerLane];
#pragma unroll
    for (int c = 0; c < kPerLane; ++c) {
        const int p = tid + c * kWg;
        const long long g = (long long)t0 + (long long)(p - halo);
        u[c] = 0u;
        if (p < W) u[c] = g >= 0 ? x[g] : hist[(long long)n + g];   // hist = the n samples before x[0], oldest first
    }
#pragma unroll
    for (int c = 0; c < kPerLane; ++c) {
        const int p = tid + c * kWg;
        if (c * kWg < W) {                                          // the same for every lane of the workgroup
            if (p < W) s_key[p] = ordfilt_key(u[c]);
            const unsigned long long nz = __ballot(p < W && u[c] == 0x80000000u);
            if ((tid & 31) == 0) s_negz[p >> 5] = (unsigned)(nz >> (tid & 32));
        }
    }
    // the window the call leaves
    if (blockIdx.x == gridDim.x - 1) {
        for (int j = tid; j < n; j += kWg) {
            const long long g = (long long)nb - (long long)n + j;
            hist_next[j] = g >= 0 ? x[g] : hist[(long long)j + (long long)nb];
        }
    }
    __syncthreads();

    for (int p = tid; p < W; p += kWg) {
        const unsigned kp = s_key[p];
        const int i0 = std::max(p - halo, 0);                       // the windows [i0, i1] of the tile hold sample p;
        const int i1 = std::min(p, cnt - 1);                        // window i is the staged samples [i, i + halo]
        unsigned raw = ordfilt_unkey(kp);
        if ((s_negz[p >> 5] >> (p & 31)) & 1u) raw = 0x80000000u;
        int r = 0;
        for (int l = i0; l < p; ++l) r += (s_key[l] <= kp) ? 1 : 0;
        for (int l = p + 1; l <= i0 + halo; ++l) r += (s_key[l] < kp) ? 1 : 0;
        if (r == k) s_out[i0] = raw;
        for (int i = i0 + 1; i <= i1; ++i) {
            r -= (s_key[i - 1] <= kp) ? 1 : 0;
            r += (s_key[i + halo] < kp) ? 1 : 0;
            if (r == k) s_out[i] = raw;
        }
    }
    __syncthreads();

    unsigned *yt = y + t0;
    if (cnt == kT && (reinterpret_cast<uintptr_t>(yt) & 15u) == 0) {
        const uint4 *src = reinterpret_cast<const uint4 *>(s_out);
        uint4 *dst = reinterpret_cast<uint4 *>(yt);
        for (int q = tid; q < kT / 4; q += kWg) dst[q] = src[q];
    } else {
        for (int i = tid; i < cnt; i += kWg) yt[i] = s_out[i];
    }
}

// ordfilt_reg_kernel<N>: the register-resident form for short windows, same tile.  The raw samples are staged in LDS in
// rows of kRegR words padded to kRegRow, so that the 16-byte reads of any 16 lanes at consecutive rows cover all 64
// banks.  Lane t owns the kRegR consecutive outputs of row t and holds the bits and keys of their kRegR + N - 1 samples
// (its row and the head of the next) in registers.  Every sample gets its first rank (N - 1 compares) and walks the
// windows OF THIS LANE that hold it, two compares and one select each; every index is a compile-time constant, so
// nothing is addressed dynamically.  Samples past the block's end are staged as zeros: they belong only to windows past
// the end, which are not stored.
constexpr int kRegR = kT / kWg;                          // outputs per lane
constexpr int kRegRow = kRegR + 4;                       // LDS row stride in words
constexpr int kRegRows = kWg + 1;                        // a tile's rows and the one the last lane's halo is in
static_assert(kRegR == 16 && kOrdfiltRegNmax - 1 <= kRegR, "a lane reads four uint4 of its row and the head of the next");

template <int N>
__global__ void __launch_bounds__(kWg) ordfilt_reg_kernel(const unsigned *__restrict__ hist,
                                                          unsigned *__restrict__ hist_next,
                                                          const unsigned *__restrict__ x, size_t nb,
                                                          unsigned *__restrict__ y, int k) {
    constexpr int halo = N - 1;
    constexpr int C = kRegR + halo;                                 // samples a lane holds
    constexpr int kStaged = kRegRows * kRegR;                       // samples staged: every row a lane reads is filled
    __shared__ __attribute__((aligned(16))) unsigned s_raw[kRegRows * kRegRow];

    const int tid = (int)threadIdx.x;
    const size_t t0 = (size_t)blockIdx.x * kT;
    const int cnt = (int)std::min((size_t)kT, nb - t0);
    const int W = cnt + halo;                                       // sample p is x[t0 + p - halo]

    unsigned u[(kStaged + kWg - 1) / kWg];
#pragma unroll
    for (int c = 0; c < (kStaged + kWg - 1) / kWg; ++c) {
        const int p = tid + c * kWg;
        const long long g = (long long)t0 + (long long)(p - halo);
        u[c] = 0u;
        if (p < W) u[c] = g >= 0 ? x[g] : hist[(long long)N + g];
    }
#pragma unroll
    for (int c = 0; c < (kStaged + kWg - 1) / kWg; ++c) {
        const int p = tid + c * kWg;
        if (p < kStaged) s_raw[(p / kRegR) * kRegRow + (p % kRegR)] = u[c];
    }
    if (blockIdx.x == gridDim.x - 1) {
        for (int j = tid; j < N; j += kWg) {
            const long long g = (long long)nb - (long long)N + j;
            hist_next[j] = g >= 0 ? x[g] : hist[(long long)j + (long long)nb];
        }
    }
    __syncthreads();

    unsigned raw[kRegR + kRegR], key[C];
    {
        const uint4 *row = reinterpret_cast<const uint4 *>(s_raw + tid * kRegRow);
#pragma unroll
        for (int v = 0; v < kRegR / 4 + (halo + 3) / 4; ++v) {
            const uint4 w = v < kRegR / 4 ? row[v] : row[kRegRow / 4 + (v - kRegR / 4)];
            raw[4 * v] = w.x;
            raw[4 * v + 1] = w.y;
            raw[4 * v + 2] = w.z;
            raw[4 * v + 3] = w.w;
        }
    }
#pragma unroll
    for (int j = 0; j < C; ++j) key[j] = ordfilt_key(raw[j]);
    __syncthreads();                                                // the rows are read: the outputs go where they were

    unsigned out[kRegR];
#pragma unroll
    for (int i = 0; i < kRegR; ++i) out[i] = 0u;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const int i0 = j - halo > 0 ? j - halo : 0;                 // the lane's windows [i0, i1] hold sample j;
        const int i1 = j < kRegR - 1 ? j : kRegR - 1;               // window i is the samples [i, i + halo]
        const unsigned kj = key[j];
        int r = 0;
#pragma unroll
        for (int l = 0; l < C; ++l) {
            if (l >= i0 && l < j) r += (key[l] <= kj) ? 1 : 0;
            if (l > j && l <= i0 + halo) r += (key[l] < kj) ? 1 : 0;
        }
#pragma unroll
        for (int i = 0; i < kRegR; ++i) {
            if (i > i0 && i <= i1) {
                r -= (key[i - 1] <= kj) ? 1 : 0;
                r += (key[i + halo] < kj) ? 1 : 0;
            }
            if (i >= i0 && i <= i1) out[i] = r == k ? raw[j] : out[i];
        }
    }

    {
        uint4 *row = reinterpret_cast<uint4 *>(s_raw + tid * kRegRow);
#pragma unroll
        for (int v = 0; v < kRegR / 4; ++v) row[v] = make_uint4(out[4 * v], out[4 * v + 1], out[4 * v + 2], out[4 * v + 3]);
    }
    __syncthreads();

    unsigned *yt = y + t0;
    if (cnt == kT && (reinterpret_cast<uintptr_t>(yt) & 15u) == 0) {
        uint4 *dst = reinterpret_cast<uint4 *>(yt);
        for (int q = tid; q < kT / 4; q += kWg)
            dst[q] = *reinterpret_cast<const uint4 *>(s_raw + (q / (kRegR / 4)) * kRegRow + (q % (kRegR / 4)) * 4);
    } else {
        for (int i = tid; i < cnt; i += kWg) yt[i] = s_raw[(i / kRegR) * kRegRow + (i % kRegR)];
    }
}

template <int N>
void ordfilt_reg_launch(unsigned tiles, const unsigned *hist, unsigned *hist_next, const unsigned *x, size_t nb,
                        unsigned *y, int k, hipStream_t st) {
    ordfilt_reg_kernel<N><<<tiles, kWg, 0, st>>>(hist, hist_next, x, nb, y, k);
}

}  // namespace

float ordfilt_host_select(const float *win, int n, int k, std::vector<std::pair<unsigned, unsigned>> &tmp) {
    tmp.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        unsigned u;
        std::memcpy(&u, win + i, sizeof(u));
        tmp[(size_t)i] = {ordfilt_key(u), u};
    }
    std::stable_sort(tmp.begin(), tmp.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    float v;
    std::memcpy(&v, &tmp[(size_t)k].second, sizeof(v));
    return v;
}

int launch_ordfilt(int n, int k, int form, const float *hist, float *hist_next, const float *x, size_t nb, float *y,
                   hipStream_t st) {
    if (nb == 0) return YAGI_OK;
    if (n < 1 || n > kOrdfiltNmax || k < 0 || k >= n) return fail(YAGI_ERR_INTERNAL, "ordfilt: (n, k) out of range");
    const size_t tiles = (nb + kT - 1) / kT;
    if (tiles > 0x7fffffffu) return fail(YAGI_ERR_CONFIG, "ordfilt: block too long (%zu samples)", nb);
    if (form == ORDFILT_AUTO) form = (n >= 2 && n <= kOrdfiltRegCrossover) ? ORDFILT_REG : ORDFILT_LDS;
    const unsigned *h = reinterpret_cast<const unsigned *>(hist), *xu = reinterpret_cast<const unsigned *>(x);
    unsigned *hn = reinterpret_cast<unsigned *>(hist_next), *yu = reinterpret_cast<unsigned *>(y);
    if (form == ORDFILT_REG) {
        switch (n) {
#define YG_ORDFILT_REG(N) case N: ordfilt_reg_launch<N>((unsigned)tiles, h, hn, xu, nb, yu, k, st); break;
            YG_ORDFILT_REG(2) YG_ORDFILT_REG(3) YG_ORDFILT_REG(4) YG_ORDFILT_REG(5)
            YG_ORDFILT_REG(6) YG_ORDFILT_REG(7) YG_ORDFILT_REG(8) YG_ORDFILT_REG(9)
#undef YG_ORDFILT_REG
            default: return fail(YAGI_ERR_CONFIG, "ordfilt: the register form serves 2 <= n <= %d", kOrdfiltRegNmax);
        }
    } else if (form == ORDFILT_LDS) {
        ordfilt_rank_kernel<<<(unsigned)tiles, kWg, 0, st>>>(h, hn, xu, nb, yu, n, k);
    } else {
        return fail(YAGI_ERR_CONFIG, "ordfilt: unknown kernel form %d", form);
    }
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

}  // namespace yagi
