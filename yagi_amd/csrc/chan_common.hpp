// chan_common.hpp -- what the channelizer translation units (chan_kernels.hip, chanr_kernels.hip) share: the mixed-radix
// LDS transform over a tile of frames, the history-or-block sample load and the LDS layout of the column kernels.
#pragma once

#include "fft_radix.hpp"
#include "kernels.hpp"

namespace yagi {

// Cache policy of the analyzers' streamed accesses (interleaved A/B, profiles/r03_notes.md): sample loads sc1 (L1
// bypassed) -1.4 ... -1.6 %; channel stores stay plain -- their 64- to 128-byte runs per wave instruction lose 2.8 ... 3.6 %
// as non-temporal stores (the synthesizers, whose stores are whole lines, gain 2 % and use the library default).
constexpr int kAnaLoad = kStreamLoad, kAnaStore = 0;

struct FacList { int n; int f[16]; };

static FacList factorize_small(int n) {
    FacList L{0, {0}};
    while (n % 4 == 0) { L.f[L.n++] = 4; n /= 4; }
    for (int p : {2, 3, 5, 7}) while (n % p == 0) { L.f[L.n++] = p; n /= p; }
    for (int p = 11; n > 1 && L.n < 15; p += 2) while (n % p == 0 && L.n < 15) { L.f[L.n++] = p; n /= p; }
    if (n > 1) L.f[L.n++] = n;
    return L;
}

// nfr independent N-point DFTs stored [frame][N] in LDS buffer `src`; result buffer returned.
// tw = W_Mtab^m table (forward sign), N * tw_scale == Mtab; conj => inverse transform.
// Radices 2/3/4/5/7 run as register butterflies (fft_radix.hpp), any other prime factor as direct sums.
template <bool CONJ>
__device__ __forceinline__ float2 *lds_dft_frames_t(float2 *src, float2 *dst, int N, int nfr,
                                                    const FacList &fl, const float2 *__restrict__ tw,
                                                    int tw_scale) {
    constexpr int SIGN = CONJ ? +1 : -1;
    int Ns = 1;
    const int total = N * nfr;
    for (int f = 0; f < fl.n; ++f) {
        const int R = fl.f[f];
        const int T = N / R;
        const int tw_k = N / (Ns * R);
        switch (R) {
            case 2: stockham_pass_any<2, SIGN>(src, dst, N, Ns, nfr, tw, tw_scale, CONJ); break;
            case 3: stockham_pass_any<3, SIGN>(src, dst, N, Ns, nfr, tw, tw_scale, CONJ); break;
            case 4: stockham_pass_any<4, SIGN>(src, dst, N, Ns, nfr, tw, tw_scale, CONJ); break;
            case 5: stockham_pass_any<5, SIGN>(src, dst, N, Ns, nfr, tw, tw_scale, CONJ); break;
            case 7: stockham_pass_any<7, SIGN>(src, dst, N, Ns, nfr, tw, tw_scale, CONJ); break;
            default:
                for (int e = threadIdx.x; e < total; e += blockDim.x) {
                    const int fr = e / N, idx = e - fr * N;
                    const int q = idx / T, j = idx - q * T;
                    const int k = j % Ns;
                    const int step = (k * tw_k + q * T) % N;
                    const float2 *s = src + fr * N;
                    float2 acc = s[j];
                    int m = 0;
                    for (int r = 1; r < R; ++r) {
                        m += step;
                        if (m >= N) m -= N;
                        float2 w = tw[m * tw_scale];
                        if (CONJ) w.y = -w.y;
                        acc = cadd(acc, cmul(s[j + r * T], w));
                    }
                    dst[fr * N + (j / Ns) * Ns * R + k + q * Ns] = acc;
                }
        }
        __syncthreads();
        float2 *t = src; src = dst; dst = t;
        Ns *= R;
    }
    return src;
}
__device__ __forceinline__ float2 *lds_dft_frames(float2 *src, float2 *dst, int N, int nfr,
                                                  const FacList &fl, const float2 *__restrict__ tw,
                                                  int tw_scale, bool conj) {
    return conj ? lds_dft_frames_t<true>(src, dst, N, nfr, fl, tw, tw_scale)
                : lds_dft_frames_t<false>(src, dst, N, nfr, fl, tw, tw_scale);
}

__device__ __forceinline__ float2 load_hist(const float2 *__restrict__ hist, int hist_len,
                                            const float2 *__restrict__ x, long long idx, long long x_len) {
    if (idx >= 0) return (idx < x_len) ? x[idx] : make_float2(0.f, 0.f);
    const long long h = hist_len + idx;
    return (h >= 0) ? hist[h] : make_float2(0.f, 0.f);
}

// LDS slot pitch of one transform in the column kernels: M + 32/nq for nq <= 32 transforms in flight
// (fft_radix.hpp), M + 1 (odd: the lanes of a pass, one transform apart, cover all banks) beyond
__host__ __device__ constexpr int col_pitch(int M, int nq) { return M + (nq <= 32 ? 32 / nq : 1); }
constexpr int kColTile = 16;
constexpr int kColHalf = 8;
constexpr size_t kColWgs = 1024;               // workgroups a launch aims for: four per CU

static constexpr size_t kChanLdsBudget = 38 * 1024;   // <= 4 workgroups per CU

static bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace yagi
