// pdet_kernels.hip -- PreambleDetector (yagi_hip.h): a bank of K correlators against a known preamble of L
// samples, one per carrier-offset hypothesis, the normalised threshold
//     hit[n] = energy[n] > energy_floor && m[n] > fl(thr2 q[n]),  m = the largest fl(fl(re^2) + fl(im^2)) of rxy_k[n] (the
//     lowest k on ties),  q = fl(energy[n] ep)
// and the extraction of runs of hits and their peaks (the largest r = m / q, the earliest on ties) in two launches that
// read the samples and write only events.
//
// Rounding points.  rxy_k[n] = sum_i w[i] v_k[i] over i = 0 .. L-1 from +0.0, w[i] = X[n - L + 1 + i], the product
// num-complex's: re += fl(w.re v.re) - fl(w.im v.im), im += fl(w.re v.im) + fl(w.im v.re), every product, difference and
// add rounded on its own.  energy[n] is Autocorr(L, 0)'s: the sum in the same order of fl(fl(w.re^2) + fl(w.im^2)).
//
// pd_tile_bank: a workgroup of 256 lanes owns kPdetTile consecutive outputs.  It stages the span of cnt + L - 1 samples
// the tile needs (it starts L - 1 samples in front of the tile; each sample comes from x or from the object's history in
// front of x[0]) and their energy terms in LDS once, in rows of R padded by 16 bytes, so that the 16 lanes a
// ds_read_b128 serves together, at consecutive rows, cover all 64 banks.  Lane t owns the R consecutive outputs
// t R .. t R + R - 1 and slides a register window of R + 4 staged values along them, four taps of all R outputs per step:
// first over the energy terms (L adds per output), then once per hypothesis over the samples (the staged span is reused
// K times).  The taps of a step are the same for every lane: they are read from the template row at a wave-uniform
// address, 32 bytes per step, which the compiler turns into scalar loads; a step is 256 f32 operations per lane against
// two 16-byte LDS reads.  The window's three groups of four rotate in place (no register is moved).  Every workgroup
// also copies its share of the history the call leaves (the last L samples of history ++ x) into the other of the
// object's two buffers.
//
// pdet_tile_kernel: the bank, then hit and r per output, and from there the segment extraction of runs_common.hpp, as
// in burstdet_tile_kernel: a tile without a hit writes {0, 0} to its slot of the tile table and ends; otherwise
// the lanes' sums go to LDS, where the staged values were, and runs::tile_segments scans the lanes' runs and writes the
// tile's segments to the call's pool.  The hypothesis at a segment's peak rides in the segment's spare word.
//
// pdet_stitch_kernel: runs::stitch over the 48-byte event, as in burstdet_stitch_kernel: one workgroup walks the
// tile table in tile order, joins segments that meet at a tile seam (the pending run of the call before is the first
// run), reports closed runs of min_length or more, and stores position, pending run and a zeroed pool counter.  No
// workgroup waits on another: the second launch is the only ordering.
//
// pdet_correlate_kernel: the bank alone; rxy_k and energy leave as each lane's 64 and 32 contiguous bytes.
//
// r = m / q is IEEE f32 division, formed in f64 and rounded to f32 (runs::ratio says why that is the same value and why
// the f32 expansion is kept out of this file).
//
// Every global access is guarded: x in [0, nb), the history in [0, L), the template rows in [0, K pitch), rxy in
// [0, K nb), energy in [0, nb), the tile table at the workgroup's own slot, the pool below pool_cap, events below cap.
//
// The Makefile builds this file with -ffp-contract=off; tests/test_pdet_isa_cpu.py checks that the kernels hold no f32
// FMA and no scratch.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>

#include "kernels.hpp"
#include "runs_common.hpp"

namespace yagi {
namespace {

typedef float pd_v2f __attribute__((ext_vector_type(2)));
typedef float pd_v4f __attribute__((ext_vector_type(4)));

constexpr int kWg = kPdetWg;
constexpr int kT = kPdetTile;
constexpr int kR = kPdetR;                             // outputs per lane
constexpr int kC = 4;                                  // taps per step of the window
constexpr int kStage = kT + kPdetLmax;                 // staged positions: all a lane's last step can read
constexpr int kRows = kStage / kR;
constexpr int kPerLane = kStage / kWg;
constexpr int kHistWgs = 1024;                         // workgroups that share the copy of the history
constexpr int kWordsV = kRows * (kR * 2 + 4), kWordsE = kRows * (kR + 4);
static_assert(kR == 8 && kT == kWg * kR && kStage % kWg == 0 && kPdetLmax % kC == 0,
              "a lane reads its row as 16-byte words and steps by half a row");
static_assert((size_t)(kWordsV + kWordsE) * sizeof(float) == pdet_lds_bytes(), "kernels.hpp");

// LDS word offset of position p in rows of kR elements of `words` words each, padded by four words
template <int words>
__device__ __forceinline__ int pd_at(int p) {
    return (p / kR) * (kR * words + 4) + (p % kR) * words;
}

// element k of a window of three groups of four, held as 16-byte words
__device__ __forceinline__ pd_v2f pd_sample(const pd_v4f *w, int k) {
    const pd_v4f q = w[k / 2];
    return (k & 1) ? pd_v2f{q.z, q.w} : pd_v2f{q.x, q.y};
}

// which element of the window term t of output r is, where `rot` is the group that holds the window's first four
__device__ __forceinline__ constexpr int pd_slot(int r, int t, int rot) {
    return ((r + t) / kC + rot) % 3 * kC + (r + t) % kC;
}

// The sliding sum's control: `fetch(q, g)` reads the lane's positions q .. q + 3 into group g, `terms(t, rot, c)` adds
// term t (tap 4 c + t) of all R outputs.  Three steps on, the groups are where they were.  L is the same in every lane.
template <class Fetch, class Terms>
__device__ __forceinline__ void pd_slide(int L, Fetch &&fetch, Terms &&terms) {
    auto chunk = [&](int c, int rot) {                              // rot is a constant after inlining
        fetch(kR + kC * c, (rot + 2) % 3);
#pragma unroll
        for (int t = 0; t < kC; ++t) terms(t, rot, c);
    };
    auto rest = [&](int c, int rot, int rem) {
        fetch(kR + kC * c, (rot + 2) % 3);
#pragma unroll
        for (int t = 0; t < kC - 1; ++t) {
            if (t < rem) terms(t, rot, c);
        }
    };
    fetch(0, 0);
    fetch(kC, 1);
    const int full = L / kC, rem = L - full * kC;
    int c = 0;
#pragma unroll 1
    for (; c + 3 <= full; c += 3) {
        chunk(c, 0);
        chunk(c + 1, 1);
        chunk(c + 2, 2);
    }
    const int tail = full - c;                                      // 0, 1 or 2 steps left
    if (tail == 0) {
        if (rem) rest(c, 0, rem);
    } else if (tail == 1) {
        chunk(c, 0);
        if (rem) rest(c + 1, 1, rem);
    } else {
        chunk(c, 0);
        chunk(c + 1, 1);
        if (rem) rest(c + 2, 2, rem);
    }
}

// Lane tid's kR outputs of the tile that starts at output t0 and holds cnt outputs: en[r] the energy, and of the best
// hypothesis bm[r] = m, bz[r] = rxy, bk[r] = its index.  With CORR every hypothesis's rxy and the energy are stored as
// well (outputs below cnt only).  s_lds holds kWordsV + kWordsE words; the caller synchronises the workgroup before it
// reuses them: the staged values are being read until then.
template <bool CORR>
__device__ __forceinline__ void pd_tile_bank(float *s_lds, const cf32 *__restrict__ tmpl, const cf32 *__restrict__ hist,
                                             cf32 *__restrict__ hist_next, const cf32 *__restrict__ x, size_t nb, int L,
                                             int K, size_t t0, int cnt, float (&en)[kR], float (&bm)[kR],
                                             pd_v2f (&bz)[kR], unsigned (&bk)[kR], cf32 *__restrict__ rxy,
                                             float *__restrict__ energy) {
    float *const s_v = s_lds, *const s_e = s_lds + kWordsV;
    const int tid = (int)threadIdx.x;
    const int span = cnt + L - 1;                                   // position p is sample t0 + p - (L - 1)
    const long long H = (long long)L;                               // hist = the H samples before x[0], oldest first
    const pd_v2f *xe = reinterpret_cast<const pd_v2f *>(x), *he = reinterpret_cast<const pd_v2f *>(hist);

    {
        const long long first = (long long)t0 - (long long)(L - 1);
        pd_v2f u[kPerLane];                                         // a lane's loads are issued before the first is used
#pragma unroll
        for (int c = 0; c < kPerLane; ++c) {
            // every lane loads, past the span its last sample again, from an address picked without a branch
            const int p = std::min(tid + c * kWg, span - 1);
            const long long g = first + p;                          // -(L - 1) <= g <= t0 + cnt - 1 < nb
            u[c] = *(g >= 0 ? xe + g : he + (H + g));
        }
#pragma unroll
        for (int c = 0; c < kPerLane; ++c) {
            const int p = tid + c * kWg;
            *reinterpret_cast<pd_v2f *>(s_v + pd_at<2>(p)) = u[c];
            const float er = u[c].x * u[c].x, ei = u[c].y * u[c].y;
            s_e[pd_at<1>(p)] = er + ei;
        }
    }
    // the history the call leaves: the last H samples of hist ++ x, shared among the first kHistWgs workgroups
    if (blockIdx.x < (unsigned)kHistWgs) {
        pd_v2f *hn = reinterpret_cast<pd_v2f *>(hist_next);
        const int step = (int)std::min(gridDim.x, (unsigned)kHistWgs) * kWg;
#pragma unroll 1
        for (int j = (int)blockIdx.x * kWg + tid; j < L; j += step) {
            const long long g = (long long)nb - H + j;
            hn[j] = g >= 0 ? xe[g] : he[(long long)j + (long long)nb];
        }
    }
    __syncthreads();

    const float *rv = s_v + tid * (kR * 2 + 4), *re_ = s_e + tid * (kR + 4);
    [[maybe_unused]] const bool live0 = tid * kR < cnt;                              // the lane has an output inside the block

    // the energy: the sliding sum of the staged terms
    {
        pd_v4f we[3];
#pragma unroll
        for (int r = 0; r < kR; ++r) en[r] = 0.0f;
        pd_slide(
            L, [&](int q, int g) { we[g] = *reinterpret_cast<const pd_v4f *>(re_ + pd_at<1>(q)); },
            [&](int t, int rot, int) {
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    const int k = pd_slot(r, t, rot);
                    en[r] = en[r] + we[k / 4][k % 4];
                }
            });
        if constexpr (CORR) {
            if (energy != nullptr) {
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    if (tid * kR + r < cnt) energy[t0 + (size_t)(tid * kR + r)] = en[r];
                }
            }
        }
    }

    // the bank: one pass over the staged samples per hypothesis
    const size_t pitch = pdet_pitch((size_t)L);
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const pd_v4f *row = reinterpret_cast<const pd_v4f *>(tmpl + (size_t)k * pitch);   // the same in every lane
        pd_v4f wv[6];
        pd_v2f acc[kR];
#pragma unroll
        for (int r = 0; r < kR; ++r) acc[r] = pd_v2f{0.0f, 0.0f};
        pd_slide(
            L,
            [&](int q, int g) {
                wv[2 * g] = *reinterpret_cast<const pd_v4f *>(rv + pd_at<2>(q));
                wv[2 * g + 1] = *reinterpret_cast<const pd_v4f *>(rv + pd_at<2>(q) + 4);
            },
            [&](int t, int rot, int c) {
                // taps 4 c .. 4 c + 3 of the row: 4 c + 3 < pitch
                const pd_v4f ta = row[2 * c + t / 2];
                const float vr = (t & 1) ? ta.z : ta.x, vi = (t & 1) ? ta.w : ta.y;
                const pd_v2f tv{vr, vi}, ts{-vi, vr};
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    // (re, im) side by side, so that each line is one packed operation: a = (rr, ri), b = (-ii, ir), the
                    // product (rr - ii, ri + ir).  fl(y (-v)) = -fl(y v) and x - y is x + (-y), both exactly
                    const pd_v2f w = pd_sample(wv, pd_slot(r, t, rot));
                    const pd_v2f a = pd_v2f{w.x, w.x} * tv, b = pd_v2f{w.y, w.y} * ts;
                    const pd_v2f pr = a + b;
                    acc[r] = acc[r] + pr;
                }
            });
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const float a = acc[r].x * acc[r].x, b = acc[r].y * acc[r].y;
            const float m = a + b;
            if (k == 0 || m > bm[r]) {                              // strict: ties keep the lowest k, a NaN m_0 stays
                bm[r] = m;
                bz[r] = acc[r];
                bk[r] = (unsigned)k;
            }
        }
        if constexpr (CORR) {
            if (live0) {
                pd_v2f *yk = reinterpret_cast<pd_v2f *>(rxy) + (size_t)k * nb + t0;
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    if (tid * kR + r < cnt) yk[tid * kR + r] = acc[r];
                }
            }
        }
    }
}

}  // namespace

// what the 48-byte event takes from its peak sample: rxy and, from the segment's spare word, the hypothesis
template <>
struct runs::PeakOf<yagi_preamble_event> {
    __host__ __device__ static void set(yagi_preamble_event &e, float re, float im, unsigned word) {
        e.rxy_re = re;
        e.rxy_im = im;
        e.hypothesis = word;
        e.pad = 0;
    }
};
namespace {

constexpr int kScanAt = 2 * kT;                                     // LDS word where the scan's two buffers start
static_assert(kScanAt + 2 * kWg * 4 <= kWordsV && 2 * kT <= kWordsE && kT <= 0x10000,
              "the scan buffers lie behind the tile's sums, inside the samples' array; energy and hypothesis fit the terms'");

__global__ void __launch_bounds__(kWg) pdet_tile_kernel(const cf32 *__restrict__ tmpl, const cf32 *__restrict__ hist,
                                                        cf32 *__restrict__ hist_next, const cf32 *__restrict__ x,
                                                        size_t nb, int L, int K, float ep, float thr2, float floor_,
                                                        BurstSeg *__restrict__ pool, unsigned long long pool_cap,
                                                        ulonglong2 *__restrict__ table,
                                                        unsigned long long *__restrict__ pool_used, double zero) {
    __shared__ __attribute__((aligned(16))) float s_lds[kWordsV + kWordsE];
    __shared__ unsigned long long s_base;
    __shared__ unsigned s_any[kWg / kWave];
    static_assert(kWg / kWave == 4, "the four flags are read by name");

    const int tid = (int)threadIdx.x;
    const size_t t0 = (size_t)blockIdx.x * kT;
    const int cnt = (int)std::min((size_t)kT, nb - t0);             // samples of this tile
    float en[kR], mm[kR];
    pd_v2f zz[kR];
    unsigned kk[kR];
    pd_tile_bank<false>(s_lds, tmpl, hist, hist_next, x, nb, L, K, t0, cnt, en, mm, zz, kk, nullptr, nullptr);

    // hit and r of the lane's outputs; an output past the block is no hit
    float qq[kR];
    unsigned hm = 0;
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        qq[r] = en[r] * ep;
        const float bar = thr2 * qq[r];
        if (tid * kR + r < cnt && en[r] > floor_ && mm[r] > bar) hm |= 1u << r;
    }
    // a hit anywhere in the tile?  One flag per wave, away from the values that other waves still read; the barrier is
    // also the one after which the staged values are read
    const unsigned wave_any = __ballot(hm != 0) != 0 ? 1u : 0u;
    if (tid % kWave == 0) s_any[tid / kWave] = wave_any;
    __syncthreads();
    if ((s_any[0] | s_any[1] | s_any[2] | s_any[3]) == 0) {         // the same for every lane
        if (tid == 0) table[blockIdx.x] = ulonglong2{0ull, 0ull};
        return;
    }

    // the sums to LDS, where a segment's peak is looked up: rxy at s_lds[0 ..), energy and hypothesis where the terms were
    float *so = s_lds, *eo = s_lds + kWordsV;
    unsigned *ho = reinterpret_cast<unsigned *>(eo + kT);
#pragma unroll
    for (int r = 0; r < kR; r += 4) {
        const int o = tid * kR + r;
        *reinterpret_cast<pd_v4f *>(so + 2 * o) = pd_v4f{zz[r].x, zz[r].y, zz[r + 1].x, zz[r + 1].y};
        *reinterpret_cast<pd_v4f *>(so + 2 * o + 4) = pd_v4f{zz[r + 2].x, zz[r + 2].y, zz[r + 3].x, zz[r + 3].y};
        *reinterpret_cast<pd_v4f *>(eo + o) = pd_v4f{en[r], en[r + 1], en[r + 2], en[r + 3]};
        *reinterpret_cast<uint4 *>(ho + o) = uint4{kk[r], kk[r + 1], kk[r + 2], kk[r + 3]};
    }

    float ratio[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) ratio[r] = ((hm >> r) & 1u) ? runs::ratio(mm[r], qq[r], zero) : 0.0f;

    runs::tile_segments<kWg, kR>(reinterpret_cast<uint4 *>(s_lds + kScanAt), s_base, hm, ratio, pool, pool_cap, table,
                                 pool_used, [&](BurstSeg &g, int peak) {
                                     g.energy = eo[peak];
                                     g.re = so[2 * peak];
                                     g.im = so[2 * peak + 1];
                                     g.pad = ho[peak];              // the hypothesis at the peak
                                 });
}

__global__ void __launch_bounds__(kWg) pdet_correlate_kernel(const cf32 *__restrict__ tmpl, const cf32 *__restrict__ hist,
                                                             cf32 *__restrict__ hist_next, const cf32 *__restrict__ x,
                                                             size_t nb, int L, int K, cf32 *__restrict__ rxy,
                                                             float *__restrict__ energy) {
    __shared__ __attribute__((aligned(16))) float s_lds[kWordsV + kWordsE];
    const size_t t0 = (size_t)blockIdx.x * kT;
    const int cnt = (int)std::min((size_t)kT, nb - t0);
    float en[kR], mm[kR];
    pd_v2f zz[kR];
    unsigned kk[kR];
    pd_tile_bank<true>(s_lds, tmpl, hist, hist_next, x, nb, L, K, t0, cnt, en, mm, zz, kk, rxy, energy);
}

// correlate_block pushes samples without looking for hits: the counter advances, a pending run cannot be continued
__global__ void pdet_advance_kernel(PdetState *state, unsigned long long nb) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        state->position += nb;
        state->has_pending = 0;
    }
}

using PdetRun = runs::Run<yagi_preamble_event>;
constexpr int kStitchWg = runs::kStitchWg;

__global__ void __launch_bounds__(kStitchWg) pdet_stitch_kernel(const ulonglong2 *__restrict__ table,
                                                                 unsigned long long tiles,
                                                                 const BurstSeg *__restrict__ pool,
                                                                 unsigned long long pool_cap, PdetState *state,
                                                                 unsigned long long nb, unsigned long long min_length,
                                                                 yagi_preamble_event *__restrict__ events,
                                                                 unsigned long long cap, unsigned *__restrict__ status) {
    runs::stitch(table, tiles, pool, pool_cap, state, nb, min_length, events, cap, status, (unsigned long long)kT);
}

int pdet_check_launch(int L, int K, size_t nb, size_t *tiles) {
    if (L < 1 || L > kPdetLmax || K < 1 || K > kPdetKmax)
        return fail(YAGI_ERR_INTERNAL, "pdet: (length, hypotheses) out of range");
    *tiles = (nb + kT - 1) / kT;
    if (*tiles > 0x7fffffffu) return fail(YAGI_ERR_CONFIG, "pdet: block too long (%zu samples)", nb);
    return YAGI_OK;
}

}  // namespace

void pdet_templates(const cf32 *p, size_t L, const float *dphi, size_t K, cf32 *out) {
    for (size_t k = 0; k < K; ++k) {
        for (size_t i = 0; i < L; ++i) {
            const double theta = (double)dphi[k] * (double)i;
            const double c = std::cos(theta), s = std::sin(theta);
            const double pr = (double)p[i].re, pi = (double)p[i].im;
            // conj(p) e^{-j theta} = (pr - j pi)(c - j s)
            const double rc = pr * c, is = pi * s, rs = pr * s, ic = pi * c;
            const double re = rc - is, im = -rs - ic;
            out[k * L + i] = cf32{(float)re, (float)im};
        }
    }
}

float pdet_preamble_energy(const cf32 *p, size_t L) {
    float ep = 0.0f;
    for (size_t i = 0; i < L; ++i) {
        const float er = p[i].re * p[i].re, ei = p[i].im * p[i].im;
        const float e = er + ei;
        ep = ep + e;
    }
    return ep;
}

void pdet_host_sums(const cf32 *h, int L, int K, const cf32 *tmpl, cf32 *rxy, float *energy) {
    float en = 0.0f;
    for (int i = 0; i < L; ++i) {
        const float er = h[i].re * h[i].re, ei = h[i].im * h[i].im;
        const float e = er + ei;
        en = en + e;
    }
    *energy = en;
    for (int k = 0; k < K; ++k) {
        const cf32 *v = tmpl + (size_t)k * (size_t)L;
        float re = 0.0f, im = 0.0f;
        for (int i = 0; i < L; ++i) {
            const float rr = h[i].re * v[i].re, ii = h[i].im * v[i].im;
            const float ri = h[i].re * v[i].im, ir = h[i].im * v[i].re;
            const float pr = rr - ii, pi = ri + ir;
            re = re + pr;
            im = im + pi;
        }
        rxy[k] = cf32{re, im};
    }
}

int pdet_host(int L, int K, const cf32 *tmpl, float ep, float thr2, float floor_, unsigned long long min_length,
              cf32 *win, PdetState *state, const cf32 *x, size_t n, yagi_preamble_event *events, size_t cap,
              size_t *count, int *overflow) {
    const size_t H = (size_t)L;
    std::vector<cf32> s(H + n);                                     // win ++ x
    std::copy(win, win + H, s.begin());
    std::copy(x, x + n, s.begin() + H);
    const size_t tiles = (n + kPdetTile - 1) / kPdetTile;
    std::vector<yagi_preamble_event> found;
    std::vector<cf32> rxy((size_t)K);
    PdetRun run;
    run.have = state->has_pending != 0;
    run.ev = state->pending;
    const unsigned long long pos0 = state->position;
    size_t segments = 0;
    bool before = false;                                            // the sample before was a hit, in the same tile
    for (size_t i = 0; i < n; ++i) {
        float e;
        pdet_host_sums(s.data() + i + 1, L, K, tmpl, rxy.data(), &e);
        float m = 0.0f;
        unsigned kb = 0;
        for (int k = 0; k < K; ++k) {
            const float a = rxy[k].re * rxy[k].re, b = rxy[k].im * rxy[k].im;
            const float mk = a + b;
            if (k == 0 || mk > m) {
                m = mk;
                kb = (unsigned)k;
            }
        }
        const float q = e * ep, bar = thr2 * q;
        const bool hit = e > floor_ && m > bar;
        if (i % kPdetTile == 0) before = false;
        if (hit) {
            if (!before) ++segments;
            yagi_preamble_event done;
            if (run.add(pos0 + i, 1, pos0 + i, m / q, e, rxy[kb].re, rxy[kb].im, kb, &done)) found.push_back(done);
        }
        before = hit;
    }
    std::copy(s.end() - H, s.end(), win);
    state->position = pos0 + n;
    *overflow = segments > tiles + (size_t)kPdetSegmax;
    *count = 0;
    if (*overflow) {
        state->has_pending = 0;
        return YAGI_OK;
    }
    const bool pending = run.have && run.ev.start + run.ev.length == pos0 + n;
    if (run.have && !pending) found.push_back(run.ev);
    state->has_pending = pending;
    if (pending) state->pending = run.ev;
    for (const auto &e : found) {
        if (e.length < min_length) continue;
        if (*count < cap) events[*count] = e;
        ++*count;
    }
    return YAGI_OK;
}

int launch_pdet(int L, int K, const cf32 *tmpl, float ep, float thr2, float floor_, unsigned long long min_length,
                const cf32 *hist, cf32 *hist_next, const cf32 *x, size_t nb, void *scratch, PdetState *state,
                yagi_preamble_event *events, size_t cap, unsigned *status, hipStream_t st) {
    size_t tiles;
    YG_TRY(pdet_check_launch(L, K, nb, &tiles));
    ulonglong2 *table = static_cast<ulonglong2 *>(scratch);
    BurstSeg *pool = reinterpret_cast<BurstSeg *>(table + tiles);
    const unsigned long long pool_cap = tiles + (unsigned long long)kPdetSegmax;
    if (nb != 0) {
        pdet_tile_kernel<<<(unsigned)tiles, kWg, 0, st>>>(tmpl, hist, hist_next, x, nb, L, K, ep, thr2, floor_, pool,
                                                          pool_cap, table, &state->pool_used, 0.0);
        YG_LAUNCH_CHECK();
    }
    pdet_stitch_kernel<<<1, kStitchWg, 0, st>>>(table, tiles, pool, pool_cap, state, nb, min_length, events, cap, status);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

int launch_pdet_correlate(int L, int K, const cf32 *tmpl, const cf32 *hist, cf32 *hist_next, const cf32 *x, size_t nb,
                          cf32 *rxy, float *energy, PdetState *state, hipStream_t st) {
    if (nb == 0) return YAGI_OK;
    size_t tiles;
    YG_TRY(pdet_check_launch(L, K, nb, &tiles));
    pdet_correlate_kernel<<<(unsigned)tiles, kWg, 0, st>>>(tmpl, hist, hist_next, x, nb, L, K, rxy, energy);
    YG_LAUNCH_CHECK();
    pdet_advance_kernel<<<1, kWave, 0, st>>>(state, nb);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

}  // namespace yagi
