// burstdet_kernels.hip -- BurstDetector (yagi_hip.h): Autocorr(W, d), the normalised threshold
//     hit[n] = energy[n] > energy_floor && m[n] > fl(thr2 q[n]),  m = fl(fl(re^2) + fl(im^2)) of rxx[n],  q = fl(energy[n]^2)
// and the extraction of runs of hits and their peaks (the largest r = m / q, the earliest on ties) in two launches that
// read the samples and write only events.
//
// burstdet_tile_kernel<T>: a workgroup of 256 lanes owns kAutocorrTile consecutive samples.  Up to a lane's kAutocorrR
// sums it is autocorr_kernel<T, true>: both call ac_tile_sums (autocorr_tile.hpp, which describes the staging, the LDS
// layout and the rounding points).  Then each lane forms hit for its R outputs.  A tile without a hit writes {0, 0} to
// its slot of the tile table and ends: one workgroup-wide OR.  Otherwise the lanes' sums go to LDS, where the staged
// terms were, and runs::tile_segments (runs_common.hpp) scans the lanes' runs and writes the tile's segments (maximal
// runs of hits inside the tile) to the call's pool.
//
// burstdet_stitch_kernel: runs::stitch (runs_common.hpp) over the 40-byte event: one workgroup walks the tile table in
// tile order, joins segments that meet at a tile seam (the pending run of the call before is the first run), reports
// closed runs of min_length or more, and stores position, pending run and a zeroed pool counter.  No workgroup waits on
// another: the second launch is the only ordering.
//
// r = m / q is IEEE f32 division.  It is formed in f64 and rounded to f32, which is the same value (a p-bit quotient
// rounded from 2p + 2 bits or more rounds once; 53 >= 50): the f32 expansion's Newton steps are f32 FMAs, and this file
// holds none (tests/test_burstdet_isa_cpu.py), so that a product or an add that lost its own rounding would show.
// runs::ratio says how the quotient is kept in f64.
//
// Every global access is guarded: x in [0, nb), the history in [0, W + d), the tile table at the workgroup's own slot,
// the pool below pool_cap, events below cap.
//
// The Makefile builds this file with -ffp-contract=off.
#pragma clang fp contract(off)

#include "autocorr_tile.hpp"
#include "runs_common.hpp"

namespace yagi {

// what the 40-byte event takes from its peak sample: rxx; the segment's spare word is not used
template <>
struct runs::PeakOf<yagi_burst_event> {
    __host__ __device__ static void set(yagi_burst_event &e, float re, float im, unsigned) {
        e.rxx_re = re;
        e.rxx_im = im;
    }
};
namespace {

constexpr int kScanAt = 2 * kT;                                     // LDS word where the scan's two buffers start
static_assert(kScanAt + 2 * kWg * 4 <= AcShape<float, true>::kWordsV && kT <= 0x10000,
              "the scan buffers lie behind the tile's sums, inside the main array");

template <class T>
__global__ void __launch_bounds__(kWg) burstdet_tile_kernel(const T *__restrict__ hist, T *__restrict__ hist_next,
                                                            const T *__restrict__ x, size_t nb, int W, int d, float thr2,
                                                            float floor_, BurstSeg *__restrict__ pool,
                                                            unsigned long long pool_cap, ulonglong2 *__restrict__ table,
                                                            unsigned long long *__restrict__ pool_used, double zero) {
    using S = AcShape<T, true>;
    constexpr bool CPLX = S::CPLX;
    __shared__ __attribute__((aligned(16))) float s_lds[S::kWordsV + S::kWordsE];
    __shared__ unsigned long long s_base;
    __shared__ unsigned s_any[kWg / kWave];
    static_assert(kWg / kWave == 4, "the four flags are read by name");

    const int tid = (int)threadIdx.x;
    const size_t t0 = (size_t)blockIdx.x * kT;
    const int cnt = (int)std::min((size_t)kT, nb - t0);             // samples of this tile
    typename S::V acc[kR];
    float en[CPLX ? kR : 1];
    ac_tile_sums<T, true>(s_lds, hist, hist_next, x, nb, W, d, t0, cnt, acc, en);

    // hit and r of the lane's outputs; an output past the block is no hit
    float mm[kR], qq[kR];
    unsigned hm = 0;
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        float e;
        if constexpr (CPLX) {
            const float a = acc[r].x * acc[r].x, b = acc[r].y * acc[r].y;
            mm[r] = a + b;
            e = en[r];
        } else {
            mm[r] = acc[r].x * acc[r].x;
            e = acc[r].y;
        }
        qq[r] = e * e;
        const float bar = thr2 * qq[r];
        if (tid * kR + r < cnt && e > floor_ && mm[r] > bar) hm |= 1u << r;
    }
    // a hit anywhere in the tile?  One flag per wave, away from the terms that other waves still read; the barrier is
    // also the one after which the terms are read
    const unsigned wave_any = __ballot(hm != 0) != 0 ? 1u : 0u;
    if (tid % kWave == 0) s_any[tid / kWave] = wave_any;
    __syncthreads();
    if ((s_any[0] | s_any[1] | s_any[2] | s_any[3]) == 0) {         // the same for every lane
        if (tid == 0) table[blockIdx.x] = ulonglong2{0ull, 0ull};
        return;
    }

    // the sums to LDS, where a segment's peak is looked up: rxx at s_v[0 ..), energy at s_e[0 ..) or, for rrrf, at s_v[kT ..)
    float *so = s_lds, *eo = CPLX ? s_lds + S::kWordsV : s_lds + kT;
#pragma unroll
    for (int r = 0; r < kR; r += 4) {
        const int o = tid * kR + r;
        if constexpr (CPLX) {
            *reinterpret_cast<ac_v4f *>(so + 2 * o) = ac_v4f{acc[r].x, acc[r].y, acc[r + 1].x, acc[r + 1].y};
            *reinterpret_cast<ac_v4f *>(so + 2 * o + 4) = ac_v4f{acc[r + 2].x, acc[r + 2].y, acc[r + 3].x, acc[r + 3].y};
            *reinterpret_cast<ac_v4f *>(eo + o) = ac_v4f{en[r], en[r + 1], en[r + 2], en[r + 3]};
        } else {
            *reinterpret_cast<ac_v4f *>(so + o) = ac_v4f{acc[r].x, acc[r + 1].x, acc[r + 2].x, acc[r + 3].x};
            *reinterpret_cast<ac_v4f *>(eo + o) = ac_v4f{acc[r].y, acc[r + 1].y, acc[r + 2].y, acc[r + 3].y};
        }
    }

    float ratio[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) ratio[r] = ((hm >> r) & 1u) ? runs::ratio(mm[r], qq[r], zero) : 0.0f;

    runs::tile_segments<kWg, kR>(reinterpret_cast<uint4 *>(s_lds + kScanAt), s_base, hm, ratio, pool, pool_cap, table,
                                 pool_used, [&](BurstSeg &g, int peak) {
                                     g.energy = eo[peak];
                                     g.re = CPLX ? so[2 * peak] : so[peak];
                                     g.im = CPLX ? so[2 * peak + 1] : 0.0f;
                                     g.pad = 0;
                                 });
}

constexpr int kStitchWg = runs::kStitchWg;

__global__ void __launch_bounds__(kStitchWg) burstdet_stitch_kernel(const ulonglong2 *__restrict__ table,
                                                                     unsigned long long tiles,
                                                                     const BurstSeg *__restrict__ pool,
                                                                     unsigned long long pool_cap, BurstState *state,
                                                                     unsigned long long nb, unsigned long long min_length,
                                                                     yagi_burst_event *__restrict__ events,
                                                                     unsigned long long cap, unsigned *__restrict__ status) {
    runs::stitch(table, tiles, pool, pool_cap, state, nb, min_length, events, cap, status, (unsigned long long)kT);
}

}  // namespace

template <class T>
int burstdet_host(int W, int d, float thr2, float floor_, unsigned long long min_length, T *win, BurstState *state,
                  const T *x, size_t n, yagi_burst_event *events, size_t cap, size_t *count, int *overflow) {
    constexpr bool CPLX = sizeof(T) == 2 * sizeof(float);
    const size_t H = (size_t)W + (size_t)d;
    std::vector<T> s(H + n);                                        // win ++ x
    std::copy(win, win + H, s.begin());
    std::copy(x, x + n, s.begin() + H);
    const size_t tiles = (n + kAutocorrTile - 1) / kAutocorrTile;
    std::vector<yagi_burst_event> found;
    runs::Run<yagi_burst_event> run;
    run.have = state->has_pending != 0;
    run.ev = state->pending;
    const unsigned long long pos0 = state->position;
    size_t segments = 0;
    bool before = false;                                            // the sample before was a hit, in the same tile
    for (size_t i = 0; i < n; ++i) {
        T rxx;
        float e;
        autocorr_host<T>(s.data() + i + 1, W, d, &rxx, &e);
        const float *v = reinterpret_cast<const float *>(&rxx);
        float m;
        if constexpr (CPLX) {
            const float a = v[0] * v[0], b = v[1] * v[1];
            m = a + b;
        } else {
            m = v[0] * v[0];
        }
        const float q = e * e, bar = thr2 * q;
        const bool hit = e > floor_ && m > bar;
        if (i % kAutocorrTile == 0) before = false;
        if (hit) {
            if (!before) ++segments;
            yagi_burst_event done;
            if (run.add(pos0 + i, 1, pos0 + i, m / q, e, v[0], CPLX ? v[1] : 0.0f, 0, &done)) found.push_back(done);
        }
        before = hit;
    }
    std::copy(s.end() - H, s.end(), win);
    state->position = pos0 + n;
    *overflow = segments > tiles + (size_t)kBurstSegmax;
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
template int burstdet_host<float>(int, int, float, float, unsigned long long, float *, BurstState *, const float *, size_t,
                                  yagi_burst_event *, size_t, size_t *, int *);
template int burstdet_host<cf32>(int, int, float, float, unsigned long long, cf32 *, BurstState *, const cf32 *, size_t,
                                 yagi_burst_event *, size_t, size_t *, int *);

template <class T>
int launch_burstdet(int W, int d, float thr2, float floor_, unsigned long long min_length, const T *hist, T *hist_next,
                    const T *x, size_t nb, void *scratch, BurstState *state, yagi_burst_event *events, size_t cap,
                    unsigned *status, hipStream_t st) {
    if (W < 1 || W > kAutocorrWmax || d < 0 || d > kAutocorrDmax)
        return fail(YAGI_ERR_INTERNAL, "burstdet: (window_size, delay) out of range");
    const size_t tiles = (nb + kT - 1) / kT;
    if (tiles > 0x7fffffffu) return fail(YAGI_ERR_CONFIG, "burstdet: block too long (%zu samples)", nb);
    ulonglong2 *table = static_cast<ulonglong2 *>(scratch);
    BurstSeg *pool = reinterpret_cast<BurstSeg *>(table + tiles);
    const unsigned long long pool_cap = tiles + (unsigned long long)kBurstSegmax;
    if (nb != 0) {
        burstdet_tile_kernel<T><<<(unsigned)tiles, kWg, 0, st>>>(hist, hist_next, x, nb, W, d, thr2, floor_, pool, pool_cap,
                                                                 table, &state->pool_used, 0.0);
        YG_LAUNCH_CHECK();
    }
    burstdet_stitch_kernel<<<1, kStitchWg, 0, st>>>(table, tiles, pool, pool_cap, state, nb, min_length, events, cap, status);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}
template int launch_burstdet<float>(int, int, float, float, unsigned long long, const float *, float *, const float *,
                                    size_t, void *, BurstState *, yagi_burst_event *, size_t, unsigned *, hipStream_t);
template int launch_burstdet<cf32>(int, int, float, float, unsigned long long, const cf32 *, cf32 *, const cf32 *, size_t,
                                   void *, BurstState *, yagi_burst_event *, size_t, unsigned *, hipStream_t);

}  // namespace yagi
