// burstdet_kernels.hip -- BurstDetector (yagi_hip.h): Autocorr(W, d), the normalised threshold
//     hit[n] = energy[n] > energy_floor && m[n] > fl(thr2 q[n]),  m = fl(fl(re^2) + fl(im^2)) of rxx[n],  q = fl(energy[n]^2)
// and the extraction of runs of hits and their peaks (the largest r = m / q, the earliest on ties) in two launches that
// read the samples and write only events.
//
// burstdet_tile_kernel<T>: a workgroup of 256 lanes owns kAutocorrTile consecutive samples.  Up to a lane's kAutocorrR
// sums it is autocorr_kernel<T, true> (ac_tile_sums below is that kernel's staging, history hand-over and register-window
// accumulation, statement for statement; autocorr_kernels.hip describes the LDS layout and the rounding points and keeps
// its own text, so that its code objects stay the ones its table was measured on).  Then each lane forms hit for its
// R outputs.  A tile without a hit writes {0, 0} to its slot of the tile table and ends: one workgroup-wide OR.
// Otherwise the tile's hits fall into segments (maximal runs of hits inside the tile).  The lanes' sums go to LDS, where
// the staged terms were, each lane reduces its own R outputs to one element
//     (r, peak, start) of the run that reaches its last output, open / through / first flags, segments it closes
// and a Hillis-Steele scan over the 256 elements (eight steps in two LDS buffers) hands every lane the run that reaches
// it from the left and the number of segments closed before it.  A lane closes a segment at the first non-hit after it
// (the last lane also at the tile's end), so each lane writes at most five, whatever the runs' lengths: no lane walks a
// run.  The last lane takes room for the tile's segments with one atomicAdd on the call's pool counter and writes
// {base, count} to the tile table; the segments go to pool[base ..) in order, those past the pool's end nowhere.
//
// burstdet_stitch_kernel: one workgroup.  It reads the pool counter: zero is the common case and ends at once, more
// than the pool holds is the overflow of yagi_hip.h.  Otherwise it walks the tile table in tile order, 1024 slots per
// step: every lane loads one slot and, where the tile has segments, the first of them (the only one of a tile that a
// burst crosses), a ballot per wave marks the tiles to visit, and the next step's slots are loaded while this one is
// walked.  The walk is the definition's sequential state machine, run by the first wave's lanes on the same values from LDS: a
// segment that starts where the run before it ends extends it (the pending run of the call before is the first run),
// anything else closes it; a closed run of min_length or more is an event, written by lane 0.  A tile's further
// segments come 256 per load.  Where the marked tiles among 64 hold one segment each that touches neither edge of its
// tile, those are runs of their own and the wave reports them together, a lane each.  The run that ends on the call's last sample becomes the pending run.  The kernel then
// stores position, pending run and a zeroed pool counter.  No workgroup waits on another: the second launch is the
// only ordering.
//
// r = m / q is IEEE f32 division.  It is formed in f64 and rounded to f32, which is the same value (a p-bit quotient
// rounded from 2p + 2 bits or more rounds once; 53 >= 50): the f32 expansion's Newton steps are f32 FMAs, and this file
// holds none (tests/test_burstdet_isa_cpu.py), so that a product or an add that lost its own rounding would show.
// bd_ratio says how the quotient is kept in f64.
//
// Every global access is guarded: x in [0, nb), the history in [0, W + d), the tile table at the workgroup's own slot,
// the pool below pool_cap, events below cap.
//
// The Makefile builds this file with -ffp-contract=off.
#pragma clang fp contract(off)

#include <algorithm>
#include <type_traits>

#include "kernels.hpp"

namespace yagi {
namespace {

typedef float ac_v2f __attribute__((ext_vector_type(2)));
typedef float ac_v4f __attribute__((ext_vector_type(4)));

constexpr int kWg = kAutocorrWg;
constexpr int kT = kAutocorrTile;
constexpr int kR = kAutocorrR;                         // outputs per lane
constexpr int kC = 4;                                  // terms per step of the window
constexpr int kStage = kT + kAutocorrWmax;             // staged positions: all a lane's last step can read
constexpr int kRows = kStage / kR;
constexpr int kPerLane = kStage / kWg;
constexpr int kHistWgs = 1024;                         // workgroups that share the copy of the history
static_assert(kR == 8 && kT == kWg * kR && kStage % kWg == 0 && kAutocorrWmax % kC == 0,
              "a lane reads its row as 16-byte words and steps by half a row");

// LDS word offset of position p in rows of kR elements of `words` words each, padded by four words
template <int words>
__device__ __forceinline__ int ac_at(int p) {
    return (p / kR) * (kR * words + 4) + (p % kR) * words;
}

// element k of a window held as 16-byte words
template <int words>
__device__ __forceinline__ auto ac_elem(const ac_v4f *w, int k) {
    if constexpr (words == 2) {
        const ac_v4f q = w[k / 2];
        return (k & 1) ? ac_v2f{q.z, q.w} : ac_v2f{q.x, q.y};
    } else {
        return w[k / 4][k % 4];
    }
}

// the shapes of autocorr_kernel<T, ENERGY> and of whatever shares its body
template <class T, bool ENERGY>
struct AcShape {
    static constexpr bool CPLX = sizeof(T) == 2 * sizeof(float);
    static constexpr int VW = (CPLX || ENERGY) ? 2 : 1;             // words of the main LDS element: P, or (P, E) of rrrf
    static constexpr bool SEP_E = CPLX && ENERGY;                   // E in an array of its own
    using X = std::conditional_t<CPLX, ac_v2f, float>;              // a sample
    using V = std::conditional_t<VW == 2, ac_v2f, float>;           // a main element
    static constexpr int kWordsV = kRows * (kR * VW + 4), kWordsE = SEP_E ? kRows * (kR + 4) : 0;
    static_assert((size_t)(kWordsV + kWordsE) * sizeof(float) == autocorr_lds_bytes(sizeof(T), ENERGY), "kernels.hpp");
};

// Lane tid's kR sums of the tile that starts at output t0 and holds cnt outputs: acc[r] is rxx (for rrrf with ENERGY,
// (rxx, energy)) and, for cccf with ENERGY, en[r] the energy of output t0 + tid kR + r.  s_lds holds kWordsV + kWordsE
// words.  The caller synchronises the workgroup before it reuses s_lds: the terms are being read until then.
template <class T, bool ENERGY>
__device__ __forceinline__ void ac_tile_sums(float *s_lds, const T *__restrict__ hist, T *__restrict__ hist_next,
                                             const T *__restrict__ x, size_t nb, int W, int d, size_t t0, int cnt,
                                             typename AcShape<T, ENERGY>::V (&acc)[kR],
                                             float (&en)[AcShape<T, ENERGY>::SEP_E ? kR : 1]) {
    using S = AcShape<T, ENERGY>;
    constexpr bool CPLX = S::CPLX, SEP_E = S::SEP_E;
    constexpr int VW = S::VW;
    using X = typename S::X;
    using V = typename S::V;
    float *const s_v = s_lds, *const s_e = s_lds + S::kWordsV;

    const int tid = (int)threadIdx.x;
    const int span = cnt + W - 1;                                   // position p is sample t0 + p - (W - 1)
    const long long H = (long long)W + (long long)d;                // hist = the H samples before x[0], oldest first
    const X *xe = reinterpret_cast<const X *>(x), *he = reinterpret_cast<const X *>(hist);

    {
        const long long first = (long long)t0 - (long long)(W - 1);
        X ua[kPerLane], ub[kPerLane];                               // a lane's loads are issued before the first is used
#pragma unroll
        for (int c = 0; c < kPerLane; ++c) {
            // every lane loads, past the span its last sample again, from an address picked without a branch
            const int p = std::min(tid + c * kWg, span - 1);
            const long long ga = first + p, gb = ga - (long long)d; // gb >= -(W - 1) - d > -H
            ua[c] = *(ga >= 0 ? xe + ga : he + (H + ga));
            ub[c] = *(gb >= 0 ? xe + gb : he + (H + gb));
        }
#pragma unroll
        for (int c = 0; c < kPerLane; ++c) {
            const int p = tid + c * kWg;
            if constexpr (CPLX) {
                const ac_v2f a = ua[c], b = ub[c];
                const float rr = a.x * b.x, ii = a.y * b.y, ir = a.y * b.x, ri = a.x * b.y;
                *reinterpret_cast<ac_v2f *>(s_v + ac_at<2>(p)) = ac_v2f{rr + ii, ir - ri};
                if constexpr (ENERGY) {
                    const float er = a.x * a.x, ei = a.y * a.y;
                    s_e[ac_at<1>(p)] = er + ei;
                }
            } else if constexpr (ENERGY) {
                *reinterpret_cast<ac_v2f *>(s_v + ac_at<2>(p)) = ac_v2f{ua[c] * ub[c], ua[c] * ua[c]};
            } else {
                s_v[ac_at<1>(p)] = ua[c] * ub[c];
            }
        }
    }
    // the history the call leaves: the last H samples of hist ++ x, shared among the first kHistWgs workgroups (the loop
    // is kept rolled: a runtime trip count would cost a division)
    if (blockIdx.x < (unsigned)kHistWgs) {
        X *hn = reinterpret_cast<X *>(hist_next);
        const int Hi = W + d, step = (int)std::min(gridDim.x, (unsigned)kHistWgs) * kWg;
#pragma unroll 1
        for (int j = (int)blockIdx.x * kWg + tid; j < Hi; j += step) {
            const long long g = (long long)nb - H + j;
            hn[j] = g >= 0 ? xe[g] : he[(long long)j + (long long)nb];
        }
    }
    __syncthreads();

    // the register windows, kept as the 16-byte words they are read as: element k of wv is ac_elem<VW>(wv, k)
    constexpr int kWv = (kR + kC) * VW / 4, kStepV = kC * VW / 4;   // words of a window, and of one step of it
    const float *rv = s_v + tid * (kR * VW + 4), *re_ = s_e + tid * (kR + 4);
    ac_v4f wv[kWv], we[SEP_E ? (kR + kC) / 4 : 1];
    // positions q .. q + 3 of the lane (q a multiple of 4) into step w of the windows: row q / R from its own, either half
    auto fetch = [&](int q, int w) {
#pragma unroll
        for (int v = 0; v < kStepV; ++v) wv[w * kStepV + v] = *reinterpret_cast<const ac_v4f *>(rv + ac_at<VW>(q) + 4 * v);
        if constexpr (SEP_E) we[w] = *reinterpret_cast<const ac_v4f *>(re_ + ac_at<1>(q));
    };
    // term t of all R outputs; rot = which of the window's three steps is its first
    auto terms = [&](int t, int rot) {
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const int k = ((r + t) / kC + rot) % 3 * kC + (r + t) % kC;
            acc[r] = acc[r] + ac_elem<VW>(wv, k);
            if constexpr (SEP_E) en[r] = en[r] + ac_elem<1>(we, k);
        }
    };
    // four terms of all R outputs: the next step of the window is read into the slot behind the two in use
    auto chunk = [&](int c, int rot) {
        fetch(kR + kC * c, (rot + 2) % 3);
#pragma unroll
        for (int t = 0; t < kC; ++t) terms(t, rot);
    };
    fetch(0, 0);
    fetch(kC, 1);
#pragma unroll
    for (int r = 0; r < kR; ++r) acc[r] = V(0.0f);
    if constexpr (SEP_E) {
#pragma unroll
        for (int r = 0; r < kR; ++r) en[r] = 0.0f;
    }

    const int full = W / kC, rem = W - full * kC;                   // the same for every lane
    int c = 0;
#pragma unroll 1
    for (; c + 3 <= full; c += 3) {                                 // three steps on, the window's slots are where they
        chunk(c, 0);                                                // were: no register is moved
        chunk(c + 1, 1);
        chunk(c + 2, 2);
    }
#pragma unroll 1
    for (; c < full; ++c) {
        chunk(c, 0);
#pragma unroll
        for (int v = 0; v < kWv - kStepV; ++v) wv[v] = wv[v + kStepV];
        if constexpr (SEP_E) {
            we[0] = we[1];
            we[1] = we[2];
        }
    }
    if (rem) {
        fetch(kR + kC * full, 2);
#pragma unroll
        for (int t = 0; t < kC - 1; ++t) {
            if (t < rem) terms(t, 0);
        }
    }
}

// m / q rounded once to f32 (see the head of the file).  The compiler narrows an f64 quotient of two widened floats back to
// the f32 division, FMAs and all, whenever it can see that this changes nothing; `zero` is an exact 0.0 that it cannot
// see (a kernel argument), and adding it keeps the quotient an f64 expression.
__device__ __forceinline__ float bd_ratio(float m, float q, double zero) {
    return (float)(((double)m + zero) / (double)q);
}

// A scan element: x = r of the peak of the run that reaches the range's last output, y = peak | start << 16 (offsets in
// the tile), z = flags, w = segments closed inside the range.
constexpr unsigned kOpen = 1;       // the range's last output is a hit
constexpr unsigned kThrough = 2;    // every output of the range is a hit
constexpr unsigned kFirst = 4;      // the range's first output is a hit
// a = the range on the left, b = the range that follows it
__device__ __forceinline__ uint4 bd_join(uint4 a, uint4 b) {
    uint4 c;
    c.w = a.w + b.w + (((a.z & kOpen) && !(b.z & kFirst)) ? 1u : 0u);     // a's open run ends on the seam
    if ((b.z & kThrough) && (a.z & kOpen)) {                              // a's run goes on through all of b
        const bool later = __uint_as_float(b.x) > __uint_as_float(a.x);    // ties stay with the earlier peak
        c.x = later ? b.x : a.x;
        c.y = ((later ? b.y : a.y) & 0xffffu) | (a.y & 0xffff0000u);
        c.z = kOpen | (a.z & kThrough) | (a.z & kFirst);
    } else {
        c.x = b.x;
        c.y = b.y;
        c.z = (b.z & kOpen) | (a.z & kFirst);
    }
    return c;
}

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
    for (int r = 0; r < kR; ++r) ratio[r] = ((hm >> r) & 1u) ? bd_ratio(mm[r], qq[r], zero) : 0.0f;

    // one step of a run along the lane's outputs: a hit opens or extends it
    bool act = false;
    int start = 0, peak = 0;
    float best = 0.0f;
    auto step = [&](int r) {
        const int o = tid * kR + r;
        if (!act) {
            act = true;
            start = o;
            best = ratio[r];
            peak = o;
        } else if (ratio[r] > best) {
            best = ratio[r];
            peak = o;
        }
    };
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        if ((hm >> r) & 1u) step(r);
        else act = false;
    }
    uint4 val;
    val.x = __float_as_uint(best);
    val.y = (unsigned)peak | ((unsigned)start << 16);
    val.z = (act ? kOpen : 0u) | (hm == 0xffu ? kThrough : 0u) | ((hm & 1u) ? kFirst : 0u);
    val.w = (unsigned)__popc(~hm & (hm << 1) & 0xffu) + ((tid == kWg - 1 && act) ? 1u : 0u);

    // inclusive scan over the lanes; the two buffers alternate, so one barrier per step is enough
    uint4 *sc = reinterpret_cast<uint4 *>(s_lds + kScanAt);
    int cur = 0;
#pragma unroll
    for (int s = 1; s < kWg; s <<= 1) {
        sc[cur * kWg + tid] = val;
        __syncthreads();
        if (tid >= s) val = bd_join(sc[cur * kWg + tid - s], val);
        cur ^= 1;
    }
    if (tid == kWg - 1) {                                           // val.w is the tile's segment count
        const unsigned long long base = atomicAdd(pool_used, (unsigned long long)val.w);
        s_base = base;
        table[blockIdx.x] = ulonglong2{base, (unsigned long long)val.w};
    }
    sc[cur * kWg + tid] = val;
    __syncthreads();

    // the run that reaches the lane from the left, and the slot of the first segment the lane closes
    unsigned long long slot = s_base;
    act = false;
    if (tid > 0) {
        const uint4 left = sc[cur * kWg + tid - 1];
        slot += left.w;
        if (left.z & kOpen) {
            act = true;
            best = __uint_as_float(left.x);
            peak = (int)(left.y & 0xffffu);
            start = (int)(left.y >> 16);
        }
    }
    auto close = [&](int end) {
        if (slot < pool_cap) {
            BurstSeg g;
            g.start = (unsigned)start;
            g.length = (unsigned)(end - start);
            g.peak = (unsigned)peak;
            g.ratio = best;
            g.energy = eo[peak];
            g.re = CPLX ? so[2 * peak] : so[peak];
            g.im = CPLX ? so[2 * peak + 1] : 0.0f;
            g.pad = 0;
            pool[slot] = g;
        }
        ++slot;
        act = false;
    };
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        if ((hm >> r) & 1u) step(r);
        else if (act) close(tid * kR + r);
    }
    if (tid == kWg - 1 && act) close(kT);                           // a hit on output kT - 1: the tile is full
}

// the sequential state machine of the definition, over segments instead of samples
struct BurstRun {
    bool have = false;
    yagi_burst_event ev{};
    // a piece [s, s + len) with its peak; returns true where `out` is a closed run to report
    __host__ __device__ bool add(unsigned long long s, unsigned long long len, unsigned long long pk, float ratio,
                                 float energy, float re, float im, yagi_burst_event *out) {
        if (have && ev.start + ev.length == s) {
            ev.length += len;
            if (ratio > ev.ratio) {
                ev.peak = pk;
                ev.ratio = ratio;
                ev.energy = energy;
                ev.rxx_re = re;
                ev.rxx_im = im;
            }
            return false;
        }
        const bool closed = have;
        if (closed) *out = ev;
        have = true;
        ev.start = s;
        ev.length = len;
        ev.peak = pk;
        ev.ratio = ratio;
        ev.energy = energy;
        ev.rxx_re = re;
        ev.rxx_im = im;
        return closed;
    }
};

constexpr int kStitchWg = 1024;                                    // tiles per step of the stitch kernel's walk
constexpr int kStitchMore = 256;                                   // a tile's further segments per load

__global__ void __launch_bounds__(kStitchWg) burstdet_stitch_kernel(const ulonglong2 *__restrict__ table,
                                                                     unsigned long long tiles,
                                                                     const BurstSeg *__restrict__ pool,
                                                                     unsigned long long pool_cap, BurstState *state,
                                                                     unsigned long long nb, unsigned long long min_length,
                                                                     yagi_burst_event *__restrict__ events,
                                                                     unsigned long long cap, unsigned *__restrict__ status) {
    __shared__ ulonglong2 s_tab[kStitchWg];                         // {base, count} of the step's tiles
    __shared__ BurstSeg s_first[kStitchWg];                         // the first segment of each that has one
    __shared__ BurstSeg s_more[kStitchMore];
    __shared__ unsigned long long s_mask[kStitchWg / kWave];        // per wave: which of its tiles have segments
    const int tid = (int)threadIdx.x;
    const BurstState in = *state;                                   // every lane holds the same copy
    const unsigned long long pos0 = in.position, used = in.pool_used;
    const bool overflow = used > pool_cap;
    // the state machine below runs in the lanes of the first wave, each on the same values; lane 0 does the writing.  The
    // other waves load, and keep step at the barriers: every loop bound below is the same in every lane.
    const bool walker = tid < kWave;
    BurstRun run;
    run.have = in.has_pending != 0 && !overflow;
    run.ev = in.pending;
    unsigned long long nev = 0;
    auto report = [&](const yagi_burst_event &e) {
        if (e.length < min_length) return;
        if (tid == 0 && nev < cap) events[nev] = e;
        ++nev;
    };
    auto piece = [&](unsigned long long tile_at, const BurstSeg &g) {
        yagi_burst_event done;
        if (walker && run.add(tile_at + g.start, g.length, tile_at + g.peak, g.ratio, g.energy, g.re, g.im, &done))
            report(done);
    };
    auto slot_of = [&](unsigned long long k) { return k < tiles ? table[k] : ulonglong2{0ull, 0ull}; };

    if (!overflow && used != 0) {
        ulonglong2 slot = slot_of((unsigned long long)tid);
        for (unsigned long long k0 = 0; k0 < tiles; k0 += kStitchWg) {
            s_tab[tid] = slot;
            if (slot.y != 0) s_first[tid] = pool[slot.x];           // base + count <= used <= pool_cap
            const unsigned long long any = __ballot(slot.y != 0);
            if (tid % kWave == 0) s_mask[tid / kWave] = any;
            slot = slot_of(k0 + (unsigned long long)(kStitchWg + tid));   // the next step's, while this one is walked
            __syncthreads();
            for (int w = 0; w < kStitchWg / kWave; ++w) {
                const unsigned long long marked = s_mask[w];
                if (marked == 0) continue;
                // A tile's only segment that touches neither edge of the tile is a run of its own.  Where all the marked
                // tiles of these 64 are like that (scattered short runs), they are reported together: lane l looks at
                // tile w 64 + l, in every wave alike, so that all waves take the same way.
                const int lane = tid % kWave, jl = w * kWave + lane;
                const bool mine = (marked >> lane) & 1ull;
                const BurstSeg own = s_first[jl];                   // meaningful where mine
                const unsigned long long own_at = (k0 + (unsigned long long)jl) * (unsigned long long)kT;
                const bool alone = mine && s_tab[jl].y == 1 && own.start != 0 &&
                                   (unsigned long long)own.start + own.length < std::min((unsigned long long)kT, nb - own_at);
                if (__ballot(mine && !alone) == 0) {
                    if (walker) {
                        if (run.have) report(run.ev);               // it ends in an earlier tile: nothing here extends it
                        run.have = false;
                        const bool keep = alone && own.length >= min_length;
                        const unsigned long long kept = __ballot(keep);
                        const unsigned long long at = nev + (unsigned long long)__popcll(kept & ((1ull << lane) - 1ull));
                        if (keep && at < cap) {
                            yagi_burst_event e;
                            e.start = pos0 + own_at + own.start;
                            e.length = own.length;
                            e.peak = pos0 + own_at + own.peak;
                            e.ratio = own.ratio;
                            e.energy = own.energy;
                            e.rxx_re = own.re;
                            e.rxx_im = own.im;
                            events[at] = e;
                        }
                        nev += (unsigned long long)__popcll(kept);
                    }
                    continue;
                }
                for (unsigned long long mask = marked; mask; mask &= mask - 1) {
                    const int j = w * kWave + __ffsll((long long)mask) - 1;
                    const unsigned long long base = s_tab[j].x, count = s_tab[j].y;
                    const unsigned long long tile_at = pos0 + (k0 + (unsigned long long)j) * (unsigned long long)kT;
                    piece(tile_at, s_first[j]);
                    for (unsigned long long s0 = 1; s0 < count; s0 += kStitchMore) {   // the same trip count in every lane
                        const int m = (int)std::min((unsigned long long)kStitchMore, count - s0);
                        __syncthreads();                            // the segments of the load before are read
                        if (tid < m) s_more[tid] = pool[base + s0 + (unsigned long long)tid];
                        __syncthreads();
                        if (walker) {
                            for (int i = 0; i < m; ++i) piece(tile_at, s_more[i]);
                        }
                    }
                }
            }
            __syncthreads();                                        // the step's tables are read
        }
    }
    const bool pending = run.have && run.ev.start + run.ev.length == pos0 + nb;
    if (run.have && !pending) report(run.ev);
    if (tid == 0) {
        status[0] = (unsigned)std::min(nev, 0xffffffffull);
        status[1] = overflow ? 1u : 0u;
        state->position = pos0 + nb;
        state->pool_used = 0;
        state->has_pending = pending ? 1u : 0u;
        if (pending) state->pending = run.ev;
    }
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
    BurstRun run;
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
            if (run.add(pos0 + i, 1, pos0 + i, m / q, e, v[0], CPLX ? v[1] : 0.0f, &done)) found.push_back(done);
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
