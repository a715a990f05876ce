// runs_common.hpp -- from per-sample hits to events, for detectors whose front end leaves every lane with hit and r of its
// R consecutive outputs (burstdet_kernels.hip behind autocorr_tile.hpp's sums, pdet_kernels.hip behind its own bank).
// Three pieces, each over an event type Ev that has {uint64 start, length, peak; float ratio, energy} and whatever else
// PeakOf<Ev> stores at a peak:
//
// tile_segments: the back end of a tile kernel of WG lanes with R outputs each.  The tile's hits fall into segments
// (maximal runs of hits inside the tile).  Each lane reduces its own R outputs to one scan element
//     (r, peak, start) of the run that reaches its last output, open / through / first flags, segments it closes
// and a Hillis-Steele scan over the WG elements (two LDS buffers, one barrier per step) hands every lane the run that
// reaches it from the left and the number of segments closed before it.  A lane closes a segment at the first non-hit
// after it (the last lane also at the tile's end), so each lane writes at most R / 2 + 1, whatever the runs' lengths: no
// lane walks a run.  The last lane takes room for the tile's segments with one atomicAdd on the call's pool counter and
// writes {base, count} to the tile table; the segments go to pool[base ..) in order, those past the pool's end nowhere.
//
// stitch: the body of a one-workgroup kernel of kStitchWg lanes.  It reads the pool counter: zero is the common case and
// ends at once, more than the pool holds is the overflow of yagi_hip.h.  Otherwise it walks the tile table in tile
// order, kStitchWg slots per step: every lane loads one slot and, where the tile has segments, the first of them, a
// ballot per wave marks the tiles to visit, and the next step's slots are loaded while this one is walked.  The walk is
// the definition's sequential state machine (Run), run by the first wave's lanes on the same values from LDS; a closed
// run of min_length or more is an event, written by lane 0.  A tile's further segments come kStitchMore per load.  Where
// the marked tiles among 64 hold one segment each that touches neither edge of its tile, those are runs of their own and
// the wave reports them together, a lane each.  The run that ends on the call's last sample becomes the pending run.
// The body then stores position, pending run and a zeroed pool counter.  No workgroup waits on another.
//
// Run: the state machine itself, shared with the host form.
//
// Every global access is guarded: the tile table at the workgroup's own slot, the pool below pool_cap, events below cap.
#pragma once

#include <algorithm>

#include "kernels.hpp"

namespace yagi {
namespace runs {

// m / q rounded once to f32: IEEE f32 division formed in f64 (a p-bit quotient rounded from 2p + 2 bits or more rounds
// once; 53 >= 50), because the f32 expansion's Newton steps are f32 FMAs, which the files that include this hold none of.
// The compiler narrows an f64 quotient of two widened floats back to the f32 division, FMAs and all, whenever it can see
// that this changes nothing; `zero` is an exact 0.0 that it cannot see (a kernel argument), and adding it keeps the
// quotient an f64 expression.
__device__ __forceinline__ float ratio(float m, float q, double zero) {
    return (float)(((double)m + zero) / (double)q);
}

// what Ev carries from its peak sample besides r and the energy: set(ev, re, im, word), word = the segment's spare word
template <class Ev>
struct PeakOf;

// the sequential state machine of the definition, over segments instead of samples
template <class Ev>
struct Run {
    bool have = false;
    Ev ev{};
    // a piece [s, s + len) with its peak; returns true where `out` is a closed run to report
    __host__ __device__ bool add(unsigned long long s, unsigned long long len, unsigned long long pk, float r, float energy,
                                 float re, float im, unsigned word, Ev *out) {
        if (have && ev.start + ev.length == s) {
            ev.length += len;
            if (r > ev.ratio) {
                ev.peak = pk;
                ev.ratio = r;
                ev.energy = energy;
                PeakOf<Ev>::set(ev, re, im, word);
            }
            return false;
        }
        const bool closed = have;
        if (closed) *out = ev;
        have = true;
        ev.start = s;
        ev.length = len;
        ev.peak = pk;
        ev.ratio = r;
        ev.energy = energy;
        PeakOf<Ev>::set(ev, re, im, word);
        return closed;
    }
};

// A scan element: x = r of the peak of the run that reaches the range's last output, y = peak | start << 16 (offsets in
// the tile), z = flags, w = segments closed inside the range.
constexpr unsigned kOpen = 1;       // the range's last output is a hit
constexpr unsigned kThrough = 2;    // every output of the range is a hit
constexpr unsigned kFirst = 4;      // the range's first output is a hit
// a = the range on the left, b = the range that follows it
__device__ __forceinline__ uint4 join(uint4 a, uint4 b) {
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

// Lane threadIdx.x of WG holds hm (bit r: output tid R + r is a hit) and r[] of its hits.  sc = 2 WG scan elements in
// LDS, s_base one LDS word pair; at_peak(g, peak) fills energy, re, im and the spare word of a segment from wherever the
// caller keeps the tile's sums (LDS it wrote before the call: the scan's first barrier is in front of every read).
template <int WG, int R, class AtPeak>
__device__ __forceinline__ void tile_segments(uint4 *sc, unsigned long long &s_base, unsigned hm, const float (&r_)[R],
                                              BurstSeg *__restrict__ pool, unsigned long long pool_cap,
                                              ulonglong2 *__restrict__ table, unsigned long long *__restrict__ pool_used,
                                              AtPeak &&at_peak) {
    static_assert(WG * R <= 0x10000 && R <= 32, "tile offsets fit 16 bits, a lane's hits a word");
    constexpr unsigned kAll = R == 32 ? 0xffffffffu : (1u << R) - 1u;
    const int tid = (int)threadIdx.x;
    // one step of a run along the lane's outputs: a hit opens or extends it
    bool act = false;
    int start = 0, peak = 0;
    float best = 0.0f;
    auto step = [&](int r) {
        const int o = tid * R + r;
        if (!act) {
            act = true;
            start = o;
            best = r_[r];
            peak = o;
        } else if (r_[r] > best) {
            best = r_[r];
            peak = o;
        }
    };
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if ((hm >> r) & 1u) step(r);
        else act = false;
    }
    uint4 val;
    val.x = __float_as_uint(best);
    val.y = (unsigned)peak | ((unsigned)start << 16);
    val.z = (act ? kOpen : 0u) | (hm == kAll ? kThrough : 0u) | ((hm & 1u) ? kFirst : 0u);
    val.w = (unsigned)__popc(~hm & (hm << 1) & kAll) + ((tid == WG - 1 && act) ? 1u : 0u);

    // inclusive scan over the lanes; the two buffers alternate, so one barrier per step is enough
    int cur = 0;
#pragma unroll
    for (int s = 1; s < WG; s <<= 1) {
        sc[cur * WG + tid] = val;
        __syncthreads();
        if (tid >= s) val = join(sc[cur * WG + tid - s], val);
        cur ^= 1;
    }
    if (tid == WG - 1) {                                            // val.w is the tile's segment count
        const unsigned long long base = atomicAdd(pool_used, (unsigned long long)val.w);
        s_base = base;
        table[blockIdx.x] = ulonglong2{base, (unsigned long long)val.w};
    }
    sc[cur * WG + tid] = val;
    __syncthreads();

    // the run that reaches the lane from the left, and the slot of the first segment the lane closes
    unsigned long long slot = s_base;
    act = false;
    if (tid > 0) {
        const uint4 left = sc[cur * WG + tid - 1];
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
            at_peak(g, peak);
            pool[slot] = g;
        }
        ++slot;
        act = false;
    };
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if ((hm >> r) & 1u) step(r);
        else if (act) close(tid * R + r);
    }
    if (tid == WG - 1 && act) close(WG * R);                        // a hit on the tile's last output: the tile is full
}

constexpr int kStitchWg = 1024;                                    // tiles per step of the stitch walk
constexpr int kStitchMore = 256;                                   // a tile's further segments per load

// State has {position, pool_used, has_pending, pending}; tile = samples per tile
template <class Ev, class State>
__device__ __forceinline__ void stitch(const ulonglong2 *__restrict__ table, unsigned long long tiles,
                                       const BurstSeg *__restrict__ pool, unsigned long long pool_cap, State *state,
                                       unsigned long long nb, unsigned long long min_length, Ev *__restrict__ events,
                                       unsigned long long cap, unsigned *__restrict__ status, unsigned long long tile) {
    __shared__ ulonglong2 s_tab[kStitchWg];                         // {base, count} of the step's tiles
    __shared__ BurstSeg s_first[kStitchWg];                         // the first segment of each that has one
    __shared__ BurstSeg s_more[kStitchMore];
    __shared__ unsigned long long s_mask[kStitchWg / kWave];        // per wave: which of its tiles have segments
    const int tid = (int)threadIdx.x;
    const State in = *state;                                        // every lane holds the same copy
    const unsigned long long pos0 = in.position, used = in.pool_used;
    const bool overflow = used > pool_cap;
    // the state machine below runs in the lanes of the first wave, each on the same values; lane 0 does the writing.  The
    // other waves load, and keep step at the barriers: every loop bound below is the same in every lane.
    const bool walker = tid < kWave;
    Run<Ev> run;
    run.have = in.has_pending != 0 && !overflow;
    run.ev = in.pending;
    unsigned long long nev = 0;
    auto report = [&](const Ev &e) {
        if (e.length < min_length) return;
        if (tid == 0 && nev < cap) events[nev] = e;
        ++nev;
    };
    auto piece = [&](unsigned long long tile_at, const BurstSeg &g) {
        Ev done;
        if (walker &&
            run.add(tile_at + g.start, g.length, tile_at + g.peak, g.ratio, g.energy, g.re, g.im, g.pad, &done))
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
                // tiles of these 64 are like that (scattered detections, the common case), they are reported together:
                // lane l looks at tile w 64 + l, in every wave alike, so that all waves take the same way.
                const int lane = tid % kWave, jl = w * kWave + lane;
                const bool mine = (marked >> lane) & 1ull;
                const BurstSeg own = s_first[jl];                   // meaningful where mine
                const unsigned long long own_at = (k0 + (unsigned long long)jl) * tile;
                const bool alone = mine && s_tab[jl].y == 1 && own.start != 0 &&
                                   (unsigned long long)own.start + own.length < std::min(tile, nb - own_at);
                if (__ballot(mine && !alone) == 0) {
                    if (walker) {
                        if (run.have) report(run.ev);               // it ends in an earlier tile: nothing here extends it
                        run.have = false;
                        const bool keep = alone && own.length >= min_length;
                        const unsigned long long kept = __ballot(keep);
                        const unsigned long long at = nev + (unsigned long long)__popcll(kept & ((1ull << lane) - 1ull));
                        if (keep && at < cap) {
                            Ev e{};
                            e.start = pos0 + own_at + own.start;
                            e.length = own.length;
                            e.peak = pos0 + own_at + own.peak;
                            e.ratio = own.ratio;
                            e.energy = own.energy;
                            PeakOf<Ev>::set(e, own.re, own.im, own.pad);
                            events[at] = e;
                        }
                        nev += (unsigned long long)__popcll(kept);
                    }
                    continue;
                }
                for (unsigned long long mask = marked; mask; mask &= mask - 1) {
                    const int j = w * kWave + __ffsll((long long)mask) - 1;
                    const unsigned long long base = s_tab[j].x, count = s_tab[j].y;
                    const unsigned long long tile_at = pos0 + (k0 + (unsigned long long)j) * tile;
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

}  // namespace runs
}  // namespace yagi
