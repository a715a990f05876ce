// bank_lane.hpp -- the scaffold of the bank objects (SymSync, EqLms, EqRls, Agc, SymTrack): one lane, or one group of lanes,
// per channel loops over the rows of the call ("bank kernels: the lane scaffold").  Three pieces with no state
// of their own and no arithmetic on samples:
//   RowQueue  the rows of the call, requested a chunk ahead into registers and handed over chunk by chunk (the kernels of
//             SymSync, EqRls and SymTrack)
//   Ring      a window of `len` slots at a stride: those three kernels use it at their LDS stride over the lane's column,
//             the host forms (the library's definition) of SymSync, EqLms, EqRls and SymTrack at stride 1 over a std::vector
//   bank_launch  grid from the channels per workgroup, the opt-in to more than 64 KiB of dynamic LDS, launch, check (all five)
#pragma once
#include "common.hpp"

namespace yagi {
namespace {

#define BL_HD __host__ __device__ __forceinline__

// The rows [s0, s0 + N) of a call of n rows wait in registers while the chunk before them is worked through, so a step
// never waits for a memory round trip.  load(row, in_range) returns the lane's element of `row`, or T{} where the row is
// beyond the call (`in_range` false) or the lane has nothing to read; it is where a kernel states its own predicate
// (live lane, the group's lane 0).  put(u, value) takes row s0 + u of the chunk: lane_stage below is the put for an LDS
// stage.  Both loops are unrolled, so q[] is indexed statically and stays in registers.
template <class T, int N>
struct RowQueue {
    T q[N];

    template <class Load>
    __device__ __forceinline__ void prime(unsigned n, Load load) {
#pragma unroll
        for (int u = 0; u < N; ++u) q[u] = load((size_t)u, (unsigned)u < n);
    }

    // hands the held chunk [s0, s0 + N) over, requests [s0 + N, s0 + 2 N) and returns the rows of the held chunk below n
    template <class Put, class Load>
    __device__ __forceinline__ unsigned next(unsigned s0, unsigned n, Put put, Load load) {
#pragma unroll
        for (int u = 0; u < N; ++u) put(u, q[u]);
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const size_t ahead = (size_t)s0 + N + u;
            q[u] = load(ahead, ahead < n);
        }
        return n - s0 < (unsigned)N ? n - s0 : (unsigned)N;
    }
};

// put of RowQueue::next for an LDS stage [row of the chunk][lane]: `col` points at the lane's column, only a writer stores
template <class T>
__device__ __forceinline__ auto lane_stage(T *col, unsigned stride, bool writer = true) {
    return [=](int u, T v) {
        if (writer) col[u * stride] = v;
    };
}

// A window of len slots, slot e of the lane's column at col[e * stride]; head is the oldest slot, where the next sample
// goes.  A [len][C] array of the object (its history) holds the window oldest first, channel c in column c.
template <class T>
struct Ring {
    T *col;
    unsigned stride, len, head;

    BL_HD T operator()(unsigned j) const {                  // the j-th oldest sample, j < len
        const unsigned sl = head + j;
        return col[(sl >= len ? sl - len : sl) * stride];
    }

    // the oldest sample leaves; of a group of lanes that shares the window every lane advances and one writes
    BL_HD void push(T x, bool writer = true) {
        if (writer) col[head * stride] = x;
        head = head + 1 == len ? 0 : head + 1;
    }

    // slots first, first + step, ... from and to column c of hist; a lane that is not live fills zeros
    BL_HD void fill(const T *hist, size_t C, size_t c, bool live = true, unsigned first = 0, unsigned step = 1) {
        for (unsigned j = first; j < len; j += step) col[j * stride] = live ? hist[(size_t)j * C + c] : T{};
        head = 0;
    }
    // the slot is spelled out here: read through operator() the loop changes symtrack_cccf_kernel's registers and occupancy
    BL_HD void store(T *hist, size_t C, size_t c, unsigned first = 0, unsigned step = 1) const {
        for (unsigned j = first; j < len; j += step) {
            unsigned sl = head + j;
            sl = sl >= len ? sl - len : sl;
            hist[(size_t)j * C + c] = col[sl * stride];
        }
    }
};

// One workgroup of `wg` lanes per `per_wg` channels.  A kernel that asks for more than 64 KiB of dynamic LDS has to opt in.
template <class... P, class... A>
int bank_launch(void (*fn)(P...), size_t C, size_t per_wg, unsigned wg, size_t need, hipStream_t st, const A &...args) {
    if (need > 64 * 1024)
        YG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const unsigned grid = (unsigned)((C + per_wg - 1) / per_wg);
    hipLaunchKernelGGL(fn, dim3(grid), dim3(wg), need, st, args...);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

#undef BL_HD

}  // namespace
}  // namespace yagi
