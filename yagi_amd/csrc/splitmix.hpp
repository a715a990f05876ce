// splitmix.hpp -- the counter-based SplitMix64 draw shared by the synthetic-input generator (misc_kernels.hip) and
// Channel's noise (channel_words.hpp): word idx of the sequence of `seed`, u64 arithmetic, wrapping.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define YG_MIX_HD __host__ __device__ __forceinline__
#else
#define YG_MIX_HD inline
#endif

namespace yagi {

YG_MIX_HD uint64_t splitmix64_at(uint64_t seed, uint64_t idx) {
    uint64_t z = seed + (idx + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace yagi
