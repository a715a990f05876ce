// osc_mix.hpp -- the per-sample arithmetic of Osc's block mixing, shared by osc_kernels.hip and ddc_kernels.hip.
// Both files are built with -ffp-contract=off (Makefile): the VCO lookup value + acc * skew and the complex product
// keep the reference's two roundings each.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace yagi {

template <int VCO> struct OscEntry { using E = float2; };    // NCO {sin, cos}
template <> struct OscEntry<1> { using E = float4; };          // VCO {v_sin, s_sin, v_cos, s_cos}

template <int VCO, bool DOWN>
__host__ __device__ __forceinline__ float2 osc_one(const typename OscEntry<VCO>::E *tab, uint32_t theta, float xr, float xi) {
    float s, c;
    if constexpr (!VCO) {
        const float2 e = tab[(theta + (1u << 21)) >> 22];
        s = e.x;
        c = e.y;
    } else {
        const float4 e = tab[theta >> 22];
        const float acc = (float)(theta & 0x3FFFFFu);
        s = e.x + acc * e.y;
        c = e.z + acc * e.w;
    }
    if (DOWN) s = -s;
    return make_float2(xr * c - xi * s, xr * s + xi * c);
}

}  // namespace yagi
