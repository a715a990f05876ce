// stream_tables.hpp -- layout and host builder of the twiddle table of the 4096-point stream kernels.  Plain C++ (no HIP):
// capi.hip uploads what build_stream_twiddles makes, tests/c/stream_tables_main.cpp dumps it for the CPU test.
//
//   [0, 4096)                      W_4096^m, forward
//   [4096, 4096 + 6 * 256)         six 256-entry rows read with the lane index t: rows 0-3 W^{t 2^k}, row 4
//                                  W^{(t&15)(t>>4)}, row 5 W_256^{(t&15)(t>>4)}  (overlap-save kernel, table-twiddle FFT)
//   [kStreamTabMain, + 6 * 256)    the same six entries IN PAIRS: three arrays of 256 lanes x 2 entries, rows (0,1), (2,3),
//                                  (4,5) -- lane t's 16-byte load p of the headline kernel sits at 16 t + 4096 p bytes,
//                                  so a wave's load is 1 KiB contiguous
//   [kStreamTabCorr, + 6 * 64)     wave 0's transform twiddles in pairs, three arrays of 64 lanes x 2: (w1,w2), (w4,u1),
//                                  (u2,u4) with w = W_512^{l, 2l, 4l}, u = W_64^{b', 2b', 4b'} (b' = l & 7) = entries
//                                  8l, 16l, 32l, 64b', 128b', 256b' of the W_4096 part
// The paired parts are COPIES of entries of the first two parts: a kernel that reads them multiplies by the same
// f64-derived values as one that gathers from W_4096 or reads the rows.  The scaled FFT{h} and the scaled table of the
// fast correction sum (device buffers of the filter object, freq_kernels.hip launch_scale_cf32_pairs) use the same
// pair layout, stream_pair_slot.
#pragma once
#include <cmath>

namespace yagi {

constexpr unsigned kStreamTabRows = 4096;
constexpr unsigned kStreamTabMain = 4096 + 6 * 256;
constexpr unsigned kStreamTabCorr = kStreamTabMain + 6 * 256;
constexpr unsigned kStreamTabFloat2 = kStreamTabCorr + 6 * 64;
// entry d of lane l in a table of `lanes` lanes: pair array d / 2, lane l, half d % 2
constexpr unsigned stream_pair_slot(unsigned l, unsigned d, unsigned lanes) { return 2u * lanes * (d >> 1) + 2u * l + (d & 1u); }
// scaled conj(DFT_512{g}) / 512 of the fast correction sum (lane l reads entries l + 64 d) and scaled FFT{h} (t + 256 d)
constexpr unsigned stream_gc_slot(unsigned k) { return stream_pair_slot(k & 63u, k >> 6, 64u); }
constexpr unsigned stream_hs_slot(unsigned k) { return stream_pair_slot(k & 255u, k >> 8, 256u); }
// row r of main-wave lane t / entry j (w1 w2 w4 u1 u2 u4) of wave-0 lane l, relative to kStreamTabMain / kStreamTabCorr
constexpr unsigned stream_main_slot(unsigned t, unsigned r) { return stream_pair_slot(t, r, 256u); }
constexpr unsigned stream_corr_slot(unsigned l, unsigned j) { return stream_pair_slot(l, j, 64u); }

template <class CF>      // CF = {float re, im}
inline void build_stream_twiddles(CF *tab) {
    auto W = [](unsigned m) {
        const double a = -2.0 * 3.14159265358979323846 * (double)(m & 4095u) / 4096.0;
        return CF{(float)std::cos(a), (float)std::sin(a)};
    };
    for (unsigned m = 0; m < 4096; ++m) tab[m] = W(m);
    for (unsigned t = 0; t < 256; ++t) {
        for (unsigned k = 0; k < 4; ++k) tab[kStreamTabRows + 256 * k + t] = W(t << k);
        tab[kStreamTabRows + 1024 + t] = W((t & 15u) * (t >> 4));
        tab[kStreamTabRows + 1280 + t] = W(16u * (((t & 15u) * (t >> 4)) & 255u));
    }
    for (unsigned t = 0; t < 256; ++t)
        for (unsigned r = 0; r < 6; ++r) tab[kStreamTabMain + stream_main_slot(t, r)] = tab[kStreamTabRows + 256 * r + t];
    for (unsigned l = 0; l < 64; ++l) {
        const unsigned bp = l & 7u;
        const unsigned src[6] = {8 * l, 16 * l, 32 * l, 64 * bp, 128 * bp, 256 * bp};
        for (unsigned j = 0; j < 6; ++j) tab[kStreamTabCorr + stream_corr_slot(l, j)] = tab[src[j]];
    }
}

}  // namespace yagi
