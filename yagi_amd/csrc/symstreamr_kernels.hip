// symstreamr_kernels.hip -- SymStreamR (src/framing/symstreamr.rs): a SymStream at two samples per symbol and the
// arbitrary-rate Resamp of its MsResamp in one launch that reads no sample.
//
// A call pushes `need` samples s[0 .. need) of the SymStream through the Resamp and takes all ny = num_output(need)
// outputs.  With A_j = p0 + j * step, output j comes after sample i_j = A_j >> 24 and uses branch
// (A_j & 0xFFFFFF) >> (24 - bits) over s[i_j - 13 .. i_j] (resamp_kernel).  A workgroup owns wg_tiles tiles of `tile`
// consecutive outputs (the tile of resamp_plan); from A it knows
//   its samples         t in [i_first - (Lr - 1), i_last]; t < 0: values of the Resamp's carried window
//   their symbol slots  sample t is branch (t + p) & 1 of slot (t + p) >> 1, p = the SymStream's buf_index; where p = 1,
//                       slot 0 is the symbol the previous call pushed (`old`)
//   the slots' symbols  slot q reads X[q - old - j], j = 0 .. Ls-1, X = carried symbol window ++ new symbols
// so it stages, as symstream_kernel does, the carried symbol values and tab[sym] of the new ones (tab = map * gain once
// per workgroup; the first wave jumps the LFSR to the first new symbol, a lane adds tid * run symbols with the object's
// lane-stride matrices), forms the samples into a second LDS region with the bank kernels' chain (pfb_branch_dot: a
// lane owns a slot and forms both branches, taps through the scalar cache), and after one barrier runs resamp_kernel's
// chain (resamp_branch_dot) from LDS.  Both chains are the bodies of fir_bodies.hpp the two kernels themselves run, so
// every word equals SymStream.write_samples -> Resamp.execute_block.  Carried values are copied, never recomputed: the
// gain or the scheme may have changed since.
// Output j goes to ya[j] for j < split and to yb[j - split] behind it (the part of the call the caller asked for and
// the leftover; with half-band stages to follow, ya is the stream between the two parts and split = ny).
// The last workgroup (its span ends with sample need - 1) writes what the call leaves: the Resamp's window (the last Lr
// samples), the symbol window (the last Ls entries of X, where the call pushed a symbol) and buf[1] where the call
// ends between the two samples of a symbol.
//
// LDS, all dynamic: [symbols | samples | tab | the jumped state], every part on a 16-byte boundary.  No scratch.  Every
// global access is guarded: swin in [0, Ls), rwin in [0, Lr), map in [0, M), ya in [0, split), yb in [0, ny - split),
// swin_next in [0, Ls), rwin_next in [0, Lr), buf[1].
#include <algorithm>
#include <cstdint>

#include "fir_bodies.hpp"
#include "kernels.hpp"

namespace yagi {
namespace {

constexpr size_t kSymRLdsLimit = 64 * 1024;
// symbols + samples of a workgroup's tiles.  Measured: one jump per more tiles pays only while four or
// five workgroups still fit a CU's LDS; at 45 - 52 KiB the call was 1.2 times slower than at 23 - 34 KiB
constexpr size_t kSymRSpanBudget = 32 * 1024;
constexpr size_t kSymRTargetWgs = 1024;            // a long call keeps about this many workgroups
inline size_t round16(size_t b) { return (b + 15) / 16 * 16; }

struct SymRArgs {
    const cf32 *swin;           // Ls symbol values, oldest first
    const float *shb;           // [2][Ls]
    const cf32 *map;            // M points
    const unsigned *pow, *stride;
    cf32 *swin_next, *buf;
    const cf32 *rwin;           // Lr samples, oldest first
    const float *rhb;           // [2^bits][Lr]
    cf32 *rwin_next;
    cf32 *ya, *yb;
    unsigned long long need, ny, split;
    int Ls, M, p, old, bps, run;
    float gain, scale;
    unsigned s0, g, nmask;
    int Lr, bits;
    uint32_t step, p0;
    int wg_outputs;             // outputs per workgroup: a multiple of resamp_plan's tile
    unsigned sam_off, tab_off;  // byte offsets of the samples and of tab in LDS; the jumped state follows tab
};

__global__ void __launch_bounds__(256) symstreamr_kernel(const SymRArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    cf32 *xs = reinterpret_cast<cf32 *>(smem);                            // symbol values
    cf32 *ss = reinterpret_cast<cf32 *>(smem + a.sam_off);                // samples
    cf32 *tab = reinterpret_cast<cf32 *>(smem + a.tab_off);
    unsigned *jumped = reinterpret_cast<unsigned *>(smem + a.tab_off + (size_t)a.M * sizeof(cf32));

    const int tid = (int)threadIdx.x;
    const int Ls = a.Ls, Lr = a.Lr;
    const unsigned long long j0 = (unsigned long long)blockIdx.x * (unsigned)a.wg_outputs;
    const int nt = (int)std::min((unsigned long long)a.wg_outputs, a.ny - j0);
    const unsigned long long a0 = (unsigned long long)a.p0 + j0 * a.step;
    const long long i_first = (long long)(a0 >> 24), i_last = (long long)((a0 + (unsigned long long)(nt - 1) * a.step) >> 24);
    const long long tbase = i_first - (Lr - 1);                           // sample index of ss[0]
    const int tspan = (int)(i_last - i_first) + Lr;
    const int nrw = tbase < 0 ? (int)std::min((long long)tspan, -tbase) : 0;      // samples of the carried window
    const long long tc0 = tbase < 0 ? 0 : tbase;                          // first sample formed here
    const long long q_lo = (tc0 + a.p) >> 1, q_hi = (i_last + a.p) >> 1;  // their slots
    const int nslots = (int)(q_hi - q_lo) + 1;
    const long long xbase = q_lo - a.old - (Ls - 1);                      // index in X of xs[0]
    const int xspan = nslots + Ls - 1;
    const int nsw = xbase < 0 ? (int)std::min((long long)xspan, -xbase) : 0;      // symbols of the carried window
    const int ngen = xspan - nsw;                                         // symbols max(xbase, 0) .. + ngen - 1

    if (tid < 64 && ngen > 0) {                                           // the state at symbol max(xbase, 0): wave-uniform
        const unsigned long long off = (xbase < 0 ? 0ull : (unsigned long long)xbase) * (unsigned)a.bps;
        const unsigned s = sym_jump(a.pow, a.s0, off);
        if (tid == 0) *jumped = s;
    }
    for (int i = tid; i < a.M; i += 256) tab[i] = mul(a.map[i], a.gain);
    for (int i = tid; i < nsw; i += 256) xs[i] = a.swin[Ls + xbase + i];
    for (int i = tid; i < nrw; i += 256) ss[i] = a.rwin[Lr + tbase + i];
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (wave * 64 * a.run < ngen)                                         // wave-uniform
        sym_lane_fill(a.stride, *jumped, tid, a.run, a.bps, a.g, a.nmask, tab, xs + nsw, ngen);
    __syncthreads();

    const bool last_wg = blockIdx.x == gridDim.x - 1;
    if (last_wg && a.swin_next != nullptr)                                // the last Ls entries of X end the span
        for (int j = tid; j < Ls; j += 256) a.swin_next[j] = xs[nslots - 1 + j];

    // the samples: a lane owns a slot and forms its two branches
    const float *h0 = a.shb, *h1 = a.shb + Ls;
    for (int ql = tid; ql < nslots; ql += 256) {
        const cf32 *xr = xs + ql + (Ls - 1);                              // tap j reads xr[-j]
        const long long t = (q_lo + ql) * 2 - a.p;                        // the sample of branch 0
        const bool in0 = t >= tc0 && t <= i_last, in1 = t + 1 >= tc0 && t + 1 <= i_last;
        if (in0) ss[t - tbase] = pfb_branch_dot(xr, h0, Ls, a.scale);
        if (in1) ss[t + 1 - tbase] = pfb_branch_dot(xr, h1, Ls, a.scale);
        else if (last_wg && t + 1 > i_last) a.buf[1] = pfb_branch_dot(xr, h1, Ls, a.scale);
    }
    __syncthreads();

    if (last_wg)                                                          // samples need - Lr .. need - 1 end the span
        for (int j = tid; j < Lr; j += 256) a.rwin_next[j] = ss[tspan - Lr + j];

    const int shift = 24 - a.bits;
    for (int o = tid; o < nt; o += 256) {
        const unsigned long long aj = a0 + (unsigned long long)o * a.step;
        const int li = (int)((long long)(aj >> 24) - i_first);
        const uint32_t br = ((uint32_t)aj & 0xFFFFFFu) >> shift;
        const cf32 v = resamp_branch_dot<cf32, float>(ss + (Lr - 1) + li, a.rhb + (size_t)br * Lr, Lr);
        const unsigned long long j = j0 + (unsigned)o;
        if (j < a.split) a.ya[j] = v;
        else a.yb[j - a.split] = v;
    }
}

// upper bounds over every starting phase: samples and symbols a workgroup of `outputs` outputs stages
size_t symr_samples(size_t outputs, uint32_t step, int Lr) { return (size_t)resamp_span(outputs, step, Lr); }
size_t symr_symbols(size_t outputs, uint32_t step, int Lr, int Ls) {
    return symr_samples(outputs, step, Lr) / 2 + 1 + (size_t)Ls;          // slots of the samples + Ls - 1 of history
}
size_t symr_lds(size_t outputs, uint32_t step, int Lr, int Ls, int M) {
    return round16(symr_symbols(outputs, step, Lr, Ls) * sizeof(cf32)) + round16(symr_samples(outputs, step, Lr) * sizeof(cf32)) +
           (size_t)M * sizeof(cf32) + 16;
}

}  // namespace

int symstreamr_tile(uint32_t step, int Lr) { return resamp_plan(sizeof(cf32), Lr, step).tile; }

int symstreamr_max_tiles(uint32_t step, int Lr, int Ls, int run) {
    const int tile = symstreamr_tile(step, Lr);
    if (tile == 0) return 0;
    int g = 0;
    while (g < 64) {
        const size_t out = (size_t)(g + 1) * tile;
        const size_t bytes = round16(symr_symbols(out, step, Lr, Ls) * sizeof(cf32)) + round16(symr_samples(out, step, Lr) * sizeof(cf32));
        if (symr_symbols(out, step, Lr, Ls) > (size_t)256 * (size_t)run) break;        // what the lanes generate
        if (bytes > (g == 0 ? kSymRLdsLimit - 256 * sizeof(cf32) - 16 : kSymRSpanBudget)) break;  // one tile: whatever fits
        ++g;
    }
    return g;
}

int symstreamr_wg_tiles(uint32_t step, int Lr, int Ls, int run, size_t ny) {
    const int tile = symstreamr_tile(step, Lr), gmax = symstreamr_max_tiles(step, Lr, Ls, run);
    if (tile == 0 || gmax == 0) return 0;
    const size_t tiles = (ny + (size_t)tile - 1) / (size_t)tile;
    const size_t g = std::min((tiles + kSymRTargetWgs - 1) / kSymRTargetWgs, (size_t)gmax);
    return (int)std::max(g, (size_t)1);
}

size_t symstreamr_lds_bytes(uint32_t step, int Lr, int Ls, int M, int wg_tiles) {
    return symr_lds((size_t)wg_tiles * symstreamr_tile(step, Lr), step, Lr, Ls, M);
}

bool symstreamr_fused_serves(uint32_t step, int Lr, int Ls, int M, int run) {
    if (step == 0 || Lr < 1 || Ls < 1 || M < 2 || M > 256 || run < 1) return false;
    if (firpfb_all_plan(sizeof(cf32), sizeof(float), 2, Ls).kind != kPfbPlanFew) return false;   // the chain formed here
    if (symstreamr_max_tiles(step, Lr, Ls, run) < 1) return false;
    return symstreamr_lds_bytes(step, Lr, Ls, M, 1) <= kSymRLdsLimit;
}

int launch_symstreamr(const cf32 *swin, const float *shb, int Ls, float scale, const cf32 *map, int M, float gain,
                      const SymSource &src, int p, const cf32 *rwin, const float *rhb, int Lr, int bits, uint32_t step,
                      uint32_t p0, size_t need, size_t ny, cf32 *ya, size_t split, cf32 *yb, cf32 *swin_next,
                      cf32 *rwin_next, cf32 *buf, hipStream_t st) {
    if (need == 0 || ny == 0) return fail(YAGI_ERR_INTERNAL, "symstreamr: an empty call");
    if (!symstreamr_fused_serves(step, Lr, Ls, M, src.run)) return fail(YAGI_ERR_INTERNAL, "symstreamr: no fused kernel for this shape");
    if (p < 0 || p > 1) return fail(YAGI_ERR_INTERNAL, "symstreamr: buf_index out of range");
    if (bits < 1 || bits > 16) return fail(YAGI_ERR_INTERNAL, "symstreamr: bad schedule (bits %d)", bits);
    if (src.bps < 1 || src.bps > 8 || (1 << src.bps) != M) return fail(YAGI_ERR_INTERNAL, "symstreamr: bps does not match M");
    if (split > ny) return fail(YAGI_ERR_INTERNAL, "symstreamr: split beyond the call");
    if (((uintptr_t)ya | (uintptr_t)yb) & 7) return fail(YAGI_ERR_CONFIG, "symstreamr: sample buffers must be 8-byte aligned");
    // the schedule must be the call's: output ny - 1 is the last one sample need - 1 gives, output ny needs another
    const unsigned __int128 end = (unsigned __int128)need << 24;
    const unsigned __int128 a_last = (unsigned __int128)p0 + (unsigned __int128)(ny - 1) * step;
    if ((a_last >> 24) != (unsigned __int128)(need - 1) || a_last + step < end)
        return fail(YAGI_ERR_INTERNAL, "symstreamr: output count does not match the schedule");
    SymRArgs a{};
    a.swin = swin;
    a.shb = shb;
    a.map = map;
    a.pow = src.pow;
    a.stride = src.stride + 32 * ((src.bps - 1) * kSymStrides);
    a.buf = buf;
    a.rwin = rwin;
    a.rhb = rhb;
    a.rwin_next = rwin_next;
    a.ya = ya;
    a.yb = yb;
    a.need = need;
    a.ny = ny;
    a.split = split;
    a.Ls = Ls;
    a.M = M;
    a.p = p;
    a.old = p > 0 ? 1 : 0;
    a.swin_next = ((size_t)p + need + 1) / 2 > (size_t)a.old ? swin_next : nullptr;
    a.bps = src.bps;
    a.run = src.run;
    a.gain = gain;
    a.scale = scale;
    a.s0 = src.s0;
    a.g = src.g;
    a.nmask = src.nmask;
    a.Lr = Lr;
    a.bits = bits;
    a.step = step;
    a.p0 = p0;
    const int tile = symstreamr_tile(step, Lr), g = symstreamr_wg_tiles(step, Lr, Ls, src.run, ny);
    a.wg_outputs = tile * g;
    a.sam_off = (unsigned)round16(symr_symbols((size_t)a.wg_outputs, step, Lr, Ls) * sizeof(cf32));
    a.tab_off = a.sam_off + (unsigned)round16(symr_samples((size_t)a.wg_outputs, step, Lr) * sizeof(cf32));
    const size_t lds = symr_lds((size_t)a.wg_outputs, step, Lr, Ls, M);
    if (lds > kSymRLdsLimit) return fail(YAGI_ERR_INTERNAL, "symstreamr: LDS request out of range");
    const size_t nblk = (ny + (size_t)a.wg_outputs - 1) / (size_t)a.wg_outputs;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    symstreamr_kernel<<<(unsigned)nblk, 256, lds, st>>>(a);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

}  // namespace yagi
