// symstream_kernels.hip -- SymStream (src/framing/symstream.rs): symbol source, modulator and pulse shaper in one launch.
//
// A call writes samples [t0, t0 + n) of the stream, t0 = (symbols pushed so far) * k - (k - p) % k with p = buf_index.  In
// symbol SLOTS: slot q of the call holds the samples of one symbol, the call's samples are (q, branch i) with
// q * k + i - p in [0, n).  Where p > 0, slot 0 is the symbol the previous call pushed (`old` = 1: its value is the newest
// entry of the carried window); every other slot is a new symbol.  With X = window ++ new symbols, slot q reads
// X[q - old - j], j = 0 .. Ls-1: the interpolator's bank kernels (fir_bodies.hpp: firpfb_fewbranch_body,
// firpfb_all_body) over nslots inputs, with the outputs shifted by p and guarded by the call's range.
//
// The sums are those bodies' sums: the variant comes from the same firpfb_all_plan(8, 4, k, Ls), a lane walks the taps
// j = 0 .. Ls-1 with the same mac and ends with the same mul by the scale (1), so a shape reaches the same words fused
// or through FirInterpolationFilter.  What differs is where the span in LDS comes from:
//   carried window entries (stream index < 0)   copied as values
//   new symbol idx >= 0                         tab[s], tab[s] = map[s] * gain computed once per workgroup into LDS behind
//                                               the span (two f32 products, no multiply in the hot loop)
//   s, modulate_symbols                         the caller's byte sym[idx]; symstream_check_kernel has range-checked the
//                                               block into `flag` first, and a set flag ends every workgroup before it
//                                               writes anything
//   s, write_samples                            no input at all: the first wave jumps the LFSR to the workgroup's first
//                                               new symbol with the T^(2^b) matrices (wave-uniform: scalar registers and
//                                               scalar loads, as msequence_gen_kernel) and leaves the state in LDS; a
//                                               lane adds tid * run symbols with the eight lane-stride matrices
//                                               T^(run * bps * 2^b) of the object, then steps its `run` symbols and
//                                               leaves tab[s] in the span.  Waves whose symbols lie beyond the span skip
//                                               their part.
// The jump costs a few thousand scalar instructions (one matrix of m columns per set bit of the offset), far more than
// the sums of a 256-symbol tile at small k, so a workgroup owns `wg_slots` = G tiles of the bank kernels' size (256
// slots few-branch, 64 otherwise) and stages the span of all of them at once: one jump per G tiles.  The host picks G
// per call so that a long call still has about a thousand workgroups and a short one runs one tile per workgroup;
// symstream_max_slots bounds it by the LDS.  `run` is fixed per object for the largest G (the lane strides are built
// for it); with a smaller G fewer lanes generate.  The sums do not depend on G.
// The last workgroup writes the window the call leaves (the last Ls entries of X, all of them in its span) into the
// object's other window buffer, and the branches of the last slot that lie beyond the call's range into `buf` (the
// reference's buf: what a following call through the three-launch route copies from).
//
// LDS, all dynamic: [span | taps (kPfbPlanTapsLds) | tab | the jumped state], every part on a 16-byte boundary.  No
// scratch.  Every global access is guarded: win in [0, Ls), sym in [0, nnew), y in [0, n), buf in [0, k), win_next in
// [0, Ls), map in [0, M).
#include <algorithm>
#include <cstdint>

#include "fir_bodies.hpp"
#include "kernels.hpp"

namespace yagi {
namespace {

constexpr size_t kSymLdsLimit = 64 * 1024;
inline size_t round16(size_t b) { return (b + 15) / 16 * 16; }

struct SymArgs {
    const cf32 *win;            // Ls entries, oldest first
    const float *hb;            // [k][Ls]
    const cf32 *map;            // M points
    const uint8_t *sym;         // nnew bytes (modulate_symbols) or null
    const int *flag;            // range-check result of sym, or null (M = 256: every byte is a symbol)
    const unsigned *pow, *stride;
    cf32 *y, *win_next, *buf;
    size_t n, nslots, nnew;
    int k, Ls, M, p, old;
    float gain, scale;
    unsigned s0, g, nmask;
    int bps, run;
    int wg_slots;               // slots per workgroup: a multiple of the bank kernels' tile
    unsigned taps_off, tab_off; // byte offsets of the transposed taps and of tab in LDS; the jumped state follows tab
};

template <int PLAN, bool LFSR>
__global__ void __launch_bounds__(256) symstream_kernel(const SymArgs a) {
    const int TN = a.wg_slots;
    extern __shared__ __align__(16) unsigned char smem[];
    cf32 *xs = reinterpret_cast<cf32 *>(smem);                            // TN + Ls - 1 values
    cf32 *tab = reinterpret_cast<cf32 *>(smem + a.tab_off);
    float *hsT = reinterpret_cast<float *>(smem + a.taps_off);
    unsigned *jumped = reinterpret_cast<unsigned *>(smem + a.tab_off + (size_t)a.M * sizeof(cf32));
    if (!LFSR && a.flag != nullptr && *a.flag) return;                    // uniform: nothing is written

    const int tid = (int)threadIdx.x;
    const int k = a.k, Ls = a.Ls;
    const size_t n0 = (size_t)blockIdx.x * TN;                            // first slot of the workgroup
    const int nt = (int)std::min((size_t)TN, a.nslots - n0);
    const long long base = (long long)n0 - a.old - (Ls - 1);              // stream index of xs[0]
    const int span = nt + Ls - 1;
    const int nwin = base < 0 ? (int)std::min((long long)span, -base) : 0;
    if (LFSR && tid < 64) {                                               // the state at symbol max(base, 0): wave-uniform
        const unsigned long long off = (base < 0 ? 0ull : (unsigned long long)base) * (unsigned)a.bps;
        const unsigned s = sym_jump(a.pow, a.s0, off);                    // fir_bodies.hpp
        if (tid == 0) *jumped = s;
    }
    for (int i = tid; i < a.M; i += 256) tab[i] = mul(a.map[i], a.gain);
    if (PLAN == kPfbPlanTapsLds)
        for (int e = tid; e < k * Ls; e += 256) {
            const int i = e / Ls, j = e - i * Ls;
            hsT[j * k + i] = a.hb[e];
        }
    __syncthreads();

    for (int i = tid; i < nwin; i += 256) xs[i] = a.win[Ls + base + i];
    if (LFSR) {
        const int ngen = span - nwin;                                     // symbols max(base, 0) .. + ngen - 1
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        if (wave * 64 * a.run < ngen)                                     // wave-uniform
            sym_lane_fill(a.stride, *jumped, tid, a.run, a.bps, a.g, a.nmask, tab, xs + nwin, ngen);
    } else {
        for (int i = nwin + tid; i < span; i += 256) xs[i] = tab[a.sym[base + i]];
    }
    __syncthreads();

    const bool last_wg = blockIdx.x == gridDim.x - 1;
    if (a.win_next != nullptr && last_wg)                                 // the last Ls entries of X end the span
        for (int j = tid; j < Ls; j += 256) a.win_next[j] = xs[nt - 1 + j];

    const long long n = (long long)a.n;
    auto store = [&](long long o, int i, bool last_slot, cf32 v) {
        if (o >= 0 && o < n) a.y[o] = v;
        else if (last_slot && o >= n) a.buf[i] = v;
    };
    if (PLAN == kPfbPlanFew) {
        for (int nl = tid; nl < nt; nl += 256) {
            const cf32 *xr = xs + nl + (Ls - 1);                          // tap j reads xr[-j]
            const long long ob = (long long)(n0 + nl) * k - a.p;
            const bool last_slot = n0 + nl == a.nslots - 1;
            const bool whole = ob >= 0 && ob + k <= n;                    // every branch of the slot lies in the call
            cf32 *yo = a.y + ob;                                          // used where whole
            int g0 = 0;
            for (; g0 + 4 <= k; g0 += 4) {
                const float *h0 = a.hb + (size_t)g0 * Ls;
                cf32 acc[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = zero_of<cf32>();
#pragma unroll 4
                for (int t = 0; t < Ls; ++t) {
                    const cf32 sk = xr[-t];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = mac(acc[j], sk, h0[(size_t)j * Ls + t]);
                }
                if (whole) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) yo[g0 + j] = mul(acc[j], a.scale);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) store(ob + g0 + j, g0 + j, last_slot, mul(acc[j], a.scale));
                }
            }
            for (; g0 < k; ++g0) {                                        // the last k % 4 branches
                const float *h0 = a.hb + (size_t)g0 * Ls;
                const cf32 v = pfb_branch_dot(xr, h0, Ls, a.scale);       // fir_bodies.hpp
                if (whole) yo[g0] = v;
                else store(ob + g0, g0, last_slot, v);
            }
        }
    } else {
        const int total = nt * k;
        for (int e = tid; e < total; e += 256) {
            const int nl = e / k, i = e - nl * k;
            cf32 acc = zero_of<cf32>();
            for (int t = 0; t < Ls; ++t) {
                const float ht = PLAN == kPfbPlanTapsLds ? hsT[t * k + i] : a.hb[i * Ls + t];
                acc = mac(acc, xs[nl + (Ls - 1) - t], ht);
            }
            store((long long)(n0 + nl) * k + i - a.p, i, n0 + nl == a.nslots - 1, mul(acc, a.scale));
        }
    }
}

constexpr int kChkTile = 4096;

__global__ void __launch_bounds__(256) symstream_check_kernel(int M, const uint8_t *__restrict__ sym, size_t n, int *flag) {
    const size_t base = (size_t)blockIdx.x * kChkTile;
    const int cnt = (int)std::min((size_t)kChkTile, n - base);
    bool bad = false;
    for (int i = threadIdx.x; i < cnt; i += 256) bad |= (int)sym[base + i] >= M;
    if (bad) atomicOr(flag, 1);
}

__global__ void __launch_bounds__(256) symstream_gain_kernel(cf32 *__restrict__ v, size_t n, float gain) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = mul(v[i], gain);
}

template <int PLAN>
void run_symstream(unsigned nblk, size_t lds, hipStream_t st, const SymArgs &a, bool lfsr) {
    if (lfsr) symstream_kernel<PLAN, true><<<nblk, 256, lds, st>>>(a);
    else symstream_kernel<PLAN, false><<<nblk, 256, lds, st>>>(a);
}

}  // namespace

namespace {
constexpr size_t kSymSpanBudget = 40 * 1024;       // the span of a workgroup's G tiles: leaves three workgroups per CU
constexpr size_t kSymTabMax = 256 * sizeof(cf32) + 16;
constexpr size_t kSymTargetWgs = 1024;             // a long call keeps about this many workgroups (four per CU)
int sym_tile(const FirPfbPlan &p) { return p.kind == kPfbPlanFew ? 256 : kPfbTN; }
size_t sym_taps_bytes(const FirPfbPlan &p, int k, int Ls) { return p.kind == kPfbPlanTapsLds ? (size_t)k * Ls * sizeof(float) : 0; }
size_t sym_lds(const FirPfbPlan &p, int k, int Ls, int M, int wg_slots) {
    return round16((size_t)(wg_slots + Ls - 1) * sizeof(cf32)) + round16(sym_taps_bytes(p, k, Ls)) + (size_t)M * sizeof(cf32) + 16;
}
}  // namespace

int symstream_max_slots(int k, int Ls) {
    const FirPfbPlan p = firpfb_all_plan(sizeof(cf32), sizeof(float), k, Ls);
    const int tn = sym_tile(p);
    const size_t room = kSymLdsLimit - kSymTabMax - round16(sym_taps_bytes(p, k, Ls)) - 16;
    const size_t entries = std::min(kSymSpanBudget, room) / sizeof(cf32);
    if (entries < (size_t)(tn + Ls - 1)) return tn;
    return (int)((entries - (size_t)(Ls - 1)) / tn) * tn;
}

int symstream_run(int k, int Ls) { return (symstream_max_slots(k, Ls) + Ls - 1 + 255) / 256; }

void symstream_strides(const unsigned *pow, int run, unsigned *stride) {
    for (int bps = 1; bps <= 8; ++bps)
        for (int b = 0; b < kSymStrides; ++b) {
            unsigned *S = stride + 32 * ((bps - 1) * kSymStrides + b);
            for (int j = 0; j < 32; ++j) S[j] = msequence_skip(pow, 1u << j, (uint64_t)(run * bps) << b);
        }
}

size_t symstream_lds_bytes(int k, int Ls, int M, int wg_slots) {
    return sym_lds(firpfb_all_plan(sizeof(cf32), sizeof(float), k, Ls), k, Ls, M, wg_slots);
}

int symstream_wg_slots(int k, int Ls, size_t nslots) {
    const FirPfbPlan p = firpfb_all_plan(sizeof(cf32), sizeof(float), k, Ls);
    const size_t tn = (size_t)sym_tile(p), tiles = (nslots + tn - 1) / tn;
    const size_t g = std::min((tiles + kSymTargetWgs - 1) / kSymTargetWgs, (size_t)symstream_max_slots(k, Ls) / tn);
    return (int)(std::max(g, (size_t)1) * tn);
}

bool symstream_fused_serves(int k, int Ls, int M) {
    if (k < 2 || Ls < 1 || M < 2 || M > 256) return false;
    const FirPfbPlan p = firpfb_all_plan(sizeof(cf32), sizeof(float), k, Ls);
    if (p.kind == kPfbPlanNone) return false;
    return sym_lds(p, k, Ls, M, sym_tile(p)) <= kSymLdsLimit;
}

int launch_symstream(const cf32 *win, const float *hb, int k, int Ls, float scale, const cf32 *map, int M, float gain,
                     const uint8_t *sym, const int *flag, const SymSource *src, int p, size_t n, cf32 *y, cf32 *win_next,
                     cf32 *buf, hipStream_t st) {
    if (n == 0) return YAGI_OK;
    if (!symstream_fused_serves(k, Ls, M)) return fail(YAGI_ERR_INTERNAL, "symstream: no fused kernel for this shape");
    if (p < 0 || p >= k) return fail(YAGI_ERR_INTERNAL, "symstream: buf_index out of range");
    if ((sym == nullptr) == (src == nullptr)) return fail(YAGI_ERR_INTERNAL, "symstream: one symbol source per call");
    if ((uintptr_t)y & 7) return fail(YAGI_ERR_CONFIG, "symstream: sample buffers must be 8-byte aligned");
    const FirPfbPlan plan = firpfb_all_plan(sizeof(cf32), sizeof(float), k, Ls);
    SymArgs a{};
    a.win = win;
    a.hb = hb;
    a.map = map;
    a.sym = sym;
    a.flag = flag;
    a.y = y;
    a.buf = buf;
    a.n = n;
    a.old = p > 0 ? 1 : 0;
    a.nslots = ((size_t)p + n + (size_t)k - 1) / (size_t)k;
    a.nnew = a.nslots - (size_t)a.old;
    a.win_next = a.nnew ? win_next : nullptr;
    a.k = k;
    a.Ls = Ls;
    a.M = M;
    a.p = p;
    a.gain = gain;
    a.scale = scale;
    a.wg_slots = symstream_wg_slots(k, Ls, a.nslots);
    a.taps_off = (unsigned)round16((size_t)(a.wg_slots + Ls - 1) * sizeof(cf32));
    a.tab_off = a.taps_off + (unsigned)round16(sym_taps_bytes(plan, k, Ls));
    if (src) {
        if (src->bps < 1 || src->bps > 8 || (1 << src->bps) != M) return fail(YAGI_ERR_INTERNAL, "symstream: bps does not match M");
        if (src->run != symstream_run(k, Ls)) return fail(YAGI_ERR_INTERNAL, "symstream: lane strides of another shape");
        a.pow = src->pow;
        a.stride = src->stride + 32 * ((src->bps - 1) * kSymStrides);
        a.s0 = src->s0;
        a.g = src->g;
        a.nmask = src->nmask;
        a.bps = src->bps;
        a.run = src->run;
    }
    const size_t nblk = (a.nslots + (size_t)a.wg_slots - 1) / (size_t)a.wg_slots;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    const size_t lds = sym_lds(plan, k, Ls, M, a.wg_slots);
    if (lds > kSymLdsLimit) return fail(YAGI_ERR_INTERNAL, "symstream: LDS request out of range");
    if (plan.kind == kPfbPlanFew) run_symstream<kPfbPlanFew>((unsigned)nblk, lds, st, a, src != nullptr);
    else if (plan.kind == kPfbPlanTapsLds) run_symstream<kPfbPlanTapsLds>((unsigned)nblk, lds, st, a, src != nullptr);
    else run_symstream<kPfbPlanTapsGlobal>((unsigned)nblk, lds, st, a, src != nullptr);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

int launch_symstream_check(int M, const uint8_t *sym, size_t n, int *flag, hipStream_t st) {
    YG_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    if (n == 0 || M >= 256) return YAGI_OK;
    const size_t nblk = (n + kChkTile - 1) / kChkTile;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    symstream_check_kernel<<<(unsigned)nblk, 256, 0, st>>>(M, sym, n, flag);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

int launch_symstream_gain(cf32 *v, size_t n, float gain, hipStream_t st) {
    if (n == 0) return YAGI_OK;
    const size_t nblk = (n + 255) / 256;
    if (nblk > 0x7fffffffull) return fail(YAGI_ERR_CONFIG, "block too large");
    symstream_gain_kernel<<<(unsigned)nblk, 256, 0, st>>>(v, n, gain);
    YG_LAUNCH_CHECK();
    return YAGI_OK;
}

}  // namespace yagi
