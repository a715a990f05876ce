// kernels.hpp -- launcher declarations shared by the kernel translation units and capi.hip.
// Every launcher is asynchronous on `st`, performs no allocation and no host synchronisation
// (so a caller may capture it into a hipGraph), and returns a yagi_status.
#pragma once
#include <cstdint>
#include <utility>

#include "common.hpp"

namespace yagi {

// Type combinations of the FIR family (T = sample/output type, C = coefficient type).
struct RRRF { using T = float; using C = float; static constexpr int id = 0; };
struct CRCF { using T = cf32;  using C = float; static constexpr int id = 1; };
struct CCCF { using T = cf32;  using C = cf32;  static constexpr int id = 2; };

// ---- comm.cpp --------------------------------------------------------------------------------
}  // namespace yagi
// RCCL communicator handle of the C ABI (yagi_hip_comm): the ncclComm_t, this rank, a side stream for the collectives
// and the events that chain it to an object's stream
struct yagi_hip_comm_s {
    void *nccl = nullptr;
    int rank = 0, nranks = 1;
    hipStream_t st = nullptr;
    std::vector<hipEvent_t> ev;
    hipEvent_t done = nullptr;
};
namespace yagi {
using Comm = yagi_hip_comm_s;
// all-gather `bytes_per_rank` bytes from every rank into recv (rank-major), asynchronous on st
int comm_all_gather(Comm *c, const void *send, void *recv, size_t bytes_per_rank, hipStream_t st);

// ---- misc_kernels.hip ----------------------------------------------------------------------
int launch_gen_real(uint64_t seed, uint64_t first, size_t n, float *x, hipStream_t st);
int launch_gen_complex(uint64_t seed, uint64_t first, size_t n, cf32 *x, hipStream_t st);

// y[0] = post * sum_i a[i] * b[rev ? n-1-i : i]; `partials` needs dotprod_num_partials(n)
// elements of the output type.  Fixed-order two-pass combine => bitwise reproducible.
size_t dotprod_num_partials(size_t n);
template <class A, class B, class O, class S>
int launch_dotprod(const A *a, const B *b, size_t n, bool rev_b, S post, O *partials, O *y,
                   hipStream_t st);

// new_win = last L samples of (old_win ++ x[0..n))
template <class T>
int launch_update_window(const T *old_win, const T *x, size_t n, int L, T *new_win, hipStream_t st);

// ---- fir_kernels.hip -----------------------------------------------------------------------
// y[i] = scale * sum_{k<L} h[k] * X[i*M - k],  X = win(L samples, oldest first) ++ x,
// X index 0 = x[0].  i in [0, ny).  taps in natural order h[0..L).
template <class K>
int launch_fir_block(const typename K::T *win, const typename K::T *x, const typename K::C *taps,
                     int L, int M, typename K::C scale, typename K::T *y, size_t ny, hipStream_t st,
                     size_t x_len = 0 /* samples readable at x; 0 = ny*M */,
                     typename K::T *win_next = nullptr /* if set: receives the window after the block (last L samples of
                                                          win ++ x[0..ny*M)), written by the kernel's last workgroup */);

// polyphase bank, all branches per input sample: y[n*nf + i] = scale * sum_k hb[i][k] X[n-k]
// branch taps hb laid out [nf][Ls] in natural (newest-first) order.
template <class K>
int launch_firpfb_all(const typename K::T *win, const typename K::T *x, const typename K::C *hb,
                      int nf, int Ls, typename K::C scale, typename K::T *y, size_t n, hipStream_t st,
                      typename K::T *win_next = nullptr /* see launch_fir_block */);
// branch chosen per sample: y[n] = scale * sum_k hb[idx[n]][k] X[n-k]
template <class K>
int launch_firpfb_select(const typename K::T *win, const typename K::T *x, const typename K::C *hb,
                         const uint32_t *idx, int nf, int Ls, typename K::C scale,
                         typename K::T *y, size_t n, hipStream_t st);

// Rresamp: y[blk*P + n] = scale * sum_k hb[(n*Q) % P][k] X[blk*Q + (n*Q)/P - k], n < P, blk < nblocks
template <class K>
int launch_rresamp(const typename K::T *win, const typename K::T *x, const typename K::C *hb, int P, int Q,
                   int Ls, typename K::C scale, typename K::T *y, size_t nblocks, hipStream_t st,
                   typename K::T *win_next = nullptr /* see launch_fir_block */);

// Resamp: ny outputs of one call of nx inputs that starts at phase p0 (u32, 24 fractional bits):
// A_j = p0 + j*step,  y[j] = sum_k hb[(A_j & 0xFFFFFF) >> (24-bits)][k] X[(A_j >> 24) - k].  Branches hb [2^bits][Ls].
// win_next: the window after all nx inputs (see launch_fir_block); the caller handles ny == 0 itself.
template <class K>
int launch_resamp(const typename K::T *win, const typename K::T *x, const typename K::C *hb, int Ls, int bits,
                  uint32_t step, uint32_t p0, typename K::T *y, size_t ny, size_t nx, hipStream_t st,
                  typename K::T *win_next = nullptr);

// ---- stream_kernels.hip (crcf M=1 hot case; headline fused FIR -> 4096-pt FFT) -----------------
// taps_pad = h zero-padded to Lp = roundup(L, 32) floats.
constexpr int kSlideMaxTaps = 1024;
int launch_fir_crcf_slide(const cf32 *win, const cf32 *x, const float *taps_pad, int L, int Lp,
                          float scale, cf32 *y, size_t ny, hipStream_t st, cf32 *win_next = nullptr);
int launch_firfft_crcf_4096(const cf32 *win, const cf32 *x, const float *taps_pad, const float *apack,
                            int L, int Lp, int Lm, float scale, const cf32 *tw4096, cf32 *spectra,
                            size_t nframes, int variant, hipStream_t st);
// MFMA Toeplitz form (L <= 256): Lm = mfma_lp_for(L) in {64,128,256} (0 = unsupported);
// apack = pack_toeplitz_taps(h, L, Lm), toeplitz_pack_floats(Lm) floats.
int mfma_lp_for(int L);
size_t toeplitz_pack_floats(int Lp);
void pack_toeplitz_taps(const float *h, int L, int Lp, float *apack_host);
int launch_fir_crcf_mfma(const cf32 *win, const cf32 *x, const float *apack, int L, int Lm, float scale,
                         cf32 *y, size_t ny, hipStream_t st, cf32 *win_next = nullptr);

// Fast convolution (overlap-save, 4096-pt blocks) form of firfilt_crcf: hs = FFT_4096{[h;0]} (unscaled),
// forward table twf, backward table twb; 1 <= L <= 2049.
// x[-pre .. x_avail) must be readable (chunked processing of one long block); ny outputs are produced.
int launch_fir_crcf_fftconv(const cf32 *win, const cf32 *x, size_t pre, size_t x_avail, const cf32 *hs,
                            float scale, int L, const cf32 *twf, const cf32 *twb, cf32 *y, size_t ny,
                            hipStream_t st, cf32 *win_next = nullptr);
// win_next (optional): receives the filter window after the call, the last L samples of win ++ x[0, x_avail)
// same kernel for complex taps (hs = FFT of the complex taps, complex scale) and for real samples (two
// blocks per transform as its real and imaginary parts)
int launch_fir_cccf_fftconv(const cf32 *win, const cf32 *x, size_t pre, size_t x_avail, const cf32 *hs,
                            cf32 scale, int L, const cf32 *twf, const cf32 *twb, cf32 *y, size_t ny,
                            hipStream_t st, cf32 *win_next = nullptr);
int launch_fir_rrrf_fftconv(const float *win, const float *x, size_t pre, size_t x_avail, const cf32 *hs,
                            float scale, int L, const cf32 *twf, const cf32 *twb, float *y, size_t ny,
                            hipStream_t st, float *win_next = nullptr);

// frequency-domain form of the firfilt_crcf -> 4096-pt FFT stream (1 <= L <= 257): FFT{h}.FFT{x_f} + FFT{boundary
// correction}; hs_scaled = scale * FFT{h} and gfft_scaled = scale * conj(DFT_512{g}) / 512, g[j] = h[L-1-j], both in the
// pair layout of launch_scale_cf32_pairs (256 and 64 lanes); tw_stream = the table of make_stream_twiddles (capi.hip,
// stream_tables.hpp: all kStreamTabFloat2 entries); win_next <- last L samples of x.
int launch_firfft_crcf_4096_freq(const cf32 *win, const cf32 *x, const cf32 *hs_scaled, const cf32 *gfft_scaled,
                                 int L, const cf32 *tw_stream, cf32 *spectra, cf32 *win_next, size_t nframes,
                                 hipStream_t st);

// dst = s * src, entry l + lanes d (l < lanes, d < n / lanes) in slot stream_pair_slot(l, d, lanes) (stream_tables.hpp):
// lane l's entries d and d + 1 (d even) side by side, the layout of the stream kernel's 16-byte table loads
int launch_scale_cf32_pairs(const cf32 *src, float s, cf32 *dst, unsigned lanes, size_t n, hipStream_t st);

// ---- resamp2_kernels.hip -------------------------------------------------------------------
// forms of Resamp2 (resamp2.rs:104-180); values are the `mode` argument of the C ABI
enum { kR2Filter = 0, kR2Analyzer = 1, kR2Synthesizer = 2, kR2Decim = 3, kR2Interp = 4 };
constexpr int kR2MaxSemiLen = 1024;
// MsResamp2 decimator chain in one launch (resamp2_kernels.hip): stages in processing order (full rate first)
template <class T, class C>
int launch_msresamp2_decim(int ns, const int *m, const C *scale, const C *const *h1, const T *const *state,
                           T *const *state_next, const T *x, T *y, size_t nout, hipStream_t st);
// MsResamp2 interpolator chain in one launch: stages in processing order (input rate first)
template <class T, class C>
int launch_msresamp2_interp(int ns, const int *m, const C *scale, const C *const *h1, const T *const *state,
                            T *const *state_next, const T *x, T *y, size_t nin, hipStream_t st);
// What the two launchers above do for a shape: host arithmetic, shared by the launchers, MsResamp2Obj's fused-or-chain
// choice, Resamp2Obj's decimator route and the plan queries (yagi_hip_plan_msresamp2 / _resamp2).  elem = bytes per sample.
struct MsFastGeom {
    int F;                      // final outputs per tile of msresamp2_decim_fast_kernel
    int n[3];                   // outputs of stage k per tile
    int cnt0;                   // input pairs per tile
    int U;                      // first input pair of a tile = 2^(S-1) * (its first output) - U
};
enum { kMsWalkGeneral = 0, kMsWalkR1 = 1, kMsWalkR2 = 2, kMsWalkR4Rho0 = 3, kMsWalkR4Rho2 = 4 };
struct MsDecimPlan {
    bool fused;                 // false: more than four stages or more than 64 KiB of LDS -- one launch per stage
    size_t lds, fast_lds;       // dynamic LDS of the general / the fast kernel
    long long head_tiles;       // general kernel: the outputs [0, 256 head_tiles) and [tail_first, nout)
    long long fast_tiles;       // fast kernel: fast_tiles tiles of geo.F outputs from 256 head_tiles on (0: not launched)
    long long tail_first;
    long long tiles;            // tiles of the general kernel, tpw consecutive ones per workgroup
    bool long_halo;             // a tile's stage-0 streams outgrow the per-lane registers: the instance that stages the rest from memory
    int tpw, fast_tpw;
    MsFastGeom geo;             // F = 0: no geometry with F >= 64 exists (or more than three stages)
    int walk[4], walk_q[4];     // fast kernel: tap walk of stage k (kMsWalk*) and its group count Q
};
MsDecimPlan msresamp2_decim_plan(int ns, const int *m, size_t elem, size_t nout);
struct MsInterpPlan {
    bool fused;
    size_t lds;
    size_t tiles;               // workgroups of 256 inputs
};
MsInterpPlan msresamp2_interp_plan(int ns, const int *m, size_t elem, size_t nin);
// a Resamp2 decimator block of nx samples runs as the one-stage case of the chain kernels (else resamp2_kernel)
inline bool resamp2_takes_chain(int mode, int m, size_t nx) {
    return mode == kR2Decim && nx >= ((size_t)1 << 19) && m <= 64;
}
// one block of nx input samples; state = [w0 (2m, oldest first)][w1 (2m)]; state_next receives the windows after the
// block (must not alias state).  Outputs: filter 2 nx ((y0,y1) pairs), analyzer / synthesizer nx, decim nx/2, interp 2 nx.
template <class T, class C>
int launch_resamp2(int mode, const T *state, const T *x, size_t nx, const C *h1, int m, C scale, int toggle, T *y,
                   T *state_next, hipStream_t st);

// ---- fft_kernels.hip -----------------------------------------------------------------------
struct FftPlanDev {
    int n = 0;
    int dir = 0;
    int nfac = 0;
    int fac[16] = {0};
    const cf32 *tw = nullptr;        // W_n^m, m in [0,n), sign per direction
    // Bluestein (chirp-z) form for sizes with a large prime factor: X = w . IFFT_m(FFT_m(x . w) . FFT_m(b)) / m
    int bs_m = 0;                    // 0 = not used; else the power-of-two convolution length >= 2n-1
    const cf32 *bs_w = nullptr;      // chirp w[k] = e^{-+ j pi k^2 / n}, k < n
    const cf32 *bs_bf = nullptr;     // FFT_m of the circular chirp filter conj(w[|k|])
    const cf32 *bs_twf = nullptr;    // W_m tables, forward / backward (8192: followed by the W_4096 table)
    const cf32 *bs_twb = nullptr;
    cf32 *bs_scratch = nullptr;      // 2 * bs_chunk * m points
    int bs_chunk = 0;                // transforms per pass through the scratch
    const FftPlanDev *bs_fwd = nullptr, *bs_bwd = nullptr;   // host pointers: the m-point plans (own resources when m > 8192)
    // four-step form above 8192 points: n = n1 * n2 (both <= 8192), column transforms, twiddle, row transforms
    int fs_n1 = 0, fs_n2 = 0;        // 0 = not used
    const FftPlanDev *fs_p1 = nullptr, *fs_p2 = nullptr;      // host pointers: the n1- and n2-point plans
    cf32 *fs_scratch = nullptr;      // 2 * fs_chunk * n points
    int fs_chunk = 0;
    const cf32 *fs_wn = nullptr;     // W_n table when both factors are powers of two <= 256: two-launch form, no transposes
    const cf32 *fs_wlo4 = nullptr, *fs_whi4 = nullptr; // four-step form: the same split tables for its twiddle transposition
    const cf32 *fs_wlo = nullptr, *fs_whi = nullptr;   // n = 256 n2 >= 2^16 (fft_tile256_kernel): W_n^j, j < 4096, and W_n^{4096 j}
};
constexpr int kFftMaxLds = 8192;     // complex points held in LDS by the one-kernel path
constexpr int kFftTwoPassMixedMax = 1024;  // n = n1 n2 with both factors up to this: two launches (fft_mixed_twopass_kernel)
constexpr size_t kFftMaxPow2 = (size_t)1 << 24;    // largest power of two (four-step); any other n up to 2^23 (Bluestein)
int launch_fft_batch(const FftPlanDev &p, const cf32 *in, cf32 *out, size_t batch, hipStream_t st);
// what launch_fft_batch does with this plan: its dispatch and its launchers' outer loops go through these three
yagi_hip_fft_path fft_path(const FftPlanDev &p);
size_t fft_batch_chunk(const FftPlanDev &p);                    // transforms per pass of that path's loop, 0 = no loop
bool fft_nested_plan(const FftPlanDev &p, FftPlanDev &sub);     // the plan the path hands its sub-transforms to, if any
void fft_describe(const FftPlanDev &p, yagi_hip_fft_info &info);
int launch_fft_shift(cf32 *buf, size_t n, size_t batch, hipStream_t st);

// ---- fftfilt_kernels.hip (FftFilt, src/filter/fftfilt.rs:103-138) ------------------------------------
template <class T>
int launch_fftfilt_pad(const T *x, int n, size_t nblocks, cf32 *time, hipStream_t st);
int launch_fftfilt_mul(cf32 *freq, const cf32 *hf, int n2, size_t nblocks, hipStream_t st);
template <class T, class C>
int launch_fftfilt_ola(const cf32 *t, const cf32 *w, int n, size_t nblocks, C scale, T *y, cf32 *w_next,
                       hipStream_t st);

// ---- spgram_kernels.hip (fft::Spgram, src/fft/spgram.rs:237-316) ---------------------------------------
template <class T>
int launch_spgram_frames(const T *win, const T *x, const float *w, int wlen, int nfft, long long first,
                         int delay, size_t nframes, cf32 *time, hipStream_t st);
size_t spgram_accum_scratch_floats(int nfft, size_t nframes);
// `part`: spgram_accum_scratch_floats(nfft, nframes) floats of scratch
int launch_spgram_accum(const cf32 *freq, int nfft, size_t nframes, float alpha, float gamma, bool first_ever,
                        float *psd, float *part, hipStream_t st);
// fused taper -> FFT -> |X|^2 -> weighted accumulation (nfft in {256,512,1024,2048,4096});
// part: spgram_fused_scratch_floats(nfft, nframes) floats; twn = the plan's W_nfft table
bool spgram_fused_supported(int nfft);
size_t spgram_fused_scratch_floats(int nfft, size_t nframes);
template <class T>
int launch_spgram_fused(int nfft, const T *win, const T *x, size_t x_len, const float *w, int wlen, long long first,
                        int delay, size_t nframes, float alpha, float gamma, bool first_ever, const cf32 *twn,
                        float *psd, float *part, hipStream_t st);
int launch_spgram_psd(const float *psd, int nfft, float scale, bool in_db, float *out, hipStream_t st);
// the launch arithmetic, shared by the launchers, SpgramObj::run_frames and yagi_hip_plan_spgram:
//   spgram_launch_frames  transforms per launch of run_frames (the cut of a longer call)
//   spgram_fused_slab     consecutive transforms per workgroup of a fused launch of nframes (a multiple of the group)
//   spgram_fused_rows     workgroups, partial rows and the 32-to-1 fold of that launch
//   spgram_frames_grid    workgroups of the unfused frame builder (grid-stride beyond the cap)
struct SpgramFusedRows {
    unsigned group, slab, workgroups, rows, fold_rows;           // fold_rows = 0 unless folded
    bool folded;
};
size_t spgram_launch_frames(int nfft);
unsigned spgram_fused_slab(int nfft, size_t nframes);
SpgramFusedRows spgram_fused_rows(int nfft, size_t nframes);
unsigned spgram_frames_grid(int nfft, size_t nframes);
int spgram_accum_slab();

// ---- chan_kernels.hip ----------------------------------------------------------------------
// firpfbch analyzer: hist = the (p-1)*M samples preceding x[0] (oldest first).
// hist_next (optional): the object's other history buffer; when the kernel taken can write the history after the
// block itself, *hist_written is set and the caller skips its own update.
int launch_firpfbch(const cf32 *hist, const cf32 *x, const float *h, int M, int p,
                    const cf32 *twM, cf32 *y, size_t nframes, hipStream_t st, cf32 *hist_next = nullptr,
                    bool *hist_written = nullptr);
// firpfbch synthesizer: x = nframes frames of M channel samples, hist = the (p-1)*M channel samples before them;
// y[f*M + i] = sum_n h[i + n*M] * IDFT_M(frame f-n)[i]
int launch_firpfbch_syn(const cf32 *hist, const cf32 *x, const float *h, int M, int p,
                        const cf32 *twM, cf32 *y, size_t nframes, hipStream_t st);
// firpfbch2 synthesizer: x = nsteps steps of M channel samples, hist = the (4m-1)*M channel samples before them,
// step0 = index of the first step (parity selects the half the outputs come from); y = nsteps*M/2 samples
int launch_firpfbch2_syn(const cf32 *hist, int hist_len, const cf32 *x, const float *h, int M, int m,
                         const cf32 *twM, uint64_t step0, cf32 *y, size_t nsteps, hipStream_t st);
// firpfbch2 analyzer: hist = the 2*m*M - M/2 ... samples preceding x[0]; step0 = index of the
// first step (parity selects the half rotation).  rank/nranks select sub-bands k = rank + nranks*q.
int launch_firpfbch2(const cf32 *hist, int hist_len, const cf32 *x, const float *h, int M, int m,
                     const cf32 *twM, uint64_t step0, int rank, int nranks, cf32 *y, size_t nsteps,
                     hipStream_t st, cf32 *hist_next = nullptr, bool *hist_written = nullptr);
int launch_firpfbch2_assemble(const cf32 *gathered, size_t nsteps, int M, int nranks, cf32 *y,
                              hipStream_t st);

// ---- chanr_kernels.hip ---------------------------------------------------------------------
// firpfbchr (M channels, P inputs per analyzer step, prototype h[0 : 2Mm]); closed forms at the top of the file.
// YAGI_OK when the general kernels can hold (M, m) in LDS, YAGI_ERR_CONFIG otherwise (host arithmetic only).
int firpfbchr_check_shape(int M, int P, int m);
bool firpfbchr_col_served(int M, int P, int m);
// analyzer: hist = the 2Mm - P samples before x[0], step0 = index of the first step in the stream (its rotation);
// y = nsteps*M.  choice: 1 general, 2 column (an error where firpfbchr_col_served() is false); *ran = the kernel taken.
int launch_firpfbchr(const cf32 *hist, int hist_len, const cf32 *x, const float *h, int M, int P, int m,
                     const cf32 *twM, uint64_t step0, cf32 *y, size_t nsteps, hipStream_t st, int choice, int *ran);
// synthesizer, first launch: v[s][b] = sum_k x[s][k] e^{+j 2 pi k b / M} for the nsteps steps of the call
int launch_firpfbchr_syn_transform(const cf32 *x, int M, const cf32 *twM, cf32 *v, size_t nsteps, hipStream_t st);
// second launch: y[t] = (P/M) sum_r h[t mod P + rP] v[floor(t/P) - r][(step0 P + t) mod M], t < nsteps*P; vhist = the
// hist_rows = ceil(2Mm/P) - 1 transformed steps before the call
int launch_firpfbchr_syn_combine(const cf32 *vhist, int hist_rows, const cf32 *v, const float *h, int M, int P, int m,
                                 uint64_t step0, cf32 *y, size_t nsteps, hipStream_t st);

// ---- iir_kernels.hip -----------------------------------------------------------------------
// IirFilter (src/filter/iir/iirfilt.rs) as a chunked state scan.  The block is cut into chunks of T samples, one per
// lane, 64 chunks per workgroup.  The state of S entries after a chunk is A^T s0 + z, z = the chunk's final state from
// zero; the f64 power tables P_k = A^(T 2^k) (host-computed, [levels][S][S]) carry states across chunks.
//   phase A: every chunk from zero state (f32) -> z[c]; inclusive in-workgroup scan (f64) -> agg[g]
//   phase B: one workgroup scans agg[0 .. G-1) seeded with the carried state -> init[g] (state before workgroup g)
//   phase C: every chunk from its exact initial state (f64 scan rounded once to f32) -> y = scale * y; the chunk that
//            holds the last sample writes the carried state
constexpr int kIirTfMaxN = 33;    // transfer-function form: n = max(na, nb) <= 33 (S = n - 1 <= 32)
constexpr int kIirSosGroup = 16;  // second-order sections per kernel pass (longer cascades run as groups)
constexpr int kIirLevels = 40;    // power-table levels kept per group
constexpr int kIirWg = 64;        // chunks (lanes) per workgroup

template <class K>
struct IirParams {
    typename K::C b[3 * kIirSosGroup];    // TF: b[0..n), a[0..n) normalised, zero-padded to n; SOS: [sec][3]
    typename K::C a[3 * kIirSosGroup];
    typename K::C scale;
    int sos;            // 0: transfer function, 1: second-order sections
    int n;              // TF: n = S + 1; SOS: sections in this group
    int S;              // state entries
    int T;              // chunk length (power of two)
    uint32_t head0;     // TF: physical head of the reference's VecDeque before the block's first rotate
};
// f64 element types of the combine: the state (real for rrrf, complex otherwise) and the matrix (complex for cccf)
struct dcplx { double re, im; };
template <class K> struct IirF64 { using V = dcplx; using M = double; };
template <> struct IirF64<RRRF> { using V = double; using M = double; };
template <> struct IirF64<CCCF> { using V = dcplx; using M = dcplx; };

// scratch: z [ceil(n/T)][S] of T, agg and init [G][S] of IirF64<K>::V; state: S samples of T, read and rewritten
template <class K>
int launch_iir(const IirParams<K> &p, const typename K::T *x, size_t n, typename K::T *y, typename K::T *state,
               typename K::T *z, void *agg, void *init, const void *ptab, int levels, hipStream_t st);

// The mapped forms run the same scan over a virtual stream of n filter steps: an input map in front
// of phases A and C, an output map behind phase C, phase B unchanged.
// IirDecim / IirInterp: the sparse side holds sample i at step i M; the other steps read +0.0 (sparse_in) or are not
// stored (sparse_out).  The dense side is the plain x[gi] / y[gi].
constexpr uint32_t kIirMaxRate = 65536;
template <class K>
struct IirRateIo {
    const typename K::T *x;
    typename K::T *y;
    uint32_t M;
    int sparse_in, sparse_out;
};
template <class K>
int launch_iir_rate(const IirParams<K> &p, const IirRateIo<K> &io, size_t n, typename K::T *state, typename K::T *z,
                    void *agg, void *init, const void *ptab, int levels, hipStream_t st);
// IirHilbertFilter over one crcf filter; k = (phase + gi) & 3.  Plain = cf32 x[gi] / y[gi] (cascade passes in between).
enum { kHilbInPlain = 0, kHilbInReal = 1, kHilbInCplx = 2, kHilbInEven = 3 };
enum { kHilbOutPlain = 0, kHilbOutRot2 = 1, kHilbOutProj = 2, kHilbOutEven2 = 3, kHilbOutProj2 = 4 };
struct IirHilbIo {
    const void *x;      // float (InReal) or cf32
    void *y;            // float (OutProj, OutProj2) or cf32
    uint32_t phase;
    int imode, omode;
};
int launch_iir_hilb(const IirParams<CRCF> &p, const IirHilbIo &io, size_t n, cf32 *state, cf32 *z, void *agg, void *init,
                    const void *ptab, int levels, hipStream_t st);

// ---- osc_kernels.hip -----------------------------------------------------------------------
// Osc::mix_block_up / mix_block_down (src/nco/osc.rs) on device buffers: y[j] = x[j] * (cos + i sin)(theta0 + j dtheta),
// conjugated for `down`; vco selects the table (host.cpp: osc_device_table, 1024 float2 for the NCO, 1024 float4 for
// the VCO).  x == y (in place) is allowed; x and y need only their element alignment (yagi_hip.h), 16-byte alignment
// of both gives 16-byte accesses.
constexpr int kOscWg = 512;        // threads per workgroup
constexpr int kOscUnroll = 4;      // loads in flight per lane
constexpr int kOscWgPerCu = 2;     // persistent grid: 2 workgroups per CU
int launch_osc_mix(int vco, bool down, const void *tab, uint32_t theta0, uint32_t dtheta, const cf32 *x, cf32 *y,
                   size_t n, hipStream_t st);

// ---- ddc_kernels.hip -----------------------------------------------------------------------
// Ddc: launch_fir_block (M >= 2) over x mixed down with theta0 + (u32)j dtheta at sample j, in one launch; win holds
// mixed samples and win_next receives the mixed tail.  Duc: launch_firpfb_all with output j mixed up with
// theta0 + (u32)j dtheta at its store.  K is CRCF or CCCF; vco / tab as for launch_osc_mix.  The *_serves predicates say
// whether a fused kernel exists for the shape (same kernel choice as the plain launcher, span + table within 64 KiB
// of LDS); the launchers fail where it does not, and the caller runs launch_osc_mix and the plain launcher instead.
// Every output word equals that composition's.  x and y must not overlap and need 8-byte alignment only.
template <class K>
bool ddc_fused_serves(int L, int M, size_t ny, int vco);
template <class K>
int launch_ddc_block(const cf32 *win, const cf32 *x, const typename K::C *taps, int L, int M, typename K::C scale,
                     cf32 *y, size_t ny, hipStream_t st, cf32 *win_next, int vco, const void *tab, uint32_t theta0,
                     uint32_t dtheta);
template <class K>
bool duc_fused_serves(int nf, int Ls, int vco);
template <class K>
int launch_duc_all(const cf32 *win, const cf32 *x, const typename K::C *hb, int nf, int Ls, typename K::C scale,
                   cf32 *y, size_t n, hipStream_t st, cf32 *win_next, int vco, const void *tab, uint32_t theta0,
                   uint32_t dtheta);

// ---- firhilb_kernels.hip -------------------------------------------------------------------
// FirHilbertFilter (src/filter/fir/firhilb.rs) block calls on device buffers, n units (r2c: n real -> n complex; c2r:
// n complex -> 2n real; decim: 2n real -> n complex; interp: n complex -> 2n real).  win: the four windows w0..w3 of
// 2m floats, oldest first; win_next receives the windows the call leaves; toggle is the toggle at the call.  x and y
// must not overlap; they need only their element alignment (yagi_hip.h).  m <= kFirhilbFastM takes the LDS-staged sliding form.
enum { FIRHILB_R2C = 0, FIRHILB_C2R = 1, FIRHILB_DECIM = 2, FIRHILB_INTERP = 3 };
constexpr int kFirhilbWg = 256;                        // threads per workgroup
constexpr int kFirhilbR = 8;                           // consecutive pairs per lane
constexpr int kFirhilbTile = kFirhilbWg * kFirhilbR;   // pairs per workgroup
constexpr int kFirhilbFastM = 512;
int launch_firhilb(int mode, int m, const float *hq, const float *win, float *win_next, int toggle, const float *x,
                   size_t n, float *y, hipStream_t st);

// ---- fdelay_kernels.hip --------------------------------------------------------------------
// Fdelay (src/filter/fdelay.rs) block calls on device buffers: n samples in, n out.  state = [the last nmax samples of
// the input X, oldest first][the last Ls values V pushed into the bank][one float: the delay in force]
// (fdelay_state_bytes); state_next receives the state the call leaves and must not alias state.  H = the bank's rows
// [npfb][Ls] against the window oldest first.  delay == nullptr: the fixed lag D and branch f for the whole call
// (delay0 = the delay they came from, stored for the host); else one delay per sample, clamped into [0, nmax] (what is
// not >= 0 counts as 0).  x and y must not overlap.
constexpr int kFdWg = 256;                             // threads per workgroup
constexpr int kFdTrackTile = 1024;                     // outputs per workgroup of the track form
constexpr size_t kFdLdsBudget = 64 * 1024;             // the track form stages its nmax-deep input halo in LDS below this
constexpr int kFdMaxLs = 4096;                         // branch length the LDS tiles are sized for
struct FdelayDims { int nmax, Ls, npfb; };
template <class T> size_t fdelay_state_bytes(int nmax, int Ls);
template <class K>
int launch_fdelay(const FdelayDims &dm, const typename K::C *H, typename K::C scale, const typename K::T *state,
                  typename K::T *state_next, int D, int f, float delay0, const float *delay, const typename K::T *x,
                  size_t n, typename K::T *y, hipStream_t st);

// ---- modem_kernels.hip ---------------------------------------------------------------------
// Modem (src/modem/modem.rs): block modulation and hard / soft demodulation on device buffers, and the same arithmetic
// on the host (this file is the one built with contraction off).  map = M points, nbr = M * p neighbour indices
// (p = 0: none).  state / state_next: the object's ModemState on the device; a demodulating call and a DPSK modulation
// read one and write the other (the caller flips), any other modulation leaves both untouched.
enum { MODEM_PSK = 0, MODEM_DPSK, MODEM_ASK, MODEM_QAM, MODEM_BPSK, MODEM_QPSK, MODEM_OOK, MODEM_ARB };
constexpr int kModemWg = 256;                          // threads per workgroup
constexpr int kModemModTile = 4096;                    // symbols per workgroup of the modulating kernels
constexpr int kModemDemodTile = 2048;                  // samples per workgroup of the demodulating kernels
struct ModemParams {
    int kind, bps, M, p;
    float ref[8];                                      // reference[] of the linear-array schemes
    float d_phi, gamma;                                // PSK / DPSK half spacing offset; Arb's soft-bit gain
};
struct ModemState {
    cf32 r, x_hat;                                     // the last demodulated sample and its decision
    float phi;                                         // DPSK demodulator: the last sample's phase
    unsigned k;                                        // DPSK modulator: the running index (yagi_hip.h)
};
int modem_design(int kind, int bps, const cf32 *table, ModemParams &P, std::vector<cf32> &map, std::vector<uint8_t> &nbr);
unsigned modem_host_demod(const ModemParams &P, const cf32 *map, const uint8_t *nbr, cf32 x, ModemState &s, uint8_t *soft);
unsigned modem_host_modulate_dpsk(const ModemParams &P, unsigned sym, unsigned k);
size_t modem_num_partials(size_t n);                   // words of `partials` a modulating call of n symbols needs
// soft != nullptr: the soft form (n * bps bytes); xhat may be null.  x, sym, xhat, soft must not overlap.
int launch_modem_demod(const ModemParams &P, const cf32 *map, const uint8_t *nbr, const ModemState *state,
                       ModemState *state_next, const cf32 *x, size_t n, uint8_t *sym, cf32 *xhat, uint8_t *soft,
                       hipStream_t st);
// *flag is left non-zero when a symbol >= M was found; then y and state_next are not written.
int launch_modem_modulate(const ModemParams &P, const cf32 *map, const ModemState *state, ModemState *state_next,
                          const uint8_t *sym, size_t n, cf32 *y, unsigned *partials, int *flag, hipStream_t st);

// ---- ordfilt_kernels.hip -------------------------------------------------------------------
// OrdFilt (src/filter/ordfilt.rs) block calls on device buffers: nb samples in, nb out, y[i] = the sample of rank k
// (0-based, ascending, ties by age) among the n samples that end at x[i].  hist = the n samples before x[0], oldest
// first (the reference's Window); hist_next receives the window the call leaves and must not alias hist.  x and y must
// not overlap.  The order is ordfilt_key's (yagi_hip.h: partial_cmp where that is defined, NaN by sign beyond +-inf).
constexpr int kOrdfiltWg = 256;                        // threads per workgroup
constexpr int kOrdfiltTile = YAGI_ORDFILT_TILE;        // outputs per workgroup
constexpr int kOrdfiltNmax = YAGI_ORDFILT_NMAX;        // longest window the LDS tile is sized for
// LDS of the kernel: keys of a tile and its halo, the tile's outputs, one "-0.0" bit per staged sample
constexpr size_t kOrdfiltLdsBytes = (size_t)(kOrdfiltTile + kOrdfiltNmax - 1) * 4 + (size_t)kOrdfiltTile * 4 +
                                    (size_t)(kOrdfiltTile + kOrdfiltNmax - 1) / 8;
static_assert(kOrdfiltLdsBytes <= 64 * 1024, "the tile must fit a workgroup's LDS");
// The register-resident form exists for 2 <= n <= kOrdfiltRegNmax; form AUTO takes it up to kOrdfiltRegCrossover.
enum { ORDFILT_AUTO = 0, ORDFILT_LDS = 1, ORDFILT_REG = 2 };
constexpr int kOrdfiltRegNmax = YAGI_ORDFILT_REG_NMAX;
constexpr int kOrdfiltRegCrossover = 9;                // DESIGN.md section 4, profiles/r10_kbench_ordfilt.txt
static_assert(kOrdfiltRegCrossover <= kOrdfiltRegNmax, "AUTO may only pick a form that exists");
// LDS of the register form: the tile's rows of 16 samples padded to 20 words, and one row more for the last halo
constexpr size_t kOrdfiltRegLdsBytes = (size_t)(kOrdfiltWg + 1) * (kOrdfiltTile / kOrdfiltWg + 4) * 4;
int launch_ordfilt(int n, int k, int form, const float *hist, float *hist_next, const float *x, size_t nb, float *y,
                   hipStream_t st);
// element k of the window (n samples, oldest first) after a stable sort under the same order; tmp is scratch
float ordfilt_host_select(const float *win, int n, int k, std::vector<std::pair<unsigned, unsigned>> &tmp);

// ---- sequence_kernels.hip ------------------------------------------------------------------
// MSequence (src/sequence/msequence.rs): advance() is linear over GF(2) on the 32-bit state word; a matrix is 32 column
// words.  pow = T^(2^b), b = 0 .. kMseqPowers-1; stride = for bps = 1 .. 8 the kMseqStrides lane-stride matrices
// T^(kMseqRun * bps * 2^b) of the block kernel.  Both tables are built once per object and uploaded as they are.
constexpr int kMseqWg = 256;                           // threads per workgroup
constexpr int kMseqTile = YAGI_MSEQUENCE_TILE;         // symbols per workgroup
constexpr int kMseqRun = kMseqTile / kMseqWg;          // consecutive symbols per lane
constexpr int kMseqPowers = 64;
constexpr int kMseqStrides = 6;                        // one per bit of the lane number within a wave
constexpr size_t kMseqPowWords = (size_t)kMseqPowers * 32, kMseqStrideWords = (size_t)8 * kMseqStrides * 32;
constexpr size_t kMseqLdsBytes = (size_t)kMseqTile;    // the tile's bytes
void msequence_tables(unsigned g, unsigned nmask, unsigned *pow, unsigned *stride);
unsigned msequence_skip(const unsigned *pow, unsigned s, uint64_t k);     // the state k steps after s, O(log k)
// y[i] = generate_symbol(bps) for i < n from the state s0 (bps = 1: one bit per byte); the caller advances its state
int launch_msequence_gen(const unsigned *pow, const unsigned *stride, unsigned s0, unsigned g, unsigned nmask, int m,
                         int bps, size_t n, uint8_t *y, hipStream_t st);

// BSequence (src/sequence/bsequence.rs) push_correlate_block on device buffers: for each of n symbols, push its bps
// bits (MSB first) into the window cur (W words, word 0 oldest and masked by qmask), then rxy[i] = ref.correlate(q).
// next receives the window the call leaves and must not alias cur.  rxy may be null (the call then only pushes).
constexpr int kBseqWg = 256;                           // threads per workgroup
constexpr int kBseqTile = YAGI_BSEQUENCE_TILE;         // outputs per workgroup
constexpr int kBseqNmax = YAGI_BSEQUENCE_NMAX;         // longest window, in bits
// LDS of the kernel: the packed words a tile's windows span (8 bits per symbol at most, the window, one word of slack
// at either end) and the symbol bytes under them (one bit per symbol at least, 16 bytes of alignment slack)
constexpr int kBseqPackedWords = kBseqTile * 8 / 32 + kBseqNmax / 32 + 2;
constexpr int kBseqSymBytes = kBseqTile + (kBseqNmax / 32 + 2) * 32 + 16;
constexpr size_t kBseqLdsBytes = (size_t)kBseqPackedWords * 4 + (size_t)kBseqSymBytes;
static_assert(kBseqLdsBytes <= 64 * 1024 && kBseqNmax % 32 == 0 && kBseqNmax / 32 <= kBseqWg, "the tile must fit a workgroup's LDS");
int launch_bsequence_corr(const unsigned *cur, unsigned *next, const unsigned *ref, int W, unsigned qmask,
                          int ref_bits_msb, const uint8_t *sym, size_t n, int bps, int *rxy, hipStream_t st);

// ---- autocorr_kernels.hip ------------------------------------------------------------------
// Autocorr (yagi_hip.h) block calls on device buffers: nb samples in; rxx[i] and, where energy is not null, energy[i]
// after each (W = window_size, d = delay).  hist = the W + d samples before x[0], oldest first (the kernel reads the
// newest W - 1 + d; the oldest is there for an execute() right after the call); hist_next receives the history the call
// leaves and must not alias hist.  x, rxx and energy must not overlap.
constexpr int kAutocorrWg = 256;                       // threads per workgroup
constexpr int kAutocorrTile = YAGI_AUTOCORR_TILE;      // outputs per workgroup
constexpr int kAutocorrWmax = YAGI_AUTOCORR_WMAX;      // longest window the LDS tile is sized for
constexpr int kAutocorrDmax = YAGI_AUTOCORR_DMAX;      // longest delay (the carried history is W + d samples)
constexpr int kAutocorrR = kAutocorrTile / kAutocorrWg;   // consecutive outputs per lane
// LDS of the kernel: per staged sample (Tile + Wmax of them, in rows of R padded by 16 bytes) its term of rxx, two floats
// for cccf, one for rrrf, and with energy its term of that: for cccf in rows of its own, for rrrf beside the first
constexpr size_t autocorr_lds_bytes(size_t elem_bytes, bool with_energy) {
    const size_t rows = (size_t)(kAutocorrTile + kAutocorrWmax) / kAutocorrR, r = (size_t)kAutocorrR;
    return elem_bytes == 8 ? rows * (r * 8 + 16) + (with_energy ? rows * (r * 4 + 16) : 0)
                           : rows * (r * (with_energy ? 8 : 4) + 16);
}
static_assert(autocorr_lds_bytes(8, true) <= 64 * 1024, "the tile must fit a workgroup's LDS");
template <class T>
int launch_autocorr(int W, int d, const T *hist, T *hist_next, const T *x, size_t nb, T *rxx, float *energy,
                    hipStream_t st);
// rxx and energy of the window as it stands: h = the last W + d samples, oldest first; the kernel's arithmetic
template <class T>
void autocorr_host(const T *h, int W, int d, T *rxx, float *energy);

// ---- burstdet_kernels.hip ------------------------------------------------------------------
// BurstDetector (yagi_hip.h) block calls on device buffers: nb samples in, the events they close out.  hist / hist_next
// as for launch_autocorr.  scratch holds burstdet_scratch_bytes(nb): the tile table, then the segment pool.  state is the
// object's device state; its pool_used is zero between calls.  events has room for cap; status receives {count, overflow}.
constexpr int kBurstSegmax = YAGI_BURSTDET_SEGMAX;     // segments a call may hold beyond one per tile
struct BurstSeg {                                      // a run of hits inside a tile; offsets from the tile's first sample
    unsigned start, length, peak;
    float ratio, energy, re, im;                       // r, energy and rxx at the peak
    unsigned pad;
};
struct BurstState {
    unsigned long long position, pool_used;            // samples since reset(); segments the running call has taken
    unsigned has_pending, pad;
    yagi_burst_event pending;                          // the run that ends on the last sample seen
};
static_assert(sizeof(BurstSeg) == 32 && sizeof(BurstState) == 64 && sizeof(yagi_burst_event) == 40, "device layouts");
constexpr size_t burstdet_scratch_bytes(size_t nb) {
    const size_t tiles = (nb + kAutocorrTile - 1) / kAutocorrTile;
    return tiles * 16 + (tiles + (size_t)kBurstSegmax) * sizeof(BurstSeg);
}
template <class T>
int launch_burstdet(int W, int d, float thr2, float floor_, unsigned long long min_length, const T *hist, T *hist_next,
                    const T *x, size_t nb, void *scratch, BurstState *state, yagi_burst_event *events, size_t cap,
                    unsigned *status, hipStream_t st);
// the same call on the host, sample by sample over autocorr_host: win = the last W + d samples (updated), state as above
template <class T>
int burstdet_host(int W, int d, float thr2, float floor_, unsigned long long min_length, T *win, BurstState *state,
                  const T *x, size_t n, yagi_burst_event *events, size_t cap, size_t *count, int *overflow);

// ---- pdet_kernels.hip ----------------------------------------------------------------------
// PreambleDetector (yagi_hip.h) block calls on device buffers.  tmpl holds the K templates as rows of pdet_pitch(L)
// elements (the taps behind L are never added; they are there so that a four-tap read stays inside the row).  hist =
// the L samples before x[0], oldest first; hist_next receives the history the call leaves and must not alias hist.
// launch_pdet: nb samples in, the events they close out; scratch holds pdet_scratch_bytes(nb): the tile table, then the
// segment pool (BurstSeg, the hypothesis in its spare word); state's pool_used is zero between calls; events has room
// for cap; status receives {count, overflow}.  launch_pdet_correlate: rxy[k nb + i] and energy[i] (or null) of sample i;
// state's counter advances by nb and its pending run is dropped.
constexpr int kPdetWg = 256;                           // threads per workgroup
constexpr int kPdetTile = YAGI_PDET_TILE;              // outputs per workgroup
constexpr int kPdetLmax = YAGI_PDET_LMAX;              // longest preamble the LDS tile is sized for
constexpr int kPdetKmax = YAGI_PDET_KMAX;
constexpr int kPdetSegmax = YAGI_PDET_SEGMAX;          // segments a call may hold beyond one per tile
constexpr int kPdetR = kPdetTile / kPdetWg;            // consecutive outputs per lane
constexpr size_t pdet_pitch(size_t L) { return (L + 3) / 4 * 4; }
// LDS of the kernels: per staged sample (Tile + Lmax of them, in rows of R padded by 16 bytes) the sample, two floats,
// and in rows of its own its energy term
constexpr size_t pdet_lds_bytes() {
    const size_t rows = (size_t)(kPdetTile + kPdetLmax) / kPdetR, r = (size_t)kPdetR;
    return rows * (r * 8 + 16) + rows * (r * 4 + 16);
}
static_assert(pdet_lds_bytes() <= 64 * 1024, "the tile must fit a workgroup's LDS");
struct PdetState {
    unsigned long long position, pool_used;            // samples since reset(); segments the running call has taken
    unsigned has_pending, pad;
    yagi_preamble_event pending;                       // the run that ends on the last sample seen
};
static_assert(sizeof(PdetState) == 72 && sizeof(yagi_preamble_event) == 48, "device layouts");
constexpr size_t pdet_scratch_bytes(size_t nb) {
    const size_t tiles = (nb + kPdetTile - 1) / kPdetTile;
    return tiles * 16 + (tiles + (size_t)kPdetSegmax) * sizeof(BurstSeg);
}
int launch_pdet(int L, int K, const cf32 *tmpl, float ep, float thr2, float floor_, unsigned long long min_length,
                const cf32 *hist, cf32 *hist_next, const cf32 *x, size_t nb, void *scratch, PdetState *state,
                yagi_preamble_event *events, size_t cap, unsigned *status, hipStream_t st);
int launch_pdet_correlate(int L, int K, const cf32 *tmpl, const cf32 *hist, cf32 *hist_next, const cf32 *x, size_t nb,
                          cf32 *rxy, float *energy, PdetState *state, hipStream_t st);
// v_k[i] = conj(p[i]) e^{-j dphi_k i}, evaluated in f64 and rounded once per component: out[k L + i]
void pdet_templates(const cf32 *p, size_t L, const float *dphi, size_t K, cf32 *out);
// ep = the f32 sum over i, from +0.0, of fl(fl(p.re^2) + fl(p.im^2))
float pdet_preamble_energy(const cf32 *p, size_t L);
// rxy_k (k = 0 .. K-1) and the energy of the window h[0 .. L) against tmpl[k L + i]
void pdet_host_sums(const cf32 *h, int L, int K, const cf32 *tmpl, cf32 *rxy, float *energy);
// launch_pdet on the host, sample by sample: win = the last L samples (updated), tmpl = K rows of L, state as above
int pdet_host(int L, int K, const cf32 *tmpl, float ep, float thr2, float floor_, unsigned long long min_length,
              cf32 *win, PdetState *state, const cf32 *x, size_t n, yagi_preamble_event *events, size_t cap,
              size_t *count, int *overflow);

// ---- symsync_kernels.hip -------------------------------------------------------------------
// SymSync (yagi_hip.h): C independent Symsync<Complex32> loops of one design, one lane per channel.  taps holds both
// banks interleaved: entry [b Ls + j] = (H[b][j], D[b][j]), rows against the window oldest first.  hist is the last Ls
// rows of input, [Ls][C], oldest first; state one SymsyncChan per channel.  Both are updated in place (a workgroup
// touches its own channels only).  status receives ny[C], then stalled[C].
constexpr int kSymsyncWg = 64;                         // channels per workgroup: one wave
constexpr int kSymsyncAhead = 16;                      // input rows per chunk: requested one chunk ahead, staged in LDS
constexpr size_t kSymsyncLdsMax = 160 * 1024;          // ring, tap table and stage where all fit; else the table stays global
struct SymsyncChan {
    float tau, tau_decim, bf, rate, del, q, q_hat, v0, v1, v2;
    unsigned since, stalled;                           // samples since reset (saturates at Ls): the matched filter reads
    unsigned long long b, decim;                       // +0.0 for older slots; b and decim_counter in 64 bits, as usize
};
static_assert(sizeof(SymsyncChan) == 64, "device layout");
struct SymsyncLoop {
    float b0, b1, b2, a1, a2, rate_adj;                // the loop filter, normalised by a0, and rate_adjustment
    float kf, knorm, npfbf;                            // k as f32, fl(fl(kf kf) + fl(0 0)), npfb as f32
    unsigned npfb, Ls, locked;
    unsigned long long k_out;
};
constexpr size_t symsync_ring_bytes(size_t Ls) { return Ls * kSymsyncWg * sizeof(cf32); }
constexpr size_t symsync_table_bytes(size_t npfb, size_t Ls) { return npfb * Ls * 2 * sizeof(float); }
constexpr size_t symsync_stage_bytes() { return (size_t)kSymsyncAhead * kSymsyncWg * sizeof(cf32); }
// symsync.rs:37-79: both banks from the prototype, interleaved as above; YAGI_ERR_CONFIG as yagi_hip.h says
int symsync_design(size_t k, size_t npfb, const float *h, size_t h_len, std::vector<float> &taps, size_t *Ls);
// set_lf_bw (:196-213) in f32
int symsync_set_bw(float bw, SymsyncLoop *p);
// reset() of one channel (:160-172); the history is not touched
void symsync_reset_chan(SymsyncChan *s, size_t k, size_t k_out);
int launch_symsync(const SymsyncLoop &p, const float *taps, SymsyncChan *state, cf32 *hist, size_t C, const cf32 *x,
                   size_t x_pitch, size_t n, cf32 *y, size_t y_pitch, size_t ycap, unsigned *status, hipStream_t st);
// the same on the host, channel after channel; ny and stalled have C entries each
void symsync_host(const SymsyncLoop &p, const float *taps, SymsyncChan *state, cf32 *hist, size_t C, const cf32 *x,
                  size_t x_pitch, size_t n, cf32 *y, size_t y_pitch, size_t ycap, unsigned *ny, unsigned *stalled);

// ---- eqlms_kernels.hip ---------------------------------------------------------------------
// EqLms (yagi_hip.h): C independent Eqlms<Complex32> loops of one design, one lane per channel.  w = the weights w0,
// [h_len][C]; hist = the window, [h_len][C], oldest first; state one EqlmsChan per channel.  All three are updated in
// place (a workgroup touches its own channels only).  call = a YAGI_EQLMS_* mode for decim_block (n input rows, a
// multiple of k, n / k rows of y; d = n / k rows of known symbols for TRAIN; table = M points for DECISION) or kEqlmsExec
// for execute_block (n rows in, n rows out).
constexpr int kEqlmsWg = 64;                           // channels per workgroup: one wave
constexpr int kEqlmsAhead = 16;                        // input rows per chunk: requested one chunk ahead, staged in LDS
constexpr int kEqlmsAheadD = 8;                        // the same for TRAIN's rows of known symbols
constexpr int kEqlmsExec = 4;                          // execute_block, after the four YAGI_EQLMS_* modes
struct EqlmsChan {
    float x2_sum;                                      // the running f32 sum, never recomputed from the window
    unsigned pad;
    unsigned long long count;                          // pushes since reset, as usize
};
static_assert(sizeof(EqlmsChan) == 16, "device layout");
constexpr size_t eqlms_taps_bytes(size_t h_len) { return h_len * kEqlmsWg * sizeof(cf32); }
constexpr size_t eqlms_stage_bytes() { return (size_t)kEqlmsAhead * kEqlmsWg * sizeof(cf32); }
constexpr size_t eqlms_dstage_bytes() { return (size_t)kEqlmsAheadD * kEqlmsWg * sizeof(cf32); }
// ring, weights, both stages and the DECISION table: 145408 bytes at h_len = 128, under the 160 KiB of a CU
constexpr size_t eqlms_lds_bytes(size_t h_len) {
    return 2 * eqlms_taps_bytes(h_len) + eqlms_stage_bytes() + eqlms_dstage_bytes() + YAGI_EQLMS_TABLE_MAX * sizeof(cf32);
}
static_assert(eqlms_lds_bytes(YAGI_EQLMS_LEN_MAX) <= 160 * 1024, "the LDS of a CU");
int launch_eqlms(int call, size_t h_len, float mu, cf32 *w, cf32 *hist, EqlmsChan *state, size_t C, size_t k, const cf32 *x,
                 size_t x_pitch, size_t n, const cf32 *d, size_t d_pitch, const cf32 *table, size_t M, cf32 *y,
                 size_t y_pitch, hipStream_t st);
// the same on the host, channel after channel
void eqlms_host(int call, size_t h_len, float mu, cf32 *w, cf32 *hist, EqlmsChan *state, size_t C, size_t k, const cf32 *x,
                size_t x_pitch, size_t n, const cf32 *d, size_t d_pitch, const cf32 *table, size_t M, cf32 *y,
                size_t y_pitch);

// ---- eqrls_kernels.hip ---------------------------------------------------------------------
// EqRls (yagi_hip.h): C independent Eqrls<Complex32> loops of one design.  A group of L lanes (a power of two, 1 .. 64)
// runs one channel's step, so a workgroup of one wave holds 64 / L channels.  P = the recursion matrix, [p p][C], row
// major; w0 and w1 = the two weight vectors, [p][C]; hist = the window, [p][C], oldest first.  All four are updated in
// place (a workgroup touches its own channels only); w1 is written only by a call that runs at least one update.
// mode = YAGI_EQRLS_NONE / TRAIN / DECISION; n input rows, a multiple of k, n / k rows of y; d = n / k rows of known
// symbols for TRAIN; table = M points for DECISION.
constexpr int kEqrlsWg = 64;                           // lanes per workgroup: one wave
constexpr int kEqrlsAhead = 8;                         // input rows per chunk: requested one chunk ahead, staged in LDS
constexpr size_t kEqrlsLdsMax = 160 * 1024;            // the LDS of a CU
// the row pitch of P in LDS: odd, so that the L lanes of a group that read one row each (the numerators of g) fall on
// different banks, as the lanes that read one column each do by the [element][channel-in-wave] layout alone
constexpr size_t eqrls_pitch(size_t p) { return p | 1; }
// per channel two matrices (P0 and the buffer P1 is formed in), the window, w0, xp0, g and two rows of gxl; per
// workgroup the staged input rows of its 64 / L channels and the DECISION table
constexpr size_t eqrls_chan_elems(size_t p) { return 2 * p * eqrls_pitch(p) + 6 * p; }
constexpr size_t eqrls_lds_bytes(size_t p, size_t L) {
    return ((size_t)(kEqrlsWg / L) * (eqrls_chan_elems(p) + kEqrlsAhead) + YAGI_EQLMS_TABLE_MAX) * sizeof(cf32);
}
static_assert(eqrls_lds_bytes(YAGI_EQRLS_LEN_MAX, 8) <= kEqrlsLdsMax, "p = 32 runs at L = 8");
// The admissible L for p: a power of two whose 64 / L channels fit in LDS, and no more lanes than twice the columns they
// share (L / 2 < p).  Returned as a mask, bit b = (L = 2^b).
constexpr unsigned eqrls_admissible(size_t p) {
    unsigned m = 0;
    for (unsigned b = 0; b <= 6; ++b) {
        const size_t L = (size_t)1 << b;
        if (eqrls_lds_bytes(p, L) <= kEqrlsLdsMax && (L == 1 || L / 2 < p)) m |= 1u << b;
    }
    return m;
}
// The planner's choice: the largest admissible L, whatever the channel count.  The p^3 term of a step spreads over the L
// lanes of a group and a wave of fewer channels needs less LDS, so more waves fit a CU; measured on the MI355X at p = 4,
// 8, 16 and 32 and C = 64 .. 262144 the largest L is the fastest at every shape, by 1.2 to 1.9 times over the next one
// (profiles/r25_kbench_eqrls.txt).  C stays an argument: the choice is the planner's to change.
constexpr unsigned eqrls_plan(size_t C, size_t p) {
    (void)C;
    const unsigned m = eqrls_admissible(p);
    unsigned b = 6;
    while (!(m >> b & 1u)) --b;
    return 1u << b;
}
int launch_eqrls(int mode, size_t p, size_t L, float lambda, cf32 *P, cf32 *w0, cf32 *w1, cf32 *hist, size_t C, size_t k,
                 const cf32 *x, size_t x_pitch, size_t n, const cf32 *d, size_t d_pitch, const cf32 *table, size_t M, cf32 *y,
                 size_t y_pitch, hipStream_t st);
// the same on the host, channel after channel
void eqrls_host(int mode, size_t p, float lambda, cf32 *P, cf32 *w0, cf32 *w1, cf32 *hist, size_t C, size_t k, const cf32 *x,
                size_t x_pitch, size_t n, const cf32 *d, size_t d_pitch, const cf32 *table, size_t M, cf32 *y,
                size_t y_pitch);

// ---- agc_kernels.hip -----------------------------------------------------------------------
// Agc (yagi_hip.h): C independent Agc<T> loops of one set of settings, one lane per channel, T = cf32 or float.  state is
// one AgcChan per channel, updated in place.  n rows in, n rows out; status (may be null) receives the squelch mode after
// every sample, one byte each.  y may be x at the same pitch.
constexpr int kAgcWg = 64;                             // channels per workgroup: one wave
constexpr int kAgcAhead = 8;                           // input rows per chunk: requested one chunk ahead, in registers
struct AgcChan {
    float g, y2p;                                      // the gain and the smoothed output energy y2'
    unsigned timer;                                    // squelch_timer
    uint8_t mode, locked, pad[2];                      // YAGI_AGC_SQUELCH_*; is_locked
};
static_assert(sizeof(AgcChan) == 16, "device layout");
struct AgcSettings {
    float alpha = 1e-2f, scale = 1.0f, threshold = 0.0f;
    unsigned timeout = 100;
    bool squelch = false;                              // every channel's mode is Disabled exactly when this is false
};
template <class T>
int launch_agc(const AgcSettings &g, AgcChan *state, size_t C, const T *x, size_t x_pitch, size_t n, T *y, size_t y_pitch,
               uint8_t *status, size_t status_pitch, hipStream_t st);
// sum[c] = the f32 sum of |x[i x_pitch + c]|^2 over i < n, in row order
template <class T>
int launch_agc_init(const T *x, size_t x_pitch, size_t n, size_t C, float *sum, hipStream_t st);
// the same on the host, channel after channel
template <class T>
void agc_host(const AgcSettings &g, AgcChan *state, size_t C, const T *x, size_t x_pitch, size_t n, T *y, size_t y_pitch,
              uint8_t *status, size_t status_pitch);
template <class T>
void agc_init_host(const T *x, size_t x_pitch, size_t n, size_t C, float *sum);
float agc_level_gain(float sum, size_t n);             // init: 1 / (sqrt(sum / n) + 1e-16)
float agc_rssi_gain(float rssi);                       // set_rssi: max(10^(-rssi / 20), 1e-16)
float agc_rssi(float g);                               // get_rssi: -20 yg_log10f(g)
void agc_words_host(int word, const float *x, size_t n, float *y);   // word 0 yg_lnf, 1 yg_expf, 2 yg_log10f

// ---- symtrack_kernels.hip ------------------------------------------------------------------
// SymTrack (yagi_hip.h): C independent receivers of one design, one lane per channel.  The state is the parts' own: one
// AgcChan, SymsyncChan and EqlmsChan per channel, the synchroniser's [Ls][C] history, the equalizer's [h_len][C] weights
// and window, plus one SymtrackChan (the oscillator's words, sync_index, num_syms, the stall reason).  All are updated in
// place (a workgroup touches its own channels only).  taps as for launch_symsync; osc_tab as for launch_osc_mix; map = the
// modem's M points followed, on the device, by reference[8] as floats.  status receives ny[C], the stall reason[C] and
// the low word of num_syms[C].  sym may be null.
constexpr int kSymtrackWg = 64;                        // channels per workgroup: one wave
constexpr int kSymtrackAhead = 16;                     // input rows per chunk: requested one chunk ahead, staged in LDS
constexpr size_t kSymtrackLdsMax = 160 * 1024;
struct SymtrackChan {
    uint32_t theta, d_theta;                           // Osc's words
    uint32_t index, stall;                             // synchroniser outputs since reset (its parity is what counts);
    unsigned long long num_syms;                       // YAGI_SYMTRACK_STALL_*; symbols since reset, as usize
};
static_assert(sizeof(SymtrackChan) == 24, "device layout");
struct SymtrackLoop {                                  // travels to the kernel by value with every call
    SymsyncLoop ss;
    float agc_alpha, agc_scale, eq_mu, pll_alpha, pll_beta;
    unsigned h_len, vco, strategy, M;
    int kind, bps;                                     // MODEM_*, never PSK or DPSK
    unsigned long long holdoff;
    float ref[8];                                      // reference[]: read by the host form (the kernel reads it behind map)
};
struct SymtrackState {
    AgcChan *agc;
    SymsyncChan *ss;
    EqlmsChan *eq;
    SymtrackChan *st;
    cf32 *ss_hist, *eq_w, *eq_hist;
};
constexpr size_t symtrack_stage_bytes() { return (size_t)kSymtrackAhead * kSymtrackWg * sizeof(cf32); }
constexpr size_t symtrack_osc_bytes(unsigned vco) { return (size_t)1024 * (vco ? 4 : 2) * sizeof(float); }
// the LDS a launch needs without the branch taps (which join where they still fit under kSymtrackLdsMax)
size_t symtrack_lds_bytes(size_t Ls, size_t h_len, int vco, size_t M);
int launch_symtrack(const SymtrackLoop &p, const float *taps, const void *osc_tab, const cf32 *map, const SymtrackState &s,
                    size_t C, const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch, uint8_t *sym,
                    size_t sym_pitch, size_t ycap, unsigned *status, hipStream_t st);
// the same on the host, channel after channel; every pointer a host pointer, map = the M points
void symtrack_host(const SymtrackLoop &p, const float *taps, const void *osc_tab, const cf32 *map, const SymtrackState &s,
                   size_t C, const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch, uint8_t *sym,
                   size_t sym_pitch, size_t ycap, unsigned *status);

// ---- channel_kernels.hip -------------------------------------------------------------------
// Channel (yagi_hip.h): C independent links of one shape, L taps each.  Nothing feeds back along time, so the grid runs
// over tiles of cw links x tile_steps steps; a workgroup of kChannelWg lanes is cw links wide and kChannelWg / cw steps
// deep, and every lane writes `rows` outputs.  link = one ChannelLink per link as of the object's last parameter
// change, `adv` the samples executed since (the phase and the counter of sample j of the call are link.theta +
// (u32)(adv + j) link.d_theta and link.t + adv + j).  taps = hrev [L][C]; win = the carried window, [L - 1][C], oldest
// first; win_next receives the window the call leaves (the caller flips).  x is [n][x_pitch], or one stream of n samples
// for every link where bcast.
constexpr int kChannelWg = 256;
constexpr size_t kChannelLdsMax = 160 * 1024;
constexpr size_t kChannelGridMax = (size_t)1 << 20;  // workgroups per launch: beyond that a workgroup loops over tiles
constexpr unsigned kChannelRowsMax = 16;               // outputs per lane: 1, 2, 4, 8 or 16
struct ChannelLink {
    float gamma, nstd;
    uint32_t theta, d_theta;                           // Osc's words
    unsigned long long t;                              // the noise counter
};
static_assert(kChannelGridMax >= YAGI_CHANNEL_CHANNELS_MAX, "one workgroup per link tile at least");
static_assert(sizeof(ChannelLink) == 24, "device layout");
struct ChannelShape {
    unsigned cw, rows;                                 // links per wave row (a power of two, 1 .. 64); outputs per lane
};
constexpr size_t channel_tile_steps(ChannelShape s) { return (size_t)(kChannelWg / s.cw) * s.rows; }
constexpr size_t channel_lds_bytes(ChannelShape s, size_t L, int vco, bool bcast) {
    return (size_t)1024 * (vco ? 4 : 2) * sizeof(float) + L * s.cw * sizeof(cf32) +
           (bcast ? channel_tile_steps(s) + (L - 1) + (L - 1) * s.cw : (channel_tile_steps(s) + (L - 1)) * s.cw) * sizeof(cf32);
}
static_assert(channel_lds_bytes(ChannelShape{64, kChannelRowsMax}, YAGI_CHANNEL_TAPS_MAX, 1, false) <= kChannelLdsMax,
              "the largest tile fits with the longest taps");
bool channel_shape_ok(ChannelShape s);
ChannelShape channel_plan(size_t C, size_t L, size_t n);      // the shape a call of n steps runs at where none is set
int launch_channel(ChannelShape s, int vco, bool bcast, const void *osc_tab, const ChannelLink *link, const cf32 *taps,
                   const cf32 *win, cf32 *win_next, uint64_t seed, uint64_t adv, size_t C, size_t L, const cf32 *x,
                   size_t x_pitch, size_t n, cf32 *y, size_t y_pitch, hipStream_t st);
// the same on the host, link after link, from a window of zeros (osc_tab = osc_device_table's image, host memory)
void channel_host(int vco, bool bcast, const void *osc_tab, const ChannelLink *link, const cf32 *taps, uint64_t seed, size_t C,
                  size_t L, const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch);
void channel_awgn_words(float n0_db, float snr_db, float *gamma, float *nstd);   // set_awgn's two words
// the words of channel_words.hpp on arrays: (C, S)[k2] as f64, R[k1], the noise of (seed, link, counter first + i)
void channel_cos_sin_host(const uint32_t *k2, size_t n, double *c, double *s);
void channel_radius_host(const uint32_t *k1, size_t n, float *r);
void channel_noise_host(uint64_t seed, uint64_t link, uint64_t first, size_t n, cf32 *out);

// ---- symstream_kernels.hip -----------------------------------------------------------------
// SymStream (yagi_hip.h): samples [0, n) of a call that starts at buf_index p, from the carried window `win` (Ls values,
// oldest first) and new symbols that come either from the caller's bytes (sym, flag = the result of
// launch_symstream_check on them, null where M = 256) or from the LFSR (src).  hb = the interpolator's [k][Ls] branch
// taps, map = the modem's M points.  win_next receives the window the call leaves where it pushes at least one symbol
// (ceil((p + n) / k) - (p > 0) of them: the caller flips then), buf[i] branch i of the last symbol for the branches
// the call does not write.  Served shapes: symstream_fused_serves.
constexpr int kSymStrides = 8;                         // lane-stride matrices: one per bit of the lane number in a workgroup
constexpr size_t kSymStrideWords = (size_t)8 * kSymStrides * 32;
struct SymSource {
    const unsigned *pow, *stride;                      // device: T^(2^b) (kMseqPowWords); symstream_strides' table
    unsigned s0, g, nmask;
    int m, bps, run;                                   // run = symstream_run(k, Ls), what `stride` was built for
};
int symstream_max_slots(int k, int Ls);                // most symbol slots a workgroup stages (a multiple of the bank tile)
int symstream_wg_slots(int k, int Ls, size_t nslots);  // slots per workgroup of a call that touches nslots
int symstream_run(int k, int Ls);                      // consecutive symbols a lane generates
void symstream_strides(const unsigned *pow, int run, unsigned *stride);   // T^(run * bps * 2^b), bps = 1 .. 8, b < 8
size_t symstream_lds_bytes(int k, int Ls, int M, int wg_slots);   // dynamic LDS of the fused launch
bool symstream_fused_serves(int k, int Ls, int M);
int launch_symstream(const cf32 *win, const float *hb, int k, int Ls, float scale, const cf32 *map, int M, float gain,
                     const uint8_t *sym, const int *flag, const SymSource *src, int p, size_t n, cf32 *y, cf32 *win_next,
                     cf32 *buf, hipStream_t st);
int launch_symstream_check(int M, const uint8_t *sym, size_t n, int *flag, hipStream_t st);   // zeroes flag first
int launch_symstream_gain(cf32 *v, size_t n, float gain, hipStream_t st);                    // v[i] = (re gain, im gain)

// ---- symstreamr_kernels.hip ----------------------------------------------------------------
// SymStreamR (yagi_hip.h): `need` samples of a k = 2 SymStream (symbol window swin, branch taps shb [2][Ls], buf_index p,
// LFSR source src with the strides of symstream_run(2, Ls)) pushed through a Resamp (window rwin of Lr samples, bank
// rhb [2^bits][Lr], phase p0) in one launch: all ny = num_output(need) outputs, output j to ya[j] for j < split and to
// yb[j - split] behind it.  swin_next (where the call pushes a symbol: ceil((p + need) / 2) - p > 0), rwin_next and
// buf[1] (where p + need is odd) receive what the call leaves; the caller flips and advances as after the two
// launchers.  Served shapes: symstreamr_fused_serves.
int symstreamr_tile(uint32_t step, int Lr);                                    // resamp_plan's tile: outputs per tile
int symstreamr_max_tiles(uint32_t step, int Lr, int Ls, int run);              // most tiles a workgroup stages
int symstreamr_wg_tiles(uint32_t step, int Lr, int Ls, int run, size_t ny);    // tiles per workgroup of a call of ny outputs
size_t symstreamr_lds_bytes(uint32_t step, int Lr, int Ls, int M, int wg_tiles);
bool symstreamr_fused_serves(uint32_t step, int Lr, int Ls, int M, int run);
int launch_symstreamr(const cf32 *swin, const float *shb, int Ls, float scale, const cf32 *map, int M, float gain,
                      const SymSource &src, int p, const cf32 *rwin, const float *rhb, int Lr, int bits, uint32_t step,
                      uint32_t p0, size_t need, size_t ny, cf32 *ya, size_t split, cf32 *yb, cf32 *swin_next,
                      cf32 *rwin_next, cf32 *buf, hipStream_t st);

// ---- convcode_kernels.hip ------------------------------------------------------------------
// ConvCode (yagi_hip.h): a convolutional code and its puncture table; F frames per call, one per row of a byte plane.
// off[j] holds, a byte per output r, the index within a period of bit (column j, output r): the kept bits of the columns
// below j plus those of column j below r; keep[j] has bit r set where that bit is kept.  Unpunctured codes are p = 1.
struct ConvCode {
    int K = 0, R = 0, p = 1, terminated = 1;
    unsigned g[4] = {0, 0, 0, 0};
    unsigned kp = 0;                                   // kept bits of a period
    uint32_t off[YAGI_CONVCODE_PERIOD_MAX] = {}, keep[YAGI_CONVCODE_PERIOD_MAX] = {};
    size_t states() const { return (size_t)1 << (K - 1); }
    size_t steps(size_t n) const { return n + (terminated ? (size_t)(K - 1) : 0); }
    size_t pos(size_t t) const { return t / (size_t)p * kp + (off[t % (size_t)p] & 0xffu); }   // kept bits before step t
    size_t ncoded(size_t n) const { return pos(steps(n)); }
    size_t nmax() const {
        size_t T = (size_t)YAGI_CONVCODE_DECISION_BYTES * 8 / states();
        if (T > (size_t)YAGI_CONVCODE_STEPS_MAX) T = YAGI_CONVCODE_STEPS_MAX;
        return T - (terminated ? (size_t)(K - 1) : 0);
    }
};
constexpr size_t kConvTableWords = 2 * YAGI_CONVCODE_PERIOD_MAX;      // the device image: off[32], keep[32]
constexpr size_t kConvLdsMax = 160 * 1024;
constexpr unsigned kConvStage = 256;                   // staged (frame, step) pairs per wave and chunk
// The decoder's arrangement: a lane holds spl = max(1, S / 64) states, a wave fpw frames (fpw S <= 64 lanes), a workgroup
// `waves` waves; each wave stages the soft bytes of its frames chunk = kConvStage / fpw steps at a time.
struct ConvShape {
    unsigned fpw, waves;
};
constexpr unsigned conv_spl(int K) { return K > 7 ? 1u << (K - 7) : 1u; }
constexpr unsigned conv_fpw_max(int K) { return K < 7 ? 1u << (7 - K) : 1u; }
constexpr unsigned conv_fpw_min(int K) { return K < 4 ? 2u : 1u; }     // a wave's step is at least one whole byte of decisions
constexpr unsigned conv_chunk(ConvShape s) { return kConvStage / s.fpw; }
// decision bytes of one wave and step: the fpw S bits of its frames, or spl ballots
constexpr size_t conv_step_bytes(int K, ConvShape s) { return K > 7 ? (size_t)8 << (K - 7) : ((size_t)s.fpw << (K - 1)) / 8; }
// per wave: the decisions of T steps (padded to 8 bytes), kConvStage expanded steps of 8 bytes, and per frame the raw bytes
// of a chunk (4 per step at most, plus the 8 of two partial words); per workgroup the table
constexpr size_t conv_wave_bytes(int K, ConvShape s, size_t T) {
    return ((T * conv_step_bytes(K, s) + 7) & ~(size_t)7) + (size_t)kConvStage * 8 + (size_t)s.fpw * (conv_chunk(s) * 4 + 8);
}
constexpr size_t conv_lds_bytes(int K, ConvShape s, size_t T) {
    return kConvTableWords * 4 + s.waves * conv_wave_bytes(K, s, T);
}
static_assert(conv_lds_bytes(7, ConvShape{1, 1}, 16384) <= kConvLdsMax && conv_lds_bytes(9, ConvShape{1, 1}, 4096) <= kConvLdsMax &&
              conv_lds_bytes(3, ConvShape{2, 1}, YAGI_CONVCODE_STEPS_MAX) <= kConvLdsMax,
              "the longest frame of every K fits at the narrowest arrangement");
bool conv_shape_ok(int K, ConvShape s);
ConvShape conv_plan(int K, size_t T, size_t F);       // the shape a call of F frames of T steps runs at where none is set
void conv_table(const ConvCode &c, uint32_t *words);   // kConvTableWords words
// device forms; tab = conv_table's image on the device
int launch_conv_encode(const ConvCode &c, const uint32_t *tab, const uint8_t *msg, size_t msg_pitch, size_t n, size_t F,
                       uint8_t *coded, size_t coded_pitch, hipStream_t st);
int launch_conv_decode(const ConvCode &c, ConvShape s, const uint32_t *tab, const uint8_t *soft, size_t soft_pitch, size_t n,
                       size_t F, uint8_t *msg, size_t msg_pitch, uint32_t *metric, hipStream_t st);
// the definition's sequential loops on the host, frame after frame
void conv_encode_host(const ConvCode &c, const uint8_t *msg, size_t msg_pitch, size_t n, size_t F, uint8_t *coded,
                      size_t coded_pitch);
void conv_decode_host(const ConvCode &c, const uint8_t *soft, size_t soft_pitch, size_t n, size_t F, uint8_t *msg,
                      size_t msg_pitch, uint32_t *metric);

// ---- packetizer_kernels.hip ----------------------------------------------------------------
// Packetizer (yagi_hip.h): n payload bytes, a CRC of w bytes behind them, ConvCode over the 8 (n + w) message bits, a block
// interleaver of `columns` columns over the N coded bits and the scrambler's mask; F frames per call, one per row.
struct CrcParams {
    int width;                                         // 0, 8, 16, 24, 32
    uint32_t poly, init, xorout;
    bool reflected;                                    // input bytes and the result
};
bool crc_params(int scheme, CrcParams *out);           // YAGI_CRC_*; false where the scheme is none of them
uint32_t crc_host(const CrcParams &c, const uint8_t *data, size_t n);
struct Packetizer {
    ConvCode code;
    CrcParams crc{};
    int scheme = 0;
    size_t n = 0, columns = 1;
    bool scramble = true;
    size_t w() const { return (size_t)crc.width / 8; }
    size_t msg_bits() const { return 8 * (n + w()); }
    size_t N() const { return code.ncoded(msg_bits()); }
    size_t nsym(unsigned bps) const { return (N() + bps - 1) / bps; }
    size_t cols() const { return columns < N() ? columns : N(); }      // C >= N is the identity, as C = N is
};
// the device image: ConvCode's table; the coded index within a period -> step | output << 8; the encoder's per-lane powers
// x^(8 * bytes behind the lane's slice) mod P; the decoder's (T[i], i) pairs for the CRC register run backwards
constexpr size_t kPktInvAt = kConvTableWords, kPktInvWords = 4 * YAGI_CONVCODE_PERIOD_MAX;
constexpr size_t kPktZAt = kPktInvAt + kPktInvWords, kPktZWords = 256;
constexpr size_t kPktRevAt = kPktZAt + kPktZWords, kPktRevWords = 512;
constexpr size_t kPktTableWords = kPktRevAt + kPktRevWords;
constexpr size_t pkt_slice(size_t n) { return (n + kPktZWords - 1) / kPktZWords; }     // payload bytes per encoder lane
// per wave: the decisions and the expanded steps (no raw words); per workgroup ConvCode's table and, with a CRC, the pairs
constexpr size_t pkt_wave_bytes(int K, ConvShape s, size_t T) {
    return ((T * conv_step_bytes(K, s) + 7) & ~(size_t)7) + (size_t)kConvStage * 8;
}
constexpr size_t pkt_lds_bytes(int K, ConvShape s, size_t T, bool with_crc) {
    return kConvTableWords * 4 + s.waves * pkt_wave_bytes(K, s, T) + (with_crc ? kPktRevWords * 4 : 0);
}
void pkt_table(const Packetizer &k, uint32_t *words);  // kPktTableWords words
void pkt_permutation(size_t N, size_t C, uint32_t *pi);                // pi[i], the transmit position of coder-order bit i
void scramble_data_host(uint8_t *x, size_t n);         // scramble.rs scramble_data (= unscramble_data)
void unscramble_soft_host(uint8_t *x, size_t n);       // scramble.rs unscramble_data_soft
// device forms; tab = pkt_table's image on the device; the decoder runs at ConvCode's arrangement s
int launch_pkt_encode(const Packetizer &k, const uint32_t *tab, const uint8_t *payload, size_t payload_pitch, size_t F,
                      unsigned bps, uint8_t *tx, size_t tx_pitch, hipStream_t st);
int launch_pkt_decode(const Packetizer &k, ConvShape s, const uint32_t *tab, const uint8_t *soft, size_t soft_pitch, size_t F,
                      uint8_t *payload, size_t payload_pitch, uint8_t *valid, uint32_t *crc, uint32_t *metric, hipStream_t st);
// the definition's loops on the host, around conv_encode_host / conv_decode_host
void pkt_encode_host(const Packetizer &k, const uint8_t *payload, size_t payload_pitch, size_t F, unsigned bps, uint8_t *tx,
                     size_t tx_pitch);
void pkt_decode_host(const Packetizer &k, const uint8_t *soft, size_t soft_pitch, size_t F, uint8_t *payload,
                     size_t payload_pitch, uint8_t *valid, uint32_t *crc, uint32_t *metric);

}  // namespace yagi
