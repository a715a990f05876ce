/*
 * yagi_hip.h -- C ABI of libyagi_hip.so: the MI355X (gfx950) FIR/FFT engine that sits behind
 * yagi's `new / push / execute / execute_block` object API.
 *
 * yagi (EEGKit/yagi, Rust) has no FFI of its own for this path; its only C-ABI precedent is the
 * stub `c_shim` (c_shim/src/lib.rs:3-12: opaque `*mut foo_s` handle, `c_uint` sizes, `c_int`
 * status).  The entry points below are what a `hip` feature of yagi would bind with
 * `extern "C"` (see INTEGRATION.md for the Rust side).  Every group cites the reference item
 * (file:line, relative to the reference root) whose behaviour it reproduces.
 *
 * Conventions
 *   - Complex samples are `yagi_cf32` = `num_complex::Complex<f32>` (#[repr(C)] {re, im}).
 *   - Type suffixes follow liquid-dsp / yagi's test names:
 *       rrrf = FirFilter<f32, f32>, crcf = FirFilter<Complex32, f32>,
 *       cccf = FirFilter<Complex32, Complex32>   (T = sample/output type, C = Coeff type).
 *   - Every function returns a yagi_status (0 = OK).  The variants mirror error::Error
 *     (src/error.rs:7-14); YAGI_ERR_DEVICE is added for HIP/RCCL failures.  Where the reference
 *     panics on a slice index (firdecim.rs:182, dotprod/mod.rs:104, fft/mod.rs:46) this library
 *     returns YAGI_ERR_CONFIG instead of aborting.  yagi_hip_last_error() gives the message
 *     (thread-local), like the String each Error variant carries.
 *   - Pointers are HOST pointers unless the function name ends in `_dev`, in which case data
 *     pointers are device (HBM) pointers and the call is asynchronous on the handle's stream.
 *   - ALIGNMENT AND EXTENT: a device operand needs the alignment of its element type and no more (4 bytes for
 *     `float` and `uint32_t`, 8 bytes for `yagi_cf32`): a stream cut at an odd sample is a legal operand, and the
 *     kernels take their 16-byte paths only where the pointer they are given allows it.  A call writes exactly its
 *     documented output range and nothing else, and reads nothing outside its documented input range whose value
 *     could reach a result.  Where a call reports its own count (`*nw` of the arbitrary resamplers, capacity
 *     `ny_cap`), exactly `*nw` elements are written and `[*nw, ny_cap)` is left untouched.
 *   - NO ALIASING: the input and output ranges of a `_dev` block call must not overlap (no in-place
 *     execution): the kernels read tile halos and the carried window from the input while other
 *     workgroups already store the output.  Rust's borrows (`&[T]` in, `&mut [T]` out) make such a
 *     call unwritable in the reference; here it returns YAGI_ERR_CONFIG.
 *   - A handle owns its device taps, its device window (the filter state), a workspace and a
 *     stream reference.  One handle = one owner thread at a time (the reference's `&mut self`);
 *     distinct handles may be used concurrently.  Fft plans are read-only once created.
 *   - There is NO CPU fallback: every arithmetic result is produced by a HIP kernel; if no
 *     device is present the first call fails with YAGI_ERR_DEVICE.
 */
#ifndef YAGI_HIP_H
#define YAGI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { float re, im; } yagi_cf32;

typedef enum {
    YAGI_OK = 0,
    YAGI_ERR_INTERNAL = 1,        /* Error::Internal       error.rs:8  */
    YAGI_ERR_CONFIG = 2,          /* Error::Config         error.rs:9  */
    YAGI_ERR_VALUE = 3,           /* Error::Value          error.rs:10 */
    YAGI_ERR_RANGE = 4,           /* Error::Range          error.rs:11 */
    YAGI_ERR_MODE = 5,            /* Error::Mode           error.rs:12 */
    YAGI_ERR_NO_CONVERGENCE = 6,  /* Error::NoConvergence  error.rs:13 */
    YAGI_ERR_DEVICE = 7           /* HIP / RCCL failure (no reference counterpart) */
} yagi_status;

typedef void *yagi_stream_t;      /* a hipStream_t; NULL = the default stream */

/* fft::Direction (src/fft/mod.rs:13-17) */
#define YAGI_FFT_FORWARD 0
#define YAGI_FFT_BACKWARD 1

const char *yagi_hip_last_error(void);
const char *yagi_hip_version(void);

/* ---- device plumbing (no reference counterpart: the reference has no device boundary) ---- */
int yagi_hip_device_count(int *count);
int yagi_hip_set_device(int device);
int yagi_hip_malloc(void **dev_ptr, size_t bytes);
int yagi_hip_free(void *dev_ptr);
int yagi_hip_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
int yagi_hip_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);
int yagi_hip_memset_dev(void *dst_dev, int value, size_t bytes);
int yagi_hip_device_synchronize(void);
int yagi_hip_stream_synchronize(yagi_stream_t stream);

/* Synthetic input: counter-based SplitMix64 + Box-Muller in the shape of
 * random::randnf / crandnf (src/random/normal.rs:9-44); sample i of a stream depends only on
 * (seed, first + i).  Complex samples have re, im ~ N(0, 1/2). */
int yagi_hip_gen_real_dev(uint64_t seed, uint64_t first, size_t n, float *x_dev, yagi_stream_t s);
int yagi_hip_gen_complex_dev(uint64_t seed, uint64_t first, size_t n, yagi_cf32 *x_dev, yagi_stream_t s);

/* ---- dotprod: trait DotProd (src/dotprod/mod.rs:13-73) -----------------------------------
 *   rrrf: [f32].[f32]            mod.rs:19-31      rccf: [f32].[Complex]      mod.rs:33-45
 *   crcf: [Complex].[f32]        mod.rs:47-59      cccf: [Complex].[Complex]  mod.rs:61-73
 * y = sum_i a[i]*b[i] over n = the common length.  Kernel: per-lane strided FMA, wave64
 * shuffle tree, LDS cross-wave, fixed-order two-pass combine (bitwise reproducible). */
int yagi_hip_dotprod_rrrf(const float *a, const float *b, size_t n, float *y);
int yagi_hip_dotprod_rccf(const float *a, const yagi_cf32 *b, size_t n, yagi_cf32 *y);
int yagi_hip_dotprod_crcf(const yagi_cf32 *a, const float *b, size_t n, yagi_cf32 *y);
int yagi_hip_dotprod_cccf(const yagi_cf32 *a, const yagi_cf32 *b, size_t n, yagi_cf32 *y);
int yagi_hip_dotprod_rrrf_dev(const float *a, const float *b, size_t n, float *y, yagi_stream_t s);
int yagi_hip_dotprod_rccf_dev(const float *a, const yagi_cf32 *b, size_t n, yagi_cf32 *y, yagi_stream_t s);
int yagi_hip_dotprod_crcf_dev(const yagi_cf32 *a, const float *b, size_t n, yagi_cf32 *y, yagi_stream_t s);
int yagi_hip_dotprod_cccf_dev(const yagi_cf32 *a, const yagi_cf32 *b, size_t n, yagi_cf32 *y, yagi_stream_t s);

/* ---- FIR objects --------------------------------------------------------------------------
 * YAGI_FIR_API(K, T, C) declares, for type combination K:
 *
 * firfilt  = FirFilter<T,C>             src/filter/fir/firfilt.rs
 *   create              new(h)                          :63-79   (h_len == 0 -> CONFIG)
 *   create_kaiser       new_kaiser(n, fc, as_, mu)      :93-97   (design: kaiser.rs:16-51)
 *   create_rnyquist     new_rnyquist(ftype, k, m, beta, mu) :112-116 (design: yagi_hip_fir_design_prototype; 2km+1 taps)
 *   create_rect         new_rect(n)                     :149-155 (n in [1,1024])
 *   create_dc_blocker   new_dc_blocker(m, as_)          :166-170 (design/mod.rs:336-378 fir_design_notch at f0 = 0)
 *   create_notch        new_notch(m, as_, f0)           :183-186 (real taps: notch pair at +-f0; complex taps: the
 *                                                       DC blocker mixed to f0, firfilt.rs:25-44)
 *   clone               #[derive(Clone)]                :8       (state continues identically)
 *   set_coefficients    set_coefficients(h) (+reset)    :193-206
 *   reset               reset()                         :209-213
 *   push / write        push(x) / write(&[x])           :220-234
 *   execute             execute() -> T                  :241-246 (dotprod kernel on the window)
 *   execute_one         execute_one(x)                  :256-259
 *   execute_block       execute_block(x, y)             :267-278 (nx != ny -> CONFIG)
 *   set_scale/get_scale/get_length/get_coefficients      :285-314
 *   freqresponse        freqresponse(fc)                :325-328 (design/mod.rs:666-675; host arithmetic on the taps)
 *   groupdelay          groupdelay(fc)                  :339-342 (design/mod.rs:687-704)
 *   y[i] = scale * sum_{k<L} h[k] * x[i-k], history zero at start.
 *
 * firdecim = FirDecimationFilter<T,C>   src/filter/fir/firdecim.rs
 *   create              new(M, h, h_len)                :38-57   (h_len==0 or M==0 -> CONFIG)
 *   create_kaiser       new_kaiser(M, m, as_)           :70-87   (M<2, m==0, as_<0 -> CONFIG)
 *   create_prototype    new_prototype(ftype, M, m, beta, dt) :102-121 (M<2, m==0, beta outside [0,1], dt outside
 *                                                       [-1,1] -> CONFIG; design: yagi_hip_fir_design_prototype)
 *   execute             execute(&x[..M]) -> T           :179-191
 *   execute_block       execute_block(x, n, y)          :200-205 (x holds n*M samples)
 *   y[i] = scale * sum_k h[k] * x[i*M - k].
 *
 * firpfb   = FirPfbFilter<T,C>          src/filter/fir/firpfb.rs
 *   create              new(num_filters, h, h_len)      :34-65   (h_sub_len = h_len / num_filters)
 *   create_kaiser       new_kaiser(M, m, fc, as_)       :94-114
 *   create_default      default(M, m)                   :79-81
 *   push / write / execute(i) / execute_block(i, x, y)  :255-301 (i >= num_filters -> CONFIG)
 *   execute_all_dev     all num_filters branch outputs for every pushed sample (polyphase
 *                       interpolator form, firinterp.rs:224-231): y[n][i], n-major
 *   execute_select_dev  branch index per sample (the access pattern of resamp.rs:141-154)
 *   y_i[n] = scale * sum_k h[i + k*M] * x[n-k].
 *
 * `_dev` variants take device pointers and run asynchronously on the handle's stream.
 */
#define YAGI_FIR_API(K, T, C)                                                                       \
    typedef struct yagi_hip_firfilt_##K##_s *yagi_hip_firfilt_##K;                                  \
    int yagi_hip_firfilt_##K##_create(const C *h, size_t h_len, yagi_hip_firfilt_##K *q);           \
    int yagi_hip_firfilt_##K##_create_kaiser(size_t n, float fc, float as_, float mu,               \
                                             yagi_hip_firfilt_##K *q);                              \
    int yagi_hip_firfilt_##K##_create_rnyquist(int ftype, size_t k, size_t m, float beta, float mu, \
                                               yagi_hip_firfilt_##K *q);                            \
    int yagi_hip_firfilt_##K##_create_rect(size_t n, yagi_hip_firfilt_##K *q);                      \
    int yagi_hip_firfilt_##K##_create_dc_blocker(size_t m, float as_, yagi_hip_firfilt_##K *q);     \
    int yagi_hip_firfilt_##K##_create_notch(size_t m, float as_, float f0, yagi_hip_firfilt_##K *q);\
    int yagi_hip_firfilt_##K##_destroy(yagi_hip_firfilt_##K q);                                     \
    int yagi_hip_firfilt_##K##_clone(yagi_hip_firfilt_##K q, yagi_hip_firfilt_##K *out);            \
    int yagi_hip_firfilt_##K##_set_stream(yagi_hip_firfilt_##K q, yagi_stream_t s);                 \
    int yagi_hip_firfilt_##K##_set_coefficients(yagi_hip_firfilt_##K q, const C *h, size_t h_len);  \
    int yagi_hip_firfilt_##K##_reset(yagi_hip_firfilt_##K q);                                       \
    int yagi_hip_firfilt_##K##_push(yagi_hip_firfilt_##K q, T x);                                   \
    int yagi_hip_firfilt_##K##_write(yagi_hip_firfilt_##K q, const T *x, size_t n);                 \
    int yagi_hip_firfilt_##K##_execute(yagi_hip_firfilt_##K q, T *y);                               \
    int yagi_hip_firfilt_##K##_execute_one(yagi_hip_firfilt_##K q, T x, T *y);                      \
    int yagi_hip_firfilt_##K##_execute_block(yagi_hip_firfilt_##K q, const T *x, size_t nx, T *y,   \
                                             size_t ny);                                            \
    int yagi_hip_firfilt_##K##_execute_block_dev(yagi_hip_firfilt_##K q, const T *x_dev, size_t n,  \
                                                 T *y_dev);                                         \
    int yagi_hip_firfilt_##K##_set_pipeline(yagi_hip_firfilt_##K q, int on);  /* as yagi_hip_firfft_crcf_set_pipeline: */ \
    int yagi_hip_firfilt_##K##_join(yagi_hip_firfilt_##K q);  /* consecutive execute_block_dev calls overlap; y_dev and x_dev's reuse are ordered after join */ \
    int yagi_hip_firfilt_##K##_set_scale(yagi_hip_firfilt_##K q, C scale);                          \
    int yagi_hip_firfilt_##K##_get_scale(yagi_hip_firfilt_##K q, C *scale);                         \
    int yagi_hip_firfilt_##K##_get_length(yagi_hip_firfilt_##K q, size_t *h_len);                   \
    int yagi_hip_firfilt_##K##_get_coefficients(yagi_hip_firfilt_##K q, C *h, size_t h_len);        \
    int yagi_hip_firfilt_##K##_freqresponse(yagi_hip_firfilt_##K q, float fc, yagi_cf32 *H);        \
    int yagi_hip_firfilt_##K##_groupdelay(yagi_hip_firfilt_##K q, float fc, float *delay);          \
                                                                                                    \
    typedef struct yagi_hip_firdecim_##K##_s *yagi_hip_firdecim_##K;                                \
    int yagi_hip_firdecim_##K##_create(size_t M, const C *h, size_t h_len,                          \
                                       yagi_hip_firdecim_##K *q);                                   \
    int yagi_hip_firdecim_##K##_create_kaiser(size_t M, size_t m, float as_,                        \
                                              yagi_hip_firdecim_##K *q);                            \
    int yagi_hip_firdecim_##K##_create_prototype(int ftype, size_t M, size_t m, float beta,         \
                                                 float dt, yagi_hip_firdecim_##K *q);               \
    int yagi_hip_firdecim_##K##_destroy(yagi_hip_firdecim_##K q);                                   \
    int yagi_hip_firdecim_##K##_clone(yagi_hip_firdecim_##K q, yagi_hip_firdecim_##K *out);         \
    int yagi_hip_firdecim_##K##_set_stream(yagi_hip_firdecim_##K q, yagi_stream_t s);               \
    int yagi_hip_firdecim_##K##_reset(yagi_hip_firdecim_##K q);                                     \
    int yagi_hip_firdecim_##K##_get_decim_rate(yagi_hip_firdecim_##K q, size_t *M);                 \
    int yagi_hip_firdecim_##K##_set_scale(yagi_hip_firdecim_##K q, C scale);                        \
    int yagi_hip_firdecim_##K##_get_scale(yagi_hip_firdecim_##K q, C *scale);                       \
    int yagi_hip_firdecim_##K##_freqresp(yagi_hip_firdecim_##K q, float fc, yagi_cf32 *H);          \
    int yagi_hip_firdecim_##K##_execute(yagi_hip_firdecim_##K q, const T *x, size_t nx, T *y);      \
    int yagi_hip_firdecim_##K##_execute_block(yagi_hip_firdecim_##K q, const T *x, size_t nx,       \
                                              size_t n, T *y);                                      \
    int yagi_hip_firdecim_##K##_execute_block_dev(yagi_hip_firdecim_##K q, const T *x_dev,          \
                                                  size_t n, T *y_dev);                              \
                                                                                                    \
    typedef struct yagi_hip_firpfb_##K##_s *yagi_hip_firpfb_##K;                                    \
    int yagi_hip_firpfb_##K##_create(size_t num_filters, const C *h, size_t h_len,                  \
                                     yagi_hip_firpfb_##K *q);                                       \
    int yagi_hip_firpfb_##K##_create_kaiser(size_t num_filters, size_t m, float fc, float as_,      \
                                            yagi_hip_firpfb_##K *q);                                \
    int yagi_hip_firpfb_##K##_create_default(size_t num_filters, size_t m,                          \
                                             yagi_hip_firpfb_##K *q);                               \
    int yagi_hip_firpfb_##K##_destroy(yagi_hip_firpfb_##K q);                                       \
    int yagi_hip_firpfb_##K##_clone(yagi_hip_firpfb_##K q, yagi_hip_firpfb_##K *out);               \
    int yagi_hip_firpfb_##K##_set_stream(yagi_hip_firpfb_##K q, yagi_stream_t s);                   \
    int yagi_hip_firpfb_##K##_reset(yagi_hip_firpfb_##K q);                                         \
    int yagi_hip_firpfb_##K##_set_scale(yagi_hip_firpfb_##K q, C scale);                            \
    int yagi_hip_firpfb_##K##_get_scale(yagi_hip_firpfb_##K q, C *scale);                           \
    int yagi_hip_firpfb_##K##_push(yagi_hip_firpfb_##K q, T x);                                     \
    int yagi_hip_firpfb_##K##_write(yagi_hip_firpfb_##K q, const T *x, size_t n);                   \
    int yagi_hip_firpfb_##K##_execute(yagi_hip_firpfb_##K q, size_t i, T *y);                       \
    int yagi_hip_firpfb_##K##_execute_block(yagi_hip_firpfb_##K q, size_t i, const T *x,            \
                                            size_t nx, T *y, size_t ny);                            \
    int yagi_hip_firpfb_##K##_execute_block_dev(yagi_hip_firpfb_##K q, size_t i, const T *x_dev,    \
                                                size_t n, T *y_dev);                                \
    int yagi_hip_firpfb_##K##_execute_all_dev(yagi_hip_firpfb_##K q, const T *x_dev, size_t n,      \
                                              T *y_dev);                                            \
    int yagi_hip_firpfb_##K##_execute_select_dev(yagi_hip_firpfb_##K q, const uint32_t *idx_dev,    \
                                                 const T *x_dev, size_t n, T *y_dev);

YAGI_FIR_API(rrrf, float, float)
YAGI_FIR_API(crcf, yagi_cf32, float)
YAGI_FIR_API(cccf, yagi_cf32, yagi_cf32)

/* ---- FftFilt<T,Coeff>: src/filter/fftfilt.rs (overlap-add fast convolution, block n, FFT 2n) ------
 *   create            create(h, n)                     :46-84   (h_len == 0 or n < h_len-1 -> CONFIG;
 *                                                               additionally 2n <= 8192 in this engine)
 *   reset             reset()                          :86-88
 *   set_scale/get_scale                                :95-101  (internally scale/(2n), like the reference)
 *   execute           execute(x, y)                    :103-138 (x.len() != n or y.len() != n -> CONFIG)
 *   execute_blocks    `nblocks` consecutive execute() calls as one batch (device-friendly form)
 *   get_length        get_length()                     :140-142
 * y = overlap-add of IFFT(FFT([x;0]) * FFT([h;0])) * scale; for rrrf the real part is returned
 * (FromComplex32 for f32, fftfilt.rs:16-20). */
#define YAGI_FFTFILT_API(K, T, C)                                                                   \
    typedef struct yagi_hip_fftfilt_##K##_s *yagi_hip_fftfilt_##K;                                  \
    int yagi_hip_fftfilt_##K##_create(const C *h, size_t h_len, size_t n, yagi_hip_fftfilt_##K *q); \
    int yagi_hip_fftfilt_##K##_destroy(yagi_hip_fftfilt_##K q);                                     \
    int yagi_hip_fftfilt_##K##_clone(yagi_hip_fftfilt_##K q, yagi_hip_fftfilt_##K *out);            \
    int yagi_hip_fftfilt_##K##_set_stream(yagi_hip_fftfilt_##K q, yagi_stream_t s);                 \
    int yagi_hip_fftfilt_##K##_reset(yagi_hip_fftfilt_##K q);                                       \
    int yagi_hip_fftfilt_##K##_set_scale(yagi_hip_fftfilt_##K q, C scale);                          \
    int yagi_hip_fftfilt_##K##_get_scale(yagi_hip_fftfilt_##K q, C *scale);                         \
    int yagi_hip_fftfilt_##K##_get_length(yagi_hip_fftfilt_##K q, size_t *h_len);                   \
    int yagi_hip_fftfilt_##K##_execute(yagi_hip_fftfilt_##K q, const T *x, size_t nx, T *y,         \
                                       size_t ny);                                                  \
    int yagi_hip_fftfilt_##K##_execute_blocks(yagi_hip_fftfilt_##K q, const T *x, size_t nblocks,   \
                                              T *y);                                                \
    int yagi_hip_fftfilt_##K##_execute_blocks_dev(yagi_hip_fftfilt_##K q, const T *x_dev,           \
                                                  size_t nblocks, T *y_dev);

YAGI_FFTFILT_API(rrrf, float, float)
YAGI_FFTFILT_API(crcf, yagi_cf32, float)
YAGI_FFTFILT_API(cccf, yagi_cf32, yagi_cf32)

/* ---- FirInterpolationFilter<T,Coeff>: src/filter/fir/firinterp.rs (polyphase interpolator) ---------
 *   create           new(interp, h, h_len)        :36-60   (interp < 2 or h_len < interp -> CONFIG; taps
 *                                                          zero-padded to a multiple of interp)
 *   create_kaiser    new_kaiser(interp, m, as_)   :73-90   (uses the first 2*interp*m taps)
 *   create_prototype new_prototype(ftype, interp, m, beta, dt)   :105-124 (interp < 2, m == 0, beta outside [0,1],
 *                                                          dt outside [-1,1] -> CONFIG; all 2*interp*m+1 taps of
 *                                                          yagi_hip_fir_design_prototype: sub-filters of 2m+1)
 *   create_linear    new_linear(interp)           :135-147
 *   create_window    new_window(interp, m)        :159-174
 *   execute          execute(x, &mut y[..interp]) :224-231 (push x, then every branch in order)
 *   execute_block    execute_block(x, y)          :239-244 (y holds n*interp samples)
 *   flush            flush(y)                     :251-253 (execute with a zero input)
 *   reset / get_interp_rate / get_sub_len / set_scale / get_scale   :177-215
 * Device form: firpfb_all_kernel (all branches per pushed sample, output n-major). */
#define YAGI_FIRINTERP_API(K, T, C)                                                                 \
    typedef struct yagi_hip_firinterp_##K##_s *yagi_hip_firinterp_##K;                              \
    int yagi_hip_firinterp_##K##_create(size_t interp, const C *h, size_t h_len,                    \
                                        yagi_hip_firinterp_##K *q);                                 \
    int yagi_hip_firinterp_##K##_create_kaiser(size_t interp, size_t m, float as_,                  \
                                               yagi_hip_firinterp_##K *q);                          \
    int yagi_hip_firinterp_##K##_create_prototype(int ftype, size_t interp, size_t m, float beta,   \
                                                  float dt, yagi_hip_firinterp_##K *q);             \
    int yagi_hip_firinterp_##K##_create_linear(size_t interp, yagi_hip_firinterp_##K *q);           \
    int yagi_hip_firinterp_##K##_create_window(size_t interp, size_t m, yagi_hip_firinterp_##K *q); \
    int yagi_hip_firinterp_##K##_destroy(yagi_hip_firinterp_##K q);                                 \
    int yagi_hip_firinterp_##K##_clone(yagi_hip_firinterp_##K q, yagi_hip_firinterp_##K *out);      \
    int yagi_hip_firinterp_##K##_set_stream(yagi_hip_firinterp_##K q, yagi_stream_t s);             \
    int yagi_hip_firinterp_##K##_reset(yagi_hip_firinterp_##K q);                                   \
    int yagi_hip_firinterp_##K##_get_interp_rate(yagi_hip_firinterp_##K q, size_t *interp);         \
    int yagi_hip_firinterp_##K##_get_sub_len(yagi_hip_firinterp_##K q, size_t *h_sub_len);          \
    int yagi_hip_firinterp_##K##_set_scale(yagi_hip_firinterp_##K q, C scale);                      \
    int yagi_hip_firinterp_##K##_get_scale(yagi_hip_firinterp_##K q, C *scale);                     \
    int yagi_hip_firinterp_##K##_execute(yagi_hip_firinterp_##K q, T x, T *y, size_t ny);           \
    int yagi_hip_firinterp_##K##_execute_block(yagi_hip_firinterp_##K q, const T *x, size_t nx,     \
                                               T *y, size_t ny);                                    \
    int yagi_hip_firinterp_##K##_execute_block_dev(yagi_hip_firinterp_##K q, const T *x_dev,        \
                                                   size_t n, T *y_dev);                             \
    int yagi_hip_firinterp_##K##_flush(yagi_hip_firinterp_##K q, T *y, size_t ny);

YAGI_FIRINTERP_API(rrrf, float, float)
YAGI_FIRINTERP_API(crcf, yagi_cf32, float)
YAGI_FIRINTERP_API(cccf, yagi_cf32, yagi_cf32)

/* ---- Rresamp<T,Coeff>: src/filter/resampler/rresamp.rs:8-183 (rational-rate resampler P/Q) -----
 *   create          new(interp, decim, m, h)            :28-57   bank = FirPfbFilter::new(interp, h, 2*interp*m)
 *   create_kaiser   new_kaiser(interp, decim, m, bw, as) :59-82   rates reduced by their gcd (block_len = gcd),
 *                                                                bw < 0 picks the default, scale 2 bw sqrt(Q/P)
 *   create_default  new_default(interp, decim)           :99-104  m 12, bw 0.5, 60 dB
 *   reset / set_scale / get_scale                        :106-116
 *   get_params      get_interp / get_decim / get_delay (= m) / get_block_len  :118-148
 *                   (get_rate = P/Q, get_p = P*block_len, get_q = Q*block_len follow from them)
 *   write           write(buf)                           :150-152 pushes samples without producing output
 *   execute         execute(x, y)                        :154-161 Q*block_len inputs -> P*block_len outputs
 *   execute_block   execute_block(x, n, y)               :163-170 n times execute.  (For block_len > 1 the
 *                   reference slices x and y by Q and P here and panics inside execute; this engine advances
 *                   by Q*block_len and P*block_len like liquid-dsp's rresamp_execute_block.)
 *   new_prototype (:84-97) is not provided: create() with the taps of yagi_hip_fir_design_prototype and its scale.
 * Device form: rresamp_kernel -- the branch schedule is static (output n of a block = branch (nQ) mod P after
 * input floor(nQ/P)), so every output is an independent 2m-tap dot product. */
#define YAGI_RRESAMP_API(K, T, C)                                                                   \
    typedef struct yagi_hip_rresamp_##K##_s *yagi_hip_rresamp_##K;                                  \
    int yagi_hip_rresamp_##K##_create(size_t interp, size_t decim, size_t m, const C *h,            \
                                      size_t h_len, yagi_hip_rresamp_##K *q);                       \
    int yagi_hip_rresamp_##K##_create_kaiser(size_t interp, size_t decim, size_t m, float bw,       \
                                             float as_, yagi_hip_rresamp_##K *q);                   \
    int yagi_hip_rresamp_##K##_create_default(size_t interp, size_t decim, yagi_hip_rresamp_##K *q);\
    int yagi_hip_rresamp_##K##_destroy(yagi_hip_rresamp_##K q);                                     \
    int yagi_hip_rresamp_##K##_clone(yagi_hip_rresamp_##K q, yagi_hip_rresamp_##K *out); /* derive(Clone) :8 */ \
    int yagi_hip_rresamp_##K##_set_stream(yagi_hip_rresamp_##K q, yagi_stream_t s);                 \
    int yagi_hip_rresamp_##K##_reset(yagi_hip_rresamp_##K q);                                       \
    int yagi_hip_rresamp_##K##_set_scale(yagi_hip_rresamp_##K q, C scale);                          \
    int yagi_hip_rresamp_##K##_get_scale(yagi_hip_rresamp_##K q, C *scale);                         \
    int yagi_hip_rresamp_##K##_get_params(yagi_hip_rresamp_##K q, size_t *interp, size_t *decim,    \
                                          size_t *m, size_t *block_len);                            \
    int yagi_hip_rresamp_##K##_write(yagi_hip_rresamp_##K q, const T *x, size_t n);                 \
    int yagi_hip_rresamp_##K##_execute(yagi_hip_rresamp_##K q, const T *x, size_t nx, T *y,         \
                                       size_t ny);                                                  \
    int yagi_hip_rresamp_##K##_execute_block(yagi_hip_rresamp_##K q, const T *x, size_t nx,         \
                                             size_t n, T *y, size_t ny);                            \
    int yagi_hip_rresamp_##K##_execute_block_dev(yagi_hip_rresamp_##K q, const T *x_dev, size_t n,  \
                                                 T *y_dev);

YAGI_RRESAMP_API(rrrf, float, float)
YAGI_RRESAMP_API(crcf, yagi_cf32, float)
YAGI_RRESAMP_API(cccf, yagi_cf32, yagi_cf32)

/* ---- Resamp2<T,Coeff>: src/filter/resampler/resamp2.rs:26-180 (half-band filter / 2-channel bank / x2 resampler)
 *      MsResamp2<T,Coeff>: src/filter/resampler/msresamp2.rs:8-198 (2^S resampler = chain of half-band stages)
 *   create(hf, m, f0)        new(m, f0, as_) :44-88 FROM THE DESIGNED PROTOTYPE hf[4m+1]: the reference designs it with
 *                            fir_design_pm_halfband_stopband_attenuation (Parks-McClellan design code, outside the hot
 *                            path); everything after the design -- for_halfband modulation :9-23, the 2m branch taps
 *                            h1[i] = h[4m - 1 - 2i] :66-70, two 2m-sample windows, toggle -- is reproduced.
 *   create_kaiser(m, f0, as) the reference's signature with a Kaiser-windowed half-band prototype (kaiser(4m+1, 0.25, as))
 *   clone / reset / set_scale / get_scale / get_delay (= 2m - 1)                     :25,90-106
 *   execute_block[_dev](mode, x, nx, y, ny): nx input samples through one of the five forms, state carried across calls;
 *       ny = the length of y and must be the form's output count (YAGI_ERR_CONFIG otherwise: the reference's slices
 *       carry their lengths)
 *       mode 0 filter_execute       :108-130  nx samples  -> 2 nx outputs, (y0, y1) = (low, high) per sample
 *       mode 1 analyzer_execute     :132-143  nx/2 pairs  -> nx outputs,   (low, high) per pair
 *       mode 2 synthesizer_execute  :145-157  nx/2 pairs (low, high) -> nx outputs
 *       mode 3 decim_execute        :159-169  nx samples  -> nx/2 outputs
 *       mode 4 interp_execute       :171-180  nx samples  -> 2 nx outputs
 *     (modes 1-3 need an even nx.)  The per-call forms of the reference are these with nx = 1 or 2.
 *   msresamp2 create(interp, num_stages, fc, f0, as)  new() :38-93 with Kaiser half-band stages (stage plan :66-88:
 *                            estimate_req_filter_len, m = max(3, ceil((h_len - 1) / 4)), as + 5 dB)
 *   msresamp2 create_taps(interp, num_stages, m_stage, hf_all)  the same from externally designed stage prototypes
 *                            (hf_all = the stages' hf[4 m_s + 1] one after the other)
 *   msresamp2 execute_block[_dev](x, nx, y, ny)  n times execute() :137-152: interp nx = n -> ny = n 2^S, decim
 *                            nx = n 2^S -> ny = n (x 1/2^S); any other pair of lengths is YAGI_ERR_CONFIG (:181)
 *   msresamp2 get_params     get_type / get_num_stages / get_delay :95-135 (+ the stage semi-lengths) */
#define YAGI_RESAMP2_API(K, T, C)                                                                   \
    typedef struct yagi_hip_resamp2_##K##_s *yagi_hip_resamp2_##K;                                  \
    typedef struct yagi_hip_msresamp2_##K##_s *yagi_hip_msresamp2_##K;                              \
    int yagi_hip_resamp2_##K##_create(const float *hf, size_t m, float f0, yagi_hip_resamp2_##K *q);\
    int yagi_hip_resamp2_##K##_create_kaiser(size_t m, float f0, float as_, yagi_hip_resamp2_##K *q);\
    int yagi_hip_resamp2_##K##_destroy(yagi_hip_resamp2_##K q);                                     \
    int yagi_hip_resamp2_##K##_clone(yagi_hip_resamp2_##K q, yagi_hip_resamp2_##K *out);            \
    int yagi_hip_resamp2_##K##_reset(yagi_hip_resamp2_##K q);                                       \
    int yagi_hip_resamp2_##K##_set_stream(yagi_hip_resamp2_##K q, yagi_stream_t s);                 \
    int yagi_hip_resamp2_##K##_set_scale(yagi_hip_resamp2_##K q, C scale);                          \
    int yagi_hip_resamp2_##K##_get_scale(yagi_hip_resamp2_##K q, C *scale);                         \
    int yagi_hip_resamp2_##K##_get_delay(yagi_hip_resamp2_##K q, size_t *delay);                    \
    int yagi_hip_resamp2_##K##_execute_block(yagi_hip_resamp2_##K q, int mode, const T *x,          \
                                             size_t nx, T *y, size_t ny);                           \
    int yagi_hip_resamp2_##K##_execute_block_dev(yagi_hip_resamp2_##K q, int mode, const T *x_dev,  \
                                                 size_t nx, T *y_dev, size_t ny);                   \
    int yagi_hip_msresamp2_##K##_create(int interp, size_t num_stages, float fc, float f0,          \
                                        float as_, yagi_hip_msresamp2_##K *q);                      \
    int yagi_hip_msresamp2_##K##_create_taps(int interp, size_t num_stages, const size_t *m_stage,  \
                                             const float *hf_all, yagi_hip_msresamp2_##K *q);       \
    int yagi_hip_msresamp2_##K##_destroy(yagi_hip_msresamp2_##K q);                                 \
    int yagi_hip_msresamp2_##K##_clone(yagi_hip_msresamp2_##K q, yagi_hip_msresamp2_##K *out);      \
    int yagi_hip_msresamp2_##K##_reset(yagi_hip_msresamp2_##K q);                                   \
    int yagi_hip_msresamp2_##K##_set_stream(yagi_hip_msresamp2_##K q, yagi_stream_t s);             \
    int yagi_hip_msresamp2_##K##_get_params(yagi_hip_msresamp2_##K q, int *interp,                  \
                                            size_t *num_stages, float *delay, size_t *m_stage);     \
    int yagi_hip_msresamp2_##K##_execute_block(yagi_hip_msresamp2_##K q, const T *x, size_t nx,     \
                                               T *y, size_t ny);                                    \
    int yagi_hip_msresamp2_##K##_execute_block_dev(yagi_hip_msresamp2_##K q, const T *x_dev,        \
                                                   size_t nx, T *y_dev, size_t ny);

YAGI_RESAMP2_API(rrrf, float, float)
YAGI_RESAMP2_API(crcf, yagi_cf32, float)
YAGI_RESAMP2_API(cccf, yagi_cf32, yagi_cf32)

/* ---- Resamp<T,Coeff>: src/filter/resampler/resamp.rs:8-165 (arbitrary-rate resampler) ---------------------------
 *   create          new(rate, m, fc, as_, npfb)   :24-71   checks in the reference's order and wording; npfb is rounded
 *                   up to 2^bits (math/mod.rs:80-92, npfb 0 -> VALUE, bits outside [1,16] -> CONFIG); Kaiser design
 *                   of 2 m npfb + 1 taps at fc/npfb, normalised to DC gain npfb (sequential f32 sum), bank =
 *                   FirPfbFilter::new(npfb, h, 2 m npfb) (the last tap dropped, :56)
 *   create_default  new_default(rate)             :73-84   m 7, fc 0.25, 60 dB, npfb 256
 *   create_taps     the bank from external taps h[0 .. 2 m npfb) (npfb a power of two in [2, 2^16]); for exact tests
 *   clone / reset   derive(Clone) :8 / reset() :86-89 (phase 0, window zeroed)
 *   set_rate / adjust_rate / get_rate  :95-118     rate in [0.004, 250]; step = round(2^24 / rate) in f32
 *   get_delay       get_delay() :91-93 (= m)
 *   get_num_output  get_num_output(nx) :128-139   closed form, no device work
 *   execute         execute(x, y) :141-154        one sample in; *nw = the outputs written (ny_cap = y's length)
 *   execute_block   execute_block(x, y) :156-165  nx samples in
 *   ny_cap < get_num_output(nx) is YAGI_ERR_RANGE (the reference panics on the slice); y[*nw .. ny_cap) is not
 *   written.  Every path (host per-sample,
 *   host block, device block) leaves the same window and phase, so calls may be mixed.
 * Device form: resamp_kernel -- the control loop only adds integers, so with A_j = p0 + j step output j of a call
 * comes after input A_j >> 24 and uses branch (A_j & 0xFFFFFF) >> (24 - bits): every output is an independent 2m-tap
 * dot product and the host knows the output count before the launch.  symsync and the timing-phase setters (commented
 * out in the reference, :120-126) are not provided. */
#define YAGI_RESAMP_API(K, T, C)                                                                    \
    typedef struct yagi_hip_resamp_##K##_s *yagi_hip_resamp_##K;                                    \
    int yagi_hip_resamp_##K##_create(float rate, size_t m, float fc, float as_, size_t npfb,        \
                                     yagi_hip_resamp_##K *q);                                       \
    int yagi_hip_resamp_##K##_create_default(float rate, yagi_hip_resamp_##K *q);                   \
    int yagi_hip_resamp_##K##_create_taps(float rate, size_t m, size_t npfb, const C *h,            \
                                          size_t h_len, yagi_hip_resamp_##K *q);                    \
    int yagi_hip_resamp_##K##_destroy(yagi_hip_resamp_##K q);                                       \
    int yagi_hip_resamp_##K##_clone(yagi_hip_resamp_##K q, yagi_hip_resamp_##K *out);               \
    int yagi_hip_resamp_##K##_set_stream(yagi_hip_resamp_##K q, yagi_stream_t s);                   \
    int yagi_hip_resamp_##K##_reset(yagi_hip_resamp_##K q);                                         \
    int yagi_hip_resamp_##K##_set_rate(yagi_hip_resamp_##K q, float rate);                          \
    int yagi_hip_resamp_##K##_adjust_rate(yagi_hip_resamp_##K q, float gamma);                      \
    int yagi_hip_resamp_##K##_get_rate(yagi_hip_resamp_##K q, float *rate);                         \
    int yagi_hip_resamp_##K##_get_delay(yagi_hip_resamp_##K q, size_t *delay);                      \
    int yagi_hip_resamp_##K##_get_num_output(yagi_hip_resamp_##K q, size_t nx, size_t *ny);         \
    int yagi_hip_resamp_##K##_execute(yagi_hip_resamp_##K q, T x, T *y, size_t ny_cap, size_t *nw); \
    int yagi_hip_resamp_##K##_execute_block(yagi_hip_resamp_##K q, const T *x, size_t nx, T *y,     \
                                            size_t ny_cap, size_t *nw);                             \
    int yagi_hip_resamp_##K##_execute_block_dev(yagi_hip_resamp_##K q, const T *x_dev, size_t nx,   \
                                                T *y_dev, size_t ny_cap, size_t *nw);

YAGI_RESAMP_API(rrrf, float, float)
YAGI_RESAMP_API(crcf, yagi_cf32, float)
YAGI_RESAMP_API(cccf, yagi_cf32, yagi_cf32)

/* ---- MsResamp<T,Coeff>: src/filter/resampler/msresamp.rs:10-176 (multi-stage arbitrary-rate resampler) -----------
 *   create(rate, as_)   new() :28-79  rate > 1: interpolator, else decimator; S half-band stages bring the rest into
 *                       (1, 2] (interp) or [0.5, 1] (decim).  Built as MsResamp2 create(type, S, 0.4, 0.0, as_) -- the
 *                       Kaiser half-band stand-in for the reference's Parks-McClellan design, as documented at
 *                       MsResamp2 above (same structure, different tap values) -- and Resamp(rate_arbitrary, 7,
 *                       min(0.515 rate_arbitrary, 0.49), as_, 256).
 *   clone / reset       derive(Clone) :10 / reset() :81-85
 *   get_rate / get_delay  :105-107 / :87-103 (a float)
 *   get_params          type (1 = interp), number of half-band stages, the arbitrary rate
 *   get_num_output      :109-120
 *   execute[_dev]       execute(x, y) :122-176; interp: Resamp then the 2^S interpolator on its output; decim: the
 *                       half-band chain over groups of 2^S inputs (the 0 .. 2^S-1 left over are carried to the next
 *                       call), then Resamp.  *nw = outputs written; ny_cap < get_num_output(nx) is YAGI_ERR_RANGE.
 *                       The intermediate stream stays on the device. */
#define YAGI_MSRESAMP_API(K, T, C)                                                                  \
    typedef struct yagi_hip_msresamp_##K##_s *yagi_hip_msresamp_##K;                                \
    int yagi_hip_msresamp_##K##_create(float rate, float as_, yagi_hip_msresamp_##K *q);            \
    int yagi_hip_msresamp_##K##_destroy(yagi_hip_msresamp_##K q);                                   \
    int yagi_hip_msresamp_##K##_clone(yagi_hip_msresamp_##K q, yagi_hip_msresamp_##K *out);         \
    int yagi_hip_msresamp_##K##_set_stream(yagi_hip_msresamp_##K q, yagi_stream_t s);               \
    int yagi_hip_msresamp_##K##_reset(yagi_hip_msresamp_##K q);                                     \
    int yagi_hip_msresamp_##K##_get_rate(yagi_hip_msresamp_##K q, float *rate);                     \
    int yagi_hip_msresamp_##K##_get_delay(yagi_hip_msresamp_##K q, float *delay);                   \
    int yagi_hip_msresamp_##K##_get_params(yagi_hip_msresamp_##K q, int *interp,                    \
                                           size_t *num_halfband_stages, float *rate_arbitrary);     \
    int yagi_hip_msresamp_##K##_get_num_output(yagi_hip_msresamp_##K q, size_t nx, size_t *ny);     \
    int yagi_hip_msresamp_##K##_execute(yagi_hip_msresamp_##K q, const T *x, size_t nx, T *y,       \
                                        size_t ny_cap, size_t *nw);                                 \
    int yagi_hip_msresamp_##K##_execute_dev(yagi_hip_msresamp_##K q, const T *x_dev, size_t nx,     \
                                            T *y_dev, size_t ny_cap, size_t *nw);

YAGI_MSRESAMP_API(rrrf, float, float)
YAGI_MSRESAMP_API(crcf, yagi_cf32, float)
YAGI_MSRESAMP_API(cccf, yagi_cf32, yagi_cf32)

/* ---- IirFilter<T,Coeff>: src/filter/iir/iirfilt.rs:23-481, iirfiltsos.rs:1-127 (infinite impulse response filter) ---
 *   create(b, nb, a, na)      new() :65-100  transfer function, normalised by a[0] in f32; n = max(na, nb) <= 33 (a
 *                             config error beyond: f32 TF filters are unusable past about 8 coefficients, :53-56).
 *                             na != nb: the shorter vector is zero-padded to n (the reference panics there).
 *   create_sos(b, a, nsos)    new_sos() :111-137  b, a = [nsos][3], each section normalised by its own a0; any nsos
 *   create_dc_blocker(alpha)  :290-305    create_integrator / create_differentiator :204-288 (Pintelon 8th order, 4
 *                             sections through iir_design_d2sos)    create_pll(w, zeta, k) :310-330 (active lag)
 *   clone / reset             derive(Clone) (the copy's VecDeque is contiguous: head 0) / reset() :333-343
 *   set_scale / get_scale / get_length  (n for TF, 2 nsos for SOS)
 *   execute / execute_block   :385-407 (nx != ny is a config error); up to 32 host samples run on the host mirror of
 *                             the state in the reference's order, longer host blocks stage through the device
 *   execute_block_dev         asynchronous on the object's stream, no host synchronisation; the state stays on the
 *                             device.  All paths leave the same state, so calls may be mixed.
 *   freqresponse / get_psd / groupdelay  :416-480 on the host (iir_group_delay, design/mod.rs:771)
 * Device form: iir_kernels.hip -- chunked state scan with an f64 cross-chunk combine.
 * new_prototype / new_lowpass (Butterworth, Chebyshev, elliptic, Bessel design) are not provided. */
#define YAGI_IIRFILT_API(K, T, C)                                                                   \
    typedef struct yagi_hip_iirfilt_##K##_s *yagi_hip_iirfilt_##K;                                  \
    int yagi_hip_iirfilt_##K##_create(const C *b, size_t nb, const C *a, size_t na,                 \
                                      yagi_hip_iirfilt_##K *q);                                     \
    int yagi_hip_iirfilt_##K##_create_sos(const C *b, const C *a, size_t nsos, yagi_hip_iirfilt_##K *q); \
    int yagi_hip_iirfilt_##K##_create_dc_blocker(float alpha, yagi_hip_iirfilt_##K *q);             \
    int yagi_hip_iirfilt_##K##_create_integrator(yagi_hip_iirfilt_##K *q);                          \
    int yagi_hip_iirfilt_##K##_create_differentiator(yagi_hip_iirfilt_##K *q);                      \
    int yagi_hip_iirfilt_##K##_create_pll(float w, float zeta, float k, yagi_hip_iirfilt_##K *q);   \
    int yagi_hip_iirfilt_##K##_destroy(yagi_hip_iirfilt_##K q);                                     \
    int yagi_hip_iirfilt_##K##_clone(yagi_hip_iirfilt_##K q, yagi_hip_iirfilt_##K *out);            \
    int yagi_hip_iirfilt_##K##_set_stream(yagi_hip_iirfilt_##K q, yagi_stream_t s);                 \
    int yagi_hip_iirfilt_##K##_reset(yagi_hip_iirfilt_##K q);                                       \
    int yagi_hip_iirfilt_##K##_set_scale(yagi_hip_iirfilt_##K q, C scale);                          \
    int yagi_hip_iirfilt_##K##_get_scale(yagi_hip_iirfilt_##K q, C *scale);                         \
    int yagi_hip_iirfilt_##K##_get_length(yagi_hip_iirfilt_##K q, size_t *len);                     \
    int yagi_hip_iirfilt_##K##_execute(yagi_hip_iirfilt_##K q, T x, T *y);                          \
    int yagi_hip_iirfilt_##K##_execute_block(yagi_hip_iirfilt_##K q, const T *x, size_t nx, T *y,   \
                                             size_t ny);                                            \
    int yagi_hip_iirfilt_##K##_execute_block_dev(yagi_hip_iirfilt_##K q, const T *x_dev, size_t n,  \
                                                 T *y_dev);                                         \
    int yagi_hip_iirfilt_##K##_freqresponse(yagi_hip_iirfilt_##K q, float fc, yagi_cf32 *H);        \
    int yagi_hip_iirfilt_##K##_get_psd(yagi_hip_iirfilt_##K q, float fc, float *psd);               \
    int yagi_hip_iirfilt_##K##_groupdelay(yagi_hip_iirfilt_##K q, float fc, float *gd);

YAGI_IIRFILT_API(rrrf, float, float)
YAGI_IIRFILT_API(crcf, yagi_cf32, float)
YAGI_IIRFILT_API(cccf, yagi_cf32, yagi_cf32)

/* Which kernel execute_block uses.  0 = auto (always a direct form), 1 = general direct-form kernels
 * (fir_kernels.hip: register-window kernel for blocks >= 512 samples, interleaved-output kernel below; both add
 * the taps in the reference's order and never touch a tap past h_len, so a NaN poisons exactly h_len outputs),
 * 4 = overlap-save fast convolution (<= 2049 taps; stream_kernels.hip).
 * crcf also: 2 = hand-scheduled register-sliding direct form (<= 1024 taps; the crcf auto choice from 1024 samples
 * on), 3 = MFMA Toeplitz direct form (<= 256 taps; the crcf auto choice from 2^16 samples on).
 * Non-finite input (NaN, +-Inf at sample s; every set below is asserted exactly by tests/test_gpu_nonfinite.py, the
 * table is in DESIGN.md section 6):
 *   1 (and auto for rrrf / cccf, crcf below 1024 samples): outputs s .. s + h_len - 1, the reference's window.
 *   2: s .. s + Lp - 1, Lp = h_len rounded up to a multiple of 32 -- the kernel multiplies the zero-padded taps.
 *   3: the same with Lp = 64, 128 or 256 (the tap class of h_len).  No output before s: the Toeplitz operand holds
 *      zeros, not gaps, where a row's window does not reach, so a wave that finds a non-finite sample in its span
 *      runs the products with it zeroed and adds its terms to the outputs whose window holds it (stream_kernels.hip).
 *   2 and 3 within one call only: the state carried to the next call is the reference's h_len samples, and a call the
 *      auto choice sends to another kernel (e.g. a short call after a long one) has that kernel's footprint.
 *   4: whole overlap-save blocks.  Block k of a call makes outputs [kV, kV + V) of the call from the samples
 *      [kV - P0, kV + V), V = 4096 - (h_len - 1) rounded down to a multiple of 16 (rrrf: 32), P0 = 4096 - V; every
 *      block whose samples hold s is non-finite throughout; rrrf transforms blocks 2w and 2w + 1 together, so they are
 *      poisoned together.  FftFilt with h_len <= 2049 is this kernel over the nblocks * n samples of the call.
 * Outside these sets every output equals the clean stream's bit for bit, and reset() clears the window.
 * The direct forms evaluate the reference's sums (exact on integer-valued data); the fast convolution agrees
 * with them to f32 rounding (rel. L2 <= 2e-6 against the f64 truth), like the reference's own FftFilt, and is
 * 2.5x (rrrf, crcf; 256 taps) to 5x (cccf, 256 taps) faster on long blocks, a tie for short filters (63 taps). */
int yagi_hip_firfilt_rrrf_set_kernel(yagi_hip_firfilt_rrrf q, int choice);
int yagi_hip_firfilt_crcf_set_kernel(yagi_hip_firfilt_crcf q, int choice);
int yagi_hip_firfilt_cccf_set_kernel(yagi_hip_firfilt_cccf q, int choice);

/* ---- plan queries (diagnostics, like get_last_kernel: no reference counterpart) -----------------------------------
 * What a block call of the FIR family would launch for a shape, answered by the very planner the launch calls.  Read-
 * only host arithmetic: no device is needed or initialised, and YAGI_HIP_DECIM_WINDOW_MIN_STEPS is honoured as by the
 * launch.  elem / coeff_elem = bytes per sample / per tap: 4 (real) or 8 (complex), so rrrf = (4, 4), crcf = (8, 4),
 * cccf = (8, 8).  A bad argument is YAGI_ERR_CONFIG.  These describe the present kernels and may change with them.
 *
 *   plan_fir_block(elem, L, M, ny)        FirFilter kernel 1 (M = 1), FirDecimationFilter and Ddc's fused kernel: a
 *                                         call of ny outputs, L taps, decimation M.  kind = YAGI_PLAN_FIR_*; DECIM
 *                                         also sets nt (lanes per workgroup), r (outputs per lane) and staging
 *                                         (YAGI_PLAN_STAGE_*, how a tile that lies wholly inside the call's input is
 *                                         staged; tiles that touch the carried window or the end of the call stage
 *                                         entry by entry).  tile = outputs per workgroup.
 *   plan_firpfb_all(elem, coeff_elem, nf, Ls)   FirPfbFilter execute_all_dev, FirInterpolationFilter and Duc: nf
 *                                         branches of Ls taps.  kind = YAGI_PLAN_PFB_*; tile = inputs per workgroup,
 *                                         0 with YAGI_PLAN_PFB_NONE (the call itself returns YAGI_ERR_CONFIG).
 *   plan_rresamp(elem, P, Q, Ls)          Rresamp: tile = primitive blocks (Q in, P out) per workgroup; YAGI_ERR_CONFIG
 *                                         where the block call returns it (one block's span does not fit the LDS).
 *   plan_resamp(elem, Ls, step)           Resamp: tile = outputs per workgroup for the 8.24 fixed-point step
 *                                         round(2^24 / rate); YAGI_ERR_CONFIG where Ls + 1 samples do not fit.
 *   lds = the launch's dynamic LDS in bytes (Ddc / Duc add the oscillator table behind it).
 *   *_range: the same for `count` consecutive tap counts from L0 / Ls0 on into out[0 .. count); a shape that does not
 *   fit is reported as tile = 0, never as an error. */
#define YAGI_PLAN_FIR_CONSEC 0    /* M = 1 register-window kernel */
#define YAGI_PLAN_FIR_DECIM 1     /* per-phase register-window decimator <nt, r> */
#define YAGI_PLAN_FIR_STAGED 2    /* general kernel, span of `tile` outputs staged in LDS */
#define YAGI_PLAN_FIR_UNSTAGED 3  /* general kernel reading the stream from L2 / HBM */
#define YAGI_PLAN_PFB_FEW 0          /* <= 16 branches: a lane per input sample */
#define YAGI_PLAN_PFB_TAPS_LDS 1     /* a lane per (sample, branch), taps transposed in LDS */
#define YAGI_PLAN_PFB_TAPS_GLOBAL 2  /* the same, taps read from L1 / L2 */
#define YAGI_PLAN_PFB_NONE 3
#define YAGI_PLAN_STAGE_ELEMENT 0
#define YAGI_PLAN_STAGE_DESCRIPTOR 1
#define YAGI_PLAN_STAGE_POW2 2
typedef struct {
    int kind, nt, r, tile, staging;
    size_t lds;
} yagi_hip_plan;
int yagi_hip_plan_fir_block(size_t elem, size_t L, size_t M, size_t ny, yagi_hip_plan *out);
int yagi_hip_plan_firpfb_all(size_t elem, size_t coeff_elem, size_t nf, size_t Ls, yagi_hip_plan *out);
int yagi_hip_plan_rresamp(size_t elem, size_t P, size_t Q, size_t Ls, yagi_hip_plan *out);
int yagi_hip_plan_resamp(size_t elem, size_t Ls, uint32_t step, yagi_hip_plan *out);
int yagi_hip_plan_fir_block_range(size_t elem, size_t L0, size_t count, size_t M, size_t ny, yagi_hip_plan *out);
int yagi_hip_plan_firpfb_all_range(size_t elem, size_t coeff_elem, size_t nf, size_t Ls0, size_t count, yagi_hip_plan *out);
int yagi_hip_plan_rresamp_range(size_t elem, size_t P, size_t Q, size_t Ls0, size_t count, yagi_hip_plan *out);
int yagi_hip_plan_resamp_range(size_t elem, size_t Ls0, size_t count, uint32_t step, yagi_hip_plan *out);

/* What a Spgram write of `nframes` transforms (2 <= nfft <= 2^20, 1 <= nframes < 2^31) would launch, answered by the
 * functions the launch itself calls; no device is needed.  A call is cut into launches of at most launch_frames
 * transforms; the other fields describe the first launch, of min(nframes, launch_frames) transforms.
 *   fused = 1 (nfft in {256, 512, 1024, 2048, 4096}): one kernel tapers, transforms and accumulates.  group = frames
 *           transformed together (4096 / nfft), slab = consecutive transforms per workgroup (a multiple of group),
 *           rows = workgroups * group partial rows of nfft floats; folded = 1 when the rows are first summed 32 to 1
 *           into fold_rows rows (rows > 64).  launch_frames = 2^20, accum_slab = 0.
 *   fused = 0: frame builder, batched FFT, two-stage accumulation.  workgroups = the frame builder's grid (it strides
 *           beyond 8192 workgroups), accum_slab = frames per Horner slab (32), rows = slabs, group = 1, slab = 0,
 *           launch_frames = 2^25 / nfft clamped to [1, 8192]. */
typedef struct {
    int fused, group, slab, workgroups, rows, folded, fold_rows, accum_slab;
    size_t launch_frames;
} yagi_hip_spgram_plan;
int yagi_hip_plan_spgram(size_t nfft, size_t nframes, yagi_hip_spgram_plan *out);

/* What a block call of the half-band family would launch, answered by the very planners the launches call
 * (resamp2_kernels.hip).  Read-only host arithmetic: no device is needed or initialised.  elem = bytes per sample, 4
 * (rrrf) or 8 (crcf, cccf); a bad argument is YAGI_ERR_CONFIG.  These describe the present kernels and may change with
 * them.
 *
 *   plan_msresamp2(elem, interp, ns, m, n)   MsResamp2 execute_block of n execute() calls (decimator: n outputs,
 *       interpolator: n inputs).  m[0 .. ns) in the OBJECT's stage order, as get_stage_lengths returns it: the
 *       interpolator runs stage 0 first, the decimator runs stage ns - 1 first, so stage g of the object is processing
 *       stage ns - 1 - g of the decimator kernels; n[], walk[] and walk_q[] below are in processing order (0 = the
 *       stage at the full rate).
 *       fused = 1: the chain in one launch (at most four stages whose streams fit lds <= 64 KiB); fused = 0: one
 *       Resamp2 block call per stage (plan_resamp2 answers for each), every other field but lds is 0, and lds too
 *       beyond four stages.
 *       Interpolator: tiles workgroups of 256 inputs, tpw = 1.
 *       Decimator: the general kernel runs `tiles` tiles of 256 outputs, tpw consecutive ones per workgroup, over the
 *       outputs [0, 256 head_tiles) and [tail_first, n); with fast_tiles > 0 the fast kernel runs fast_tiles tiles of F
 *       outputs from 256 head_tiles on, fast_tpw per workgroup, with fast_lds bytes.  F, n[k] (outputs of stage k per
 *       fast tile), cnt0 (input pairs per tile) and U (a tile's first input pair = 2^(ns-1) first output - U) describe
 *       the geometry whenever one with F >= 64 exists (ns <= 3), else F = 0.  walk[k] = YAGI_PLAN_WALK_*: how the
 *       fast kernel walks stage k's taps -- R outputs per lane with 2 m_k = R Q + RHO -- and walk_q[k] = Q (Q = 1:
 *       the walk has no full group).  long_halo = 1: a general tile's full-rate streams, 256 * 2^(ns-1) pairs and a
 *       halo, outgrow the 256 (2^(ns-1) + 1) entries a workgroup loads through registers (a halo of more than 256
 *       pairs), and the kernel instance that stages the rest from memory runs.
 *   plan_resamp2(elem, mode, m, nx)          Resamp2 execute_block of nx samples in form `mode` (0 filter .. 4 interp).
 *       chain = 0: resamp2_kernel, tiles workgroups of 1024 units with lds bytes; chain = 1: a long decimator block
 *       as the one-stage case of the chain kernels, what plan_msresamp2(elem, 0, 1, &m, nx / 2) describes (tiles and
 *       lds are its general kernel's). */
#define YAGI_PLAN_WALK_GENERAL 0  /* general kernel only: one tap chain per output */
#define YAGI_PLAN_WALK_R1 1       /* fast kernel, one output per lane */
#define YAGI_PLAN_WALK_R2 2       /* two outputs per lane, RHO = 0 */
#define YAGI_PLAN_WALK_R4_RHO0 3  /* four outputs per lane, m even */
#define YAGI_PLAN_WALK_R4_RHO2 4  /* four outputs per lane, m odd */
typedef struct {
    int fused, tpw, fast_tpw, F, n[3], cnt0, U, walk[4], walk_q[4], long_halo;
    size_t lds, fast_lds, head_tiles, fast_tiles, tail_first, tiles;
} yagi_hip_msresamp2_plan;
typedef struct {
    int chain;
    size_t tiles, lds;
} yagi_hip_resamp2_plan;
int yagi_hip_plan_msresamp2(size_t elem, int interp, size_t ns, const size_t *m, size_t n, yagi_hip_msresamp2_plan *out);
int yagi_hip_plan_resamp2(size_t elem, int mode, size_t m, size_t nx, yagi_hip_resamp2_plan *out);

/* ---- Fft<f32>: src/fft/mod.rs:33-69 (arithmetic = rustfft 6.2 in the reference) ------------
 *   create       Fft::new(n, direction)        :39-43   any n >= 1 the engine supports
 *   run          run(input, output)            :45-48   out of place, unnormalised,
 *                                                       forward = e^{-j 2 pi n k / N}
 *   run_batch_dev  `batch` contiguous transforms, device pointers (config C3)
 *   shift        shift(input, n)               :50-57   swap halves (odd n: last stays)
 *   fft_run      fft_run(input, output, dir)   :66-69   plan + run in one call
 * Sizes: every n up to 2^23, powers of two up to 2^24.  Powers of two 256..8192: register kernels (one HBM
 * round trip); other n <= 8192: mixed-radix Stockham passes in LDS (register butterflies for 2/3/4/5/7/8/16,
 * direct sums for other primes up to 89); n > 8192 that splits as n1 n2 with both factors <= 8192 and 89-smooth
 * (every power of two, 10000, 48000, ...): four-step form (three transposes around the sub-transforms);
 * everything else -- a prime factor > 89 -- Bluestein's chirp-z form over a power of two.  Larger n returns CONFIG.  Plans with scratch (Bluestein,
 * four-step) are not safe for concurrent run() calls on one handle. */
typedef struct yagi_hip_fft_s *yagi_hip_fft;
int yagi_hip_fft_create(size_t n, int direction, yagi_hip_fft *plan);
int yagi_hip_fft_destroy(yagi_hip_fft plan);
int yagi_hip_fft_clone(yagi_hip_fft plan, yagi_hip_fft *out);
int yagi_hip_fft_len(yagi_hip_fft plan, size_t *n);
int yagi_hip_fft_run(yagi_hip_fft plan, const yagi_cf32 *input, size_t n_in, yagi_cf32 *output,
                     size_t n_out);
int yagi_hip_fft_run_batch_dev(yagi_hip_fft plan, const yagi_cf32 *in_dev, yagi_cf32 *out_dev,
                               size_t batch, yagi_stream_t s);
int yagi_hip_fft_shift(yagi_cf32 *buf, size_t n);
int yagi_hip_fft_shift_dev(yagi_cf32 *buf_dev, size_t n, size_t batch, yagi_stream_t s);
int yagi_hip_fft_run_oneshot(const yagi_cf32 *input, yagi_cf32 *output, size_t n, int direction);

/* describe: which form run / run_batch_dev take for this plan and how they cut a batch (read-only; the values come from
 * the plan fields and the predicate the dispatch itself uses, so a test can say which loop it drove):
 *   path         the form of the transform
 *   batch_chunk  transforms per pass of that form's outer loop over its scratch; 0 = one launch whatever the batch
 *   n1, n2       the split n = n1 n2 of two_pass / tile256 / mixed_two_pass / four_step, else 0
 *   bluestein_m  the power-of-two convolution length of bluestein / bluestein_fused, else 0
 *   nested_*     the plan that form hands its sub-transforms to through the same dispatch: the m-point plan of
 *                bluestein, the n2-point plan of tile256 (n2 > 256) and four_step; nested_n = 0 where there is none */
typedef enum {
    YAGI_FFT_PATH_ONE_KERNEL = 0,       /* n <= 8192: one launch, one HBM round trip */
    YAGI_FFT_PATH_BLUESTEIN_FUSED = 1,  /* chirp-z over m = 4096 / 8192 in one kernel */
    YAGI_FFT_PATH_BLUESTEIN = 2,        /* chirp-z in five stages over the scratch */
    YAGI_FFT_PATH_TWO_PASS = 3,         /* 2^14, 2^15: column / row launches */
    YAGI_FFT_PATH_TILE256 = 4,          /* powers of two from 2^16: 256 x n2 */
    YAGI_FFT_PATH_MIXED_TWO_PASS = 5,   /* n1 n2, both factors <= 1024: column / row launches */
    YAGI_FFT_PATH_FOUR_STEP = 6         /* n1 n2, transposes around the sub-transforms */
} yagi_hip_fft_path;
typedef struct {
    int path;                           /* yagi_hip_fft_path */
    size_t batch_chunk;
    size_t n1, n2;
    size_t bluestein_m;
    size_t nested_n;
    int nested_path;
    size_t nested_batch_chunk;
} yagi_hip_fft_info;
int yagi_hip_fft_describe(yagi_hip_fft plan, yagi_hip_fft_info *info);

/* ---- Spgram<T>: src/fft/spgram.rs (Welch spectral periodogram; the in-tree consumer of window -> FFT) ----
 *   spgramcf = Spgram<Complex32>, spgramf = Spgram<f32>.
 *   create          new(nfft, wtype, window_len, delay)   :49-125  (nfft < 2, window_len > nfft, window_len == 0,
 *                                                                   delay == 0, Kaiser with odd window_len -> CONFIG;
 *                                                                   additionally nfft <= 8192 in this engine)
 *   create_default  default(nfft) = new(nfft, Kaiser, nfft/2, nfft/4)   :128-131
 *   clear / reset                                          :135-155
 *   set_alpha / get_alpha   (-1 = accumulate, else [0,1])  :158-174,229
 *   set_freq / set_rate / get_nfft / get_window_len / get_delay / get_wtype / counters   :177-226
 *   push / write    one transform every `delay` samples    :237-259  (write = the batched device form)
 *   get_psd_mag / get_psd   fft-shifted linear / dB        :292-316  (like the reference, the linear scale
 *                                                                   factor is 0 unless alpha == -1)
 *   Non-finite input: a sample inside a transform's window (the window_len samples that end at a multiple of
 *   `delay`) poisons every bin of the PSD until clear() / reset(); one that no window covers (delay > window_len)
 *   changes nothing.  As in the reference, max(psd, 1e-12) drops a NaN operand: a NaN bin reads as the floor
 *   1e-12 * scale, an infinite one as +Inf (tests/test_gpu_nonfinite.py).
 *   estimate_psd    one-shot                               :319-330
 * wtype uses the reference's WindowType discriminants (math/windows.rs:7-18). */
#define YAGI_WINDOW_HAMMING 1
#define YAGI_WINDOW_HANN 2
#define YAGI_WINDOW_BLACKMANHARRIS 3
#define YAGI_WINDOW_BLACKMANHARRIS7 4
#define YAGI_WINDOW_KAISER 5
#define YAGI_WINDOW_FLATTOP 6
#define YAGI_WINDOW_TRIANGULAR 7
#define YAGI_WINDOW_RCOSTAPER 8
#define YAGI_WINDOW_KBD 9
#define YAGI_SPGRAM_API(K, T)                                                                       \
    typedef struct yagi_hip_spgram##K##_s *yagi_hip_spgram##K;                                      \
    int yagi_hip_spgram##K##_create(size_t nfft, int wtype, size_t window_len, size_t delay,        \
                                    yagi_hip_spgram##K *q);                                         \
    int yagi_hip_spgram##K##_create_default(size_t nfft, yagi_hip_spgram##K *q);                    \
    int yagi_hip_spgram##K##_destroy(yagi_hip_spgram##K q);                                         \
    int yagi_hip_spgram##K##_set_stream(yagi_hip_spgram##K q, yagi_stream_t s);                     \
    int yagi_hip_spgram##K##_clear(yagi_hip_spgram##K q);                                           \
    int yagi_hip_spgram##K##_reset(yagi_hip_spgram##K q);                                           \
    int yagi_hip_spgram##K##_set_alpha(yagi_hip_spgram##K q, float alpha);                          \
    int yagi_hip_spgram##K##_get_alpha(yagi_hip_spgram##K q, float *alpha);                         \
    int yagi_hip_spgram##K##_set_freq(yagi_hip_spgram##K q, float freq);                            \
    int yagi_hip_spgram##K##_set_rate(yagi_hip_spgram##K q, float rate);                            \
    int yagi_hip_spgram##K##_get_params(yagi_hip_spgram##K q, size_t *nfft, size_t *window_len,     \
                                        size_t *delay, int *wtype);                                 \
    int yagi_hip_spgram##K##_get_counters(yagi_hip_spgram##K q, uint64_t *num_samples,              \
                                          uint64_t *num_samples_total, uint64_t *num_transforms,    \
                                          uint64_t *num_transforms_total);                          \
    int yagi_hip_spgram##K##_push(yagi_hip_spgram##K q, T x);                                       \
    int yagi_hip_spgram##K##_write(yagi_hip_spgram##K q, const T *x, size_t n);                     \
    int yagi_hip_spgram##K##_write_dev(yagi_hip_spgram##K q, const T *x_dev, size_t n);             \
    int yagi_hip_spgram##K##_get_psd_mag(yagi_hip_spgram##K q, float *psd, size_t n);               \
    int yagi_hip_spgram##K##_get_psd(yagi_hip_spgram##K q, float *psd, size_t n);                   \
    int yagi_hip_spgram##K##_estimate_psd(size_t nfft, const T *x, size_t n, float *psd);

YAGI_SPGRAM_API(cf, yagi_cf32)
YAGI_SPGRAM_API(f, float)

/* ---- the headline stream: FirFilter<Complex32,f32>::execute_block
 * (firfilt.rs:267-278) feeding consecutive nfft-sample frames to Fft::run forward
 * (fft/mod.rs:45-48).  1..2049 taps; nfft = 4096 is fused so the FIR output never touches HBM, any other nfft the
 * Fft object supports runs as overlap-save FIR + batched transform (two launches).  Filter state carries across
 * calls exactly like the FirFilter object's. */
typedef struct yagi_hip_firfft_crcf_s *yagi_hip_firfft_crcf;
int yagi_hip_firfft_crcf_create(const float *h, size_t h_len, size_t nfft, yagi_hip_firfft_crcf *q);
int yagi_hip_firfft_crcf_destroy(yagi_hip_firfft_crcf q);
int yagi_hip_firfft_crcf_set_stream(yagi_hip_firfft_crcf q, yagi_stream_t s);
int yagi_hip_firfft_crcf_set_scale(yagi_hip_firfft_crcf q, float scale);
int yagi_hip_firfft_crcf_reset(yagi_hip_firfft_crcf q);
/* variant: 0 = auto (4 up to 257 taps, 3 up to 2049 taps),
 *   1 = fused direct form, register-sliding VALU FIR (<= 1024 taps),
 *   2 = fused direct form, MFMA Toeplitz FIR (<= 256 taps),
 *   3 = fast convolution (overlap-save kernel, then batched FFT; <= 2049 taps),
 *   4 = frequency-domain filter, one launch: FFT{h}.FFT{frame} + FFT{frame-boundary correction} (<= 257 taps).
 * All variants carry the same filter state and agree to f32 rounding (rel. L2 <= 1e-5 per frame against the
 * f64 truth); only 1 and 2 evaluate the FIR sums themselves.
 * Non-finite input at sample s: a frame is non-finite throughout or untouched.  0 and 4: the frame holding s, and the
 * next one if s is among its last h_len - 1 samples (the reference's frames).  1, 2, 3 and nfft != 4096: the frames
 * holding an output of the footprint of FirFilter kernel 2, 3, 4 (set_kernel above); never a frame before the one
 * holding s.  tests/test_gpu_nonfinite.py::test_firfftstream_4096_which_frames, DESIGN.md section 6. */
int yagi_hip_firfft_crcf_set_variant(yagi_hip_firfft_crcf q, int variant);
int yagi_hip_firfft_crcf_execute(yagi_hip_firfft_crcf q, const yagi_cf32 *x, size_t nframes,
                                 yagi_cf32 *spectra);
int yagi_hip_firfft_crcf_execute_dev(yagi_hip_firfft_crcf q, const yagi_cf32 *x_dev,
                                     size_t nframes, yagi_cf32 *spectra_dev);
/* Pipelined block calls (frequency-domain form, nfft = 4096).  Consecutive blocks of the stream depend on each other
 * only through the L-sample filter window (firfilt.rs:13,220-223), and that window is the previous block's own last L
 * INPUT samples.  With the pipeline on, execute_dev runs consecutive blocks alternately on two streams owned by the
 * object, block b + 1 reading its window straight from the tail of block b's x_dev, so block b + 1 ramps up while
 * block b drains.  The contract changes in one point: x_dev must be complete on the object's stream when execute_dev
 * is called (as before), but spectra_dev -- and the right to overwrite or free x_dev -- is ordered on the object's
 * stream only after yagi_hip_firfft_crcf_join (stream waits + a 2 KiB window copy, no host synchronisation).  Every
 * other entry point of the object joins first; results are bit-identical to the unpipelined calls. */
int yagi_hip_firfft_crcf_set_pipeline(yagi_hip_firfft_crcf q, int on);
int yagi_hip_firfft_crcf_join(yagi_hip_firfft_crcf q);

/* ---- multichannel::firpfbch / firpfbch2 analyzers ------------------------------------------
 * ABSENT from the reference (src/multichannel/mod.rs is 0 lines; LIQUID_COMPAT.md:1765-1798).
 * Semantics are liquid-dsp's (the library yagi rewrites), composed from the reference's own
 * primitives: FirPfb-style branch split (firpfb.rs:45-52), Window (window.rs), dotprod, Fft.
 *   firpfbch  analyzer: M channels, p taps/branch, prototype h[0 .. p*M); one frame = M input
 *             samples -> M channel outputs: X[M-1-i] = branch_i . window_i ; y = DFT_M(X).
 *             create_kaiser(M, m, as_): h = kaiser(2*M*m+1, 0.5/M, as_), p = 2*m.
 *   firpfbch  synthesizer: one frame = M channel samples -> M output samples:
 *             v = IDFT_M(X) (unnormalised); branch i pushes v[i] and y[i] = branch_i . window_i, i.e.
 *             y[f M + i] = sum_n h[i + n M] v_{f-n}[i].  Own state, reset() clears both.
 *   firpfbch2 synthesizer: one step = M channel samples -> M/2 outputs; v_s = IDFT_M(X_s)/2, f = step parity, b = i + f M/2:
 *             y[s M/2 + i] = sum_n h[i + n M] v_{s-2n}[b] + sum_n h[i + M/2 + n M] v_{s-1-2n}[b].  With the analyzer's
 *             create_kaiser (cutoff 1/M) and create_kaiser_synthesizer (cutoff 0.5/M) prototypes the round trip
 *             reproduces the input delayed by 2 M m - M/2 + 1 samples (-60 dB at m = 3).
 *   firpfbch2 analyzer (2x oversampled): M even, branch length 2*m, h[0 .. 2*M*m); one step =
 *             M/2 inputs -> M outputs, alternating half rotation, y = IDFT_M(X)/M.
 *             create_kaiser(M, m, as_): h = kaiser(2*M*m+1, 1/M, as_) * M / sum(h).
 * Non-finite input in frame / step f: the reference window is frames f .. f+p-1 (firpfbch2: steps f .. f+4m-1), every
 * channel of them.  Calls of >= 64 frames / steps with M a power of two in 8 .. 256 (analyzers also M 512, 1024 with
 * p <= 8) run kernels built for P = 4 / 8 / 16 taps per branch (firpfbch2 analyzer: 2 / 4 / 8 / 16) with zero taps behind
 * the p real ones: f .. f+P-1, steps f .. f+2P-1; the firpfbch2 synthesizer a ring of 8 (m <= 2) or 16 lags:
 * f .. f+7 / f+15.  Within the call; the carried history is the reference's.  Other shapes keep the reference window.
 * tests/test_gpu_nonfinite.py::test_firpfbch, test_firpfbch2; DESIGN.md section 6.
 * Output layout [frame][channel].  The `_shard_dev` form computes only the sub-bands
 * k = rank + nranks*q (q < M/nranks) into yshard[step][q] so an 8-GPU node can all-gather them
 * (RCCL) -- see INTEGRATION.md; `assemble_dev` permutes the gathered [rank][step][q] slabs into
 * [step][channel]. */
typedef struct yagi_hip_firpfbch_crcf_s *yagi_hip_firpfbch_crcf;
int yagi_hip_firpfbch_crcf_create(size_t M, size_t p, const float *h, yagi_hip_firpfbch_crcf *q);
int yagi_hip_firpfbch_crcf_create_kaiser(size_t M, size_t m, float as_, yagi_hip_firpfbch_crcf *q);
int yagi_hip_firpfbch_crcf_destroy(yagi_hip_firpfbch_crcf q);
int yagi_hip_firpfbch_crcf_set_stream(yagi_hip_firpfbch_crcf q, yagi_stream_t s);
int yagi_hip_firpfbch_crcf_reset(yagi_hip_firpfbch_crcf q);
int yagi_hip_firpfbch_crcf_analyzer_execute(yagi_hip_firpfbch_crcf q, const yagi_cf32 *x,
                                            size_t nframes, yagi_cf32 *y);
int yagi_hip_firpfbch_crcf_analyzer_execute_dev(yagi_hip_firpfbch_crcf q, const yagi_cf32 *x_dev,
                                                size_t nframes, yagi_cf32 *y_dev);
int yagi_hip_firpfbch_crcf_synthesizer_execute(yagi_hip_firpfbch_crcf q, const yagi_cf32 *x,
                                               size_t nframes, yagi_cf32 *y);
int yagi_hip_firpfbch_crcf_synthesizer_execute_dev(yagi_hip_firpfbch_crcf q, const yagi_cf32 *x_dev,
                                                   size_t nframes, yagi_cf32 *y_dev);

typedef struct yagi_hip_firpfbch2_crcf_s *yagi_hip_firpfbch2_crcf;
int yagi_hip_firpfbch2_crcf_create(size_t M, size_t m, const float *h, yagi_hip_firpfbch2_crcf *q);
int yagi_hip_firpfbch2_crcf_create_kaiser(size_t M, size_t m, float as_, yagi_hip_firpfbch2_crcf *q);
/* prototype of the matching synthesizer: kaiser(2*M*m+1, 0.5/M, as_) * M / sum(h) */
int yagi_hip_firpfbch2_crcf_create_kaiser_synthesizer(size_t M, size_t m, float as_,
                                                      yagi_hip_firpfbch2_crcf *q);
int yagi_hip_firpfbch2_crcf_destroy(yagi_hip_firpfbch2_crcf q);
int yagi_hip_firpfbch2_crcf_set_stream(yagi_hip_firpfbch2_crcf q, yagi_stream_t s);
int yagi_hip_firpfbch2_crcf_reset(yagi_hip_firpfbch2_crcf q);
int yagi_hip_firpfbch2_crcf_analyzer_execute(yagi_hip_firpfbch2_crcf q, const yagi_cf32 *x,
                                             size_t nsteps, yagi_cf32 *y);
int yagi_hip_firpfbch2_crcf_analyzer_execute_dev(yagi_hip_firpfbch2_crcf q, const yagi_cf32 *x_dev,
                                                 size_t nsteps, yagi_cf32 *y_dev);
/* synthesizer: one step = M channel samples -> M/2 output samples (include note above); own state and step parity */
int yagi_hip_firpfbch2_crcf_synthesizer_execute(yagi_hip_firpfbch2_crcf q, const yagi_cf32 *x,
                                                size_t nsteps, yagi_cf32 *y);
int yagi_hip_firpfbch2_crcf_synthesizer_execute_dev(yagi_hip_firpfbch2_crcf q, const yagi_cf32 *x_dev,
                                                    size_t nsteps, yagi_cf32 *y_dev);
int yagi_hip_firpfbch2_crcf_analyzer_execute_shard_dev(yagi_hip_firpfbch2_crcf q,
                                                       const yagi_cf32 *x_dev, size_t nsteps,
                                                       int rank, int nranks, yagi_cf32 *yshard_dev);
int yagi_hip_firpfbch2_crcf_assemble_dev(const yagi_cf32 *gathered_dev, size_t nsteps, size_t M,
                                         int nranks, yagi_cf32 *y_dev, yagi_stream_t s);

/* ---- multichannel::firpfbchr: M channels spaced 1/M, one output per channel every P inputs --------------
 * Absent from the reference like the two above (firpfbch is P = M, firpfbch2 is P = M/2); defined by closed forms
 * ("FirPfbChr").  Real prototype h[0 .. 2*M*m), stream index t from 0, zero history, steps s = 0, 1, ...
 * counted from the start of the stream and carried across calls (reset() clears histories and both counters):
 *   analyzer:    one step = P inputs -> M outputs,
 *                y_s[k] = (1/M) sum_{l < 2Mm} h[l] x[(s+1)P - 1 - l] exp(+j 2 pi k (l - sP) / M)
 *   synthesizer: one step = M channel values -> P outputs,
 *                y[t] = (P/M) sum_{r >= 0, (t mod P) + rP < 2Mm} h[(t mod P) + rP] V_{floor(t/P) - r}[t mod M],
 *                V_s[b] = sum_k X_s[k] exp(+j 2 pi k b / M)
 *   create_kaiser: h = kaiser(2Mm+1, 0.5/P, as_) * M / sum(h); create_kaiser_synthesizer: kaiser(2Mm+1, 0.5/M, as_)
 *   * M / sum(h).  Analyzer then synthesizer returns the input delayed by 2Mm - P + 1 samples (-63 dB at M 16, P 12, m 8,
 *   As 60).
 * M >= 2, 1 <= P <= M, m >= 1, M <= 8192, m <= 2048, and a shape no launch can hold (M*m beyond the LDS) are
 * YAGI_ERR_CONFIG at create, decided before a device is required.  The synthesizer's history (ceil(2Mm/P) - 1 steps of
 * M values) is allocated by the first synthesizer call, which returns YAGI_ERR_CONFIG if it exceeds 2^23 values
 * (M 4096, P 1: 8191 steps); the analyzer of such an object works.
 * set_kernel: 0 auto, 1 the general analyzer kernel, 2 the column kernel (M in {64, 128, 256}, P a multiple of M/8,
 * 2m <= 16; YAGI_ERR_CONFIG elsewhere); get_last_kernel: 1 or 2, what the last analyzer call ran (0 before the first).
 * Non-finite input sample t: the general kernel poisons exactly the steps with 0 <= (s+1)P - 1 - t < 2Mm, every channel;
 * the column kernel, built for 4 / 8 / 16 taps per branch with zero taps behind the 2m real ones, the steps with
 * 0 <= (s+1)P - 1 - t < Pb*M within the call (the carried history is 2Mm - P samples).  A non-finite X_s[k] poisons
 * exactly the synthesizer outputs sP .. sP + 2Mm - 1.  tests/test_gpu_chanr_nonfinite.py.
 * The _dev forms take device pointers that must not overlap (YAGI_ERR_CONFIG) and run on the object's stream. */
typedef struct yagi_hip_firpfbchr_crcf_s *yagi_hip_firpfbchr_crcf;
int yagi_hip_firpfbchr_crcf_create(size_t M, size_t P, size_t m, const float *h, yagi_hip_firpfbchr_crcf *q);
int yagi_hip_firpfbchr_crcf_create_kaiser(size_t M, size_t P, size_t m, float as_, yagi_hip_firpfbchr_crcf *q);
int yagi_hip_firpfbchr_crcf_create_kaiser_synthesizer(size_t M, size_t P, size_t m, float as_,
                                                      yagi_hip_firpfbchr_crcf *q);
int yagi_hip_firpfbchr_crcf_destroy(yagi_hip_firpfbchr_crcf q);
int yagi_hip_firpfbchr_crcf_set_stream(yagi_hip_firpfbchr_crcf q, yagi_stream_t s);
int yagi_hip_firpfbchr_crcf_reset(yagi_hip_firpfbchr_crcf q);
int yagi_hip_firpfbchr_crcf_set_kernel(yagi_hip_firpfbchr_crcf q, int choice);
int yagi_hip_firpfbchr_crcf_get_last_kernel(yagi_hip_firpfbchr_crcf q, int *kernel);
int yagi_hip_firpfbchr_crcf_analyzer_execute(yagi_hip_firpfbchr_crcf q, const yagi_cf32 *x,
                                             size_t nsteps, yagi_cf32 *y);
int yagi_hip_firpfbchr_crcf_analyzer_execute_dev(yagi_hip_firpfbchr_crcf q, const yagi_cf32 *x_dev,
                                                 size_t nsteps, yagi_cf32 *y_dev);
int yagi_hip_firpfbchr_crcf_synthesizer_execute(yagi_hip_firpfbchr_crcf q, const yagi_cf32 *x,
                                                size_t nsteps, yagi_cf32 *y);
int yagi_hip_firpfbchr_crcf_synthesizer_execute_dev(yagi_hip_firpfbchr_crcf q, const yagi_cf32 *x_dev,
                                                    size_t nsteps, yagi_cf32 *y_dev);

/* ---- multi-GPU: RCCL over xGMI (one process per GPU) ------------------------------------------
 * The reference has no distributed layer; the one exchange step of the hot path is the
 * firpfbch2 analyzer with its output sub-bands sharded over the GPUs of a node.
 * A communicator is created the RCCL way: ONE rank calls comm_unique_id and hands the 128 bytes to every rank by
 * whatever the host has (MPI, a socket, torch.distributed); every rank then calls comm_create (collective) with
 * its GPU current (yagi_hip_set_device).  RCCL is bound at first use (dlopen of librccl.so.1); without it these
 * calls return YAGI_ERR_DEVICE and every other entry point of the library works unchanged.
 *
 * analyzer_execute_sharded_dev: rank r of R computes the sub-bands k = r + R q of `nsteps` steps (chunk by chunk),
 * the chunks are all-gathered on the communicator's own stream while the object's stream runs the next chunk's
 * kernel, and a permutation kernel assembles y[step][channel] -- identical on every rank, and identical to
 * analyzer_execute_dev on one GPU.  nchunks = 0 picks a default (8, fewer for short blocks); nchunks < 0 forces the
 * sharded pipeline (|nchunks| chunks) even for a one-rank communicator (tests).  x, y are device pointers; the
 * call is asynchronous: on return the object's stream waits for the last chunk's assembly. */
#define YAGI_HIP_COMM_ID_BYTES 128
typedef struct yagi_hip_comm_s *yagi_hip_comm;
int yagi_hip_comm_unique_id(unsigned char *id /* [YAGI_HIP_COMM_ID_BYTES] */);
int yagi_hip_comm_create(const unsigned char *id, int rank, int nranks, yagi_hip_comm *comm);
int yagi_hip_comm_destroy(yagi_hip_comm comm);
int yagi_hip_comm_rank(yagi_hip_comm comm, int *rank, int *nranks);
int yagi_hip_comm_all_gather_dev(yagi_hip_comm comm, const void *send_dev, void *recv_dev,
                                 size_t bytes_per_rank, yagi_stream_t s);
int yagi_hip_firpfbch2_crcf_analyzer_execute_sharded_dev(yagi_hip_firpfbch2_crcf q, const yagi_cf32 *x_dev,
                                                         size_t nsteps, yagi_hip_comm comm, int nchunks,
                                                         yagi_cf32 *y_dev);

/* ---- Osc: src/nco/osc.rs:13-201, nco.rs, vco.rs (numerically controlled / voltage-controlled oscillator) -------------
 *   create(scheme)            new() :37-57  YAGI_OSC_NCO (1024-entry sine table, nearest entry) or YAGI_OSC_VCO
 *                             (1024 {value, skew} pairs, linear interpolation); PLL bandwidth 0.1
 *   clone / reset             derive(Clone) / reset() :60-63 (theta = d_theta = 0; the PLL gains stay)
 *   set/adjust_frequency, set/adjust_phase   :66-83 through constrain() :191-201 with wrapping adds; an input the
 *                             reference never returns from (an infinity, or a magnitude at which adding 2 pi leaves the
 *                             f32 unchanged) is YAGI_ERR_CONFIG; NaN gives 0 like Rust's saturating `as u32`
 *   step / get_phase / get_frequency / sin / cos / sin_cos / cexp   :86-133
 *   pll_set_bandwidth / pll_step   :138-150 (a negative bandwidth is YAGI_ERR_CONFIG: the reference panics)
 *   mix_up / mix_down         :155-176 on one sample, on the host
 *   mix_block_up/down         :161-188 on host slices; nx != ny is YAGI_ERR_RANGE.  Up to 4096 samples run on the host,
 *                             longer slices stage through the device; both give the same bits and the same theta.
 *   mix_block_up/down_dev     device buffers, asynchronous on the object's stream; x_dev == y_dev (in place) is allowed,
 *                             any other overlap is YAGI_ERR_CONFIG.  theta advances by n d_theta mod 2^32 at once, so
 *                             host and device calls may be mixed freely.
 *   get_state                 EXTENSION (not in the reference): the raw u32 words theta and d_theta.
 * Every output word equals the reference's sequential loop.  Device form: osc_kernels.hip. */
#define YAGI_OSC_NCO 0
#define YAGI_OSC_VCO 1
typedef struct yagi_hip_osc_s *yagi_hip_osc;
int yagi_hip_osc_create(int scheme, yagi_hip_osc *q);
int yagi_hip_osc_destroy(yagi_hip_osc q);
int yagi_hip_osc_clone(yagi_hip_osc q, yagi_hip_osc *out);
int yagi_hip_osc_set_stream(yagi_hip_osc q, yagi_stream_t s);
int yagi_hip_osc_reset(yagi_hip_osc q);
int yagi_hip_osc_set_frequency(yagi_hip_osc q, float dtheta);
int yagi_hip_osc_adjust_frequency(yagi_hip_osc q, float df);
int yagi_hip_osc_set_phase(yagi_hip_osc q, float phi);
int yagi_hip_osc_adjust_phase(yagi_hip_osc q, float dphi);
int yagi_hip_osc_step(yagi_hip_osc q);
int yagi_hip_osc_get_phase(yagi_hip_osc q, float *phi);
int yagi_hip_osc_get_frequency(yagi_hip_osc q, float *f);
int yagi_hip_osc_get_state(yagi_hip_osc q, uint32_t *theta, uint32_t *d_theta);
int yagi_hip_osc_sin(yagi_hip_osc q, float *s);
int yagi_hip_osc_cos(yagi_hip_osc q, float *c);
int yagi_hip_osc_sin_cos(yagi_hip_osc q, float *s, float *c);
int yagi_hip_osc_cexp(yagi_hip_osc q, yagi_cf32 *y);
int yagi_hip_osc_pll_set_bandwidth(yagi_hip_osc q, float bw);
int yagi_hip_osc_pll_step(yagi_hip_osc q, float dphi);
int yagi_hip_osc_mix_up(yagi_hip_osc q, yagi_cf32 x, yagi_cf32 *y);
int yagi_hip_osc_mix_down(yagi_hip_osc q, yagi_cf32 x, yagi_cf32 *y);
int yagi_hip_osc_mix_block_up(yagi_hip_osc q, const yagi_cf32 *x, size_t nx, yagi_cf32 *y, size_t ny);
int yagi_hip_osc_mix_block_down(yagi_hip_osc q, const yagi_cf32 *x, size_t nx, yagi_cf32 *y, size_t ny);
int yagi_hip_osc_mix_block_up_dev(yagi_hip_osc q, const yagi_cf32 *x_dev, size_t n, yagi_cf32 *y_dev);
int yagi_hip_osc_mix_block_down_dev(yagi_hip_osc q, const yagi_cf32 *x_dev, size_t n, yagi_cf32 *y_dev);

/* ---- Ddc / Duc: digital down- and up-converter (the reference's src/filter/dds.rs is an empty file) -------------------
 * Defined as compositions of two objects of this library, kinds crcf and cccf:
 *   Ddc  = Osc::mix_block_down, then FirDecimationFilter::execute_block: n M samples in, n out.  Input j of a call at
 *          oscillator state (theta, d_theta) is mixed with the phase word theta + (u32)j d_theta; the decimator's window
 *          holds MIXED samples of earlier calls; the call leaves theta + (u32)(n M) d_theta.
 *   Duc  = FirInterpolationFilter::execute_block, then Osc::mix_block_up: n samples in, n I out.  Output j is mixed with
 *          theta + (u32)j d_theta; the interpolator's window holds the unmixed inputs; theta advances by n I steps.
 * Every output word equals what separate yagi_hip_osc and yagi_hip_firdecim / yagi_hip_firinterp objects give for the
 * same taps, scale, frequency, phase and call lengths.
 *   create(scheme, rate, h, h_len)   scheme as for yagi_hip_osc_create, rate / h / h_len as for yagi_hip_firdecim_*_create
 *                             (Ddc) or yagi_hip_firinterp_*_create (Duc); the parts' own YAGI_ERR_CONFIG messages
 *   create_kaiser(scheme, rate, m, as_)   the parts' Kaiser prototype and its errors
 *   clone / set_stream / reset       reset clears the filter window and leaves the oscillator alone
 *   set/adjust_frequency, set/adjust_phase, get_frequency, get_phase   Osc's, through the same constrain()
 *   get_state / set_state            EXTENSION: the raw u32 words theta and d_theta
 *   set_scale / get_scale / get_decim_rate / get_interp_rate          the filter's
 *   execute                          Ddc: x[M] -> *y, Duc: *x -> y[I], on the host mirror with Osc's per-sample mix;
 *                                    may be interleaved with block calls
 *   execute_block(x, n, y)           host slices: n outputs from n M inputs (Ddc), n I outputs from n inputs (Duc)
 *   execute_block_dev                device buffers, asynchronous on the object's stream; x and y must not overlap and
 *                                    need 8-byte alignment only; n = 0 returns at once and changes nothing
 *   set_kernel(choice)               0 auto, 1 two launches through a scratch buffer the object owns, 2 the fused kernel
 *                                    where one serves the shape (else two launches); auto = fused where served
 *   get_last_kernel                  1 or 2: what the last block call ran (0 before the first)
 * Device form: ddc_kernels.hip (which lists the shapes that take two launches). */
#define YAGI_DECLARE_DDC(OBJ, RATE, K, C)                                                                           \
    typedef struct yagi_hip_##OBJ##_##K##_s *yagi_hip_##OBJ##_##K;                                                  \
    int yagi_hip_##OBJ##_##K##_create(int scheme, size_t rate, const C *h, size_t h_len, yagi_hip_##OBJ##_##K *q);  \
    int yagi_hip_##OBJ##_##K##_create_kaiser(int scheme, size_t rate, size_t m, float as_, yagi_hip_##OBJ##_##K *q); \
    int yagi_hip_##OBJ##_##K##_destroy(yagi_hip_##OBJ##_##K q);                                                     \
    int yagi_hip_##OBJ##_##K##_clone(yagi_hip_##OBJ##_##K q, yagi_hip_##OBJ##_##K *out);                            \
    int yagi_hip_##OBJ##_##K##_set_stream(yagi_hip_##OBJ##_##K q, yagi_stream_t s);                                 \
    int yagi_hip_##OBJ##_##K##_reset(yagi_hip_##OBJ##_##K q);                                                       \
    int yagi_hip_##OBJ##_##K##_set_frequency(yagi_hip_##OBJ##_##K q, float dtheta);                                 \
    int yagi_hip_##OBJ##_##K##_adjust_frequency(yagi_hip_##OBJ##_##K q, float df);                                  \
    int yagi_hip_##OBJ##_##K##_set_phase(yagi_hip_##OBJ##_##K q, float phi);                                        \
    int yagi_hip_##OBJ##_##K##_adjust_phase(yagi_hip_##OBJ##_##K q, float dphi);                                    \
    int yagi_hip_##OBJ##_##K##_get_frequency(yagi_hip_##OBJ##_##K q, float *f);                                     \
    int yagi_hip_##OBJ##_##K##_get_phase(yagi_hip_##OBJ##_##K q, float *phi);                                       \
    int yagi_hip_##OBJ##_##K##_get_state(yagi_hip_##OBJ##_##K q, uint32_t *theta, uint32_t *d_theta);               \
    int yagi_hip_##OBJ##_##K##_set_state(yagi_hip_##OBJ##_##K q, uint32_t theta, uint32_t d_theta);                 \
    int yagi_hip_##OBJ##_##K##_set_scale(yagi_hip_##OBJ##_##K q, C scale);                                          \
    int yagi_hip_##OBJ##_##K##_get_scale(yagi_hip_##OBJ##_##K q, C *scale);                                         \
    int yagi_hip_##OBJ##_##K##_##RATE(yagi_hip_##OBJ##_##K q, size_t *rate);                                        \
    int yagi_hip_##OBJ##_##K##_set_kernel(yagi_hip_##OBJ##_##K q, int choice);                                      \
    int yagi_hip_##OBJ##_##K##_get_last_kernel(yagi_hip_##OBJ##_##K q, int *k);                                     \
    int yagi_hip_##OBJ##_##K##_execute(yagi_hip_##OBJ##_##K q, const yagi_cf32 *x, yagi_cf32 *y);                   \
    int yagi_hip_##OBJ##_##K##_execute_block(yagi_hip_##OBJ##_##K q, const yagi_cf32 *x, size_t n, yagi_cf32 *y);   \
    int yagi_hip_##OBJ##_##K##_execute_block_dev(yagi_hip_##OBJ##_##K q, const yagi_cf32 *x_dev, size_t n,          \
                                                 yagi_cf32 *y_dev);
YAGI_DECLARE_DDC(ddc, get_decim_rate, crcf, float)
YAGI_DECLARE_DDC(ddc, get_decim_rate, cccf, yagi_cf32)
YAGI_DECLARE_DDC(duc, get_interp_rate, crcf, float)
YAGI_DECLARE_DDC(duc, get_interp_rate, cccf, yagi_cf32)
#undef YAGI_DECLARE_DDC

/* ---- FirHilbertFilter: src/filter/fir/firhilb.rs:1-263 (FIR Hilbert transform) -------------------------------------
 *   create(m, as_)            new() :38-84  m < 2 is YAGI_ERR_CONFIG; |as_| is used; hq = 2m taps of the Kaiser
 *                             half-band filter (4m + 1 taps, fc 0.25) times sin(pi/2 t), every other one reversed
 *   clone / reset             derive(Clone) / reset() :87-93 (the four windows and the toggle are zeroed)
 *   r2c_execute               :104-137 one real sample -> one complex sample
 *   c2r_execute               :149-180 one complex sample -> (lower side-band, upper side-band)
 *   decim_execute             :191-211 x[0..2) -> one complex sample
 *   interp_execute            :233-248 one complex sample -> y[0..2)
 *   decim/interp_execute_block   :220-262 on host slices: decim nx = 2 ny, interp ny = 2 nx, else YAGI_ERR_RANGE
 *   r2c/c2r_execute_block     EXTENSION: n repeated per-sample calls; r2c ny = nx, c2r ny = 2 nx (the (lsb, usb) pair
 *                             of input i at y[2i], y[2i + 1]).  Up to 4096 units run on the host, longer slices stage
 *                             through the device; both give the same bits.
 *   *_execute_block_dev       device buffers, n units (decim: n outputs from 2n inputs), asynchronous on the object's
 *                             stream; x and y overlapping is YAGI_ERR_CONFIG.
 *   design                    EXTENSION: the 2m taps hq, no device needed.
 * All four modes share the four windows and the toggle, as in the reference, so calls of every mode and form may be
 * mixed on one object.  Every output word equals the reference's sequential loop.  Device form: firhilb_kernels.hip
 * (DESIGN.md section 4). */
typedef struct yagi_hip_firhilb_s *yagi_hip_firhilb;
int yagi_hip_firhilb_create(size_t m, float as_, yagi_hip_firhilb *q);
int yagi_hip_firhilb_destroy(yagi_hip_firhilb q);
int yagi_hip_firhilb_clone(yagi_hip_firhilb q, yagi_hip_firhilb *out);
int yagi_hip_firhilb_set_stream(yagi_hip_firhilb q, yagi_stream_t s);
int yagi_hip_firhilb_reset(yagi_hip_firhilb q);
int yagi_hip_firhilb_r2c_execute(yagi_hip_firhilb q, float x, yagi_cf32 *y);
int yagi_hip_firhilb_c2r_execute(yagi_hip_firhilb q, yagi_cf32 x, float *y0, float *y1);
int yagi_hip_firhilb_decim_execute(yagi_hip_firhilb q, const float *x, yagi_cf32 *y);
int yagi_hip_firhilb_interp_execute(yagi_hip_firhilb q, yagi_cf32 x, float *y);
int yagi_hip_firhilb_r2c_execute_block(yagi_hip_firhilb q, const float *x, size_t nx, yagi_cf32 *y, size_t ny);
int yagi_hip_firhilb_c2r_execute_block(yagi_hip_firhilb q, const yagi_cf32 *x, size_t nx, float *y, size_t ny);
int yagi_hip_firhilb_decim_execute_block(yagi_hip_firhilb q, const float *x, size_t nx, yagi_cf32 *y, size_t ny);
int yagi_hip_firhilb_interp_execute_block(yagi_hip_firhilb q, const yagi_cf32 *x, size_t nx, float *y, size_t ny);
int yagi_hip_firhilb_r2c_execute_block_dev(yagi_hip_firhilb q, const float *x_dev, size_t n, yagi_cf32 *y_dev);
int yagi_hip_firhilb_c2r_execute_block_dev(yagi_hip_firhilb q, const yagi_cf32 *x_dev, size_t n, float *y_dev);
int yagi_hip_firhilb_decim_execute_block_dev(yagi_hip_firhilb q, const float *x_dev, size_t n, yagi_cf32 *y_dev);
int yagi_hip_firhilb_interp_execute_block_dev(yagi_hip_firhilb q, const yagi_cf32 *x_dev, size_t n, float *y_dev);
int yagi_hip_firhilb_design(size_t m, float as_, float *hq);

/* ---- Fdelay: src/filter/fdelay.rs:1-137 (fractional delay, 0 <= delay <= nmax) --------------------------------------
 *   create(nmax, m, npfb)     new() :26-53  a zero parameter is YAGI_ERR_CONFIG; the bank is FirPfbFilter::default(npfb,
 *                             m): Kaiser, 2 npfb m + 1 taps, cut-off 0.5 / npfb, 60 dB, branch length Ls = h_len div npfb
 *                             (2m, and 2m + 1 for npfb = 1).  Limits of this build: nmax <= 2^24 (where nmax as f32 is exact), Ls <= 4096.
 *   create_default(nmax)      new_default() :55-57  m = 8, npfb = 64
 *   clone / reset             derive(Clone) / reset() :59-65 (delay 0, the reference's w_index = nmax - 1, f_index = 0,
 *                             both windows zeroed)
 *   get_delay / set_delay / adjust_delay   :67-101 in f32; a delay outside [0, nmax] (NaN included) or a failed
 *                             adjust_delay is YAGI_ERR_CONFIG and leaves the object unchanged
 *   get_nmax / get_m / get_npfb   :103-113
 *   push / write / execute    :115-128 on the host mirror, no launch
 *   execute_block             :130-136 on host slices (the shorter of nx, ny), staged through the device
 *   execute_block_dev         device buffers, asynchronous on the object's stream; x and y overlapping is
 *                             YAGI_ERR_CONFIG
 *   execute_track             EXTENSION: one delay per sample, equal to `for i: set_delay(delay[i]); push(x[i]);
 *                             y[i] = execute()`; afterwards get_delay() is delay[n - 1].  The whole delay array is
 *                             validated before any state moves (YAGI_ERR_CONFIG, object unchanged).
 *   execute_track_dev         the same on device buffers.  It cannot validate: each delay is CLAMPED into [0, nmax], and
 *                             anything that is not >= 0 (NaN included) counts as 0.  The next call that needs the lag on
 *                             the host (get_delay, adjust_delay, a fixed-delay block call, a per-sample call) waits for
 *                             the stream and reads the last delay back.
 * Every output word equals the reference's sequential loop, also where the delay changes between or inside calls.
 * Device form: fdelay_kernels.hip. */
#define YAGI_FDELAY_API(K, T)                                                                                   \
    typedef struct yagi_hip_fdelay_##K##_s *yagi_hip_fdelay_##K;                                                     \
    int yagi_hip_fdelay_##K##_create(size_t nmax, size_t m, size_t npfb, yagi_hip_fdelay_##K *q);                    \
    int yagi_hip_fdelay_##K##_create_default(size_t nmax, yagi_hip_fdelay_##K *q);                                   \
    int yagi_hip_fdelay_##K##_destroy(yagi_hip_fdelay_##K q);                                                        \
    int yagi_hip_fdelay_##K##_clone(yagi_hip_fdelay_##K q, yagi_hip_fdelay_##K *out);                                \
    int yagi_hip_fdelay_##K##_set_stream(yagi_hip_fdelay_##K q, yagi_stream_t s);                                    \
    int yagi_hip_fdelay_##K##_reset(yagi_hip_fdelay_##K q);                                                          \
    int yagi_hip_fdelay_##K##_get_delay(yagi_hip_fdelay_##K q, float *delay);                                        \
    int yagi_hip_fdelay_##K##_set_delay(yagi_hip_fdelay_##K q, float delay);                                         \
    int yagi_hip_fdelay_##K##_adjust_delay(yagi_hip_fdelay_##K q, float delta);                                      \
    int yagi_hip_fdelay_##K##_get_nmax(yagi_hip_fdelay_##K q, size_t *nmax);                                         \
    int yagi_hip_fdelay_##K##_get_m(yagi_hip_fdelay_##K q, size_t *m);                                               \
    int yagi_hip_fdelay_##K##_get_npfb(yagi_hip_fdelay_##K q, size_t *npfb);                                         \
    int yagi_hip_fdelay_##K##_push(yagi_hip_fdelay_##K q, T x);                                                      \
    int yagi_hip_fdelay_##K##_write(yagi_hip_fdelay_##K q, const T *x, size_t n);                                    \
    int yagi_hip_fdelay_##K##_execute(yagi_hip_fdelay_##K q, T *y);                                                  \
    int yagi_hip_fdelay_##K##_execute_block(yagi_hip_fdelay_##K q, const T *x, size_t nx, T *y, size_t ny);          \
    int yagi_hip_fdelay_##K##_execute_block_dev(yagi_hip_fdelay_##K q, const T *x_dev, size_t n, T *y_dev);          \
    int yagi_hip_fdelay_##K##_execute_track(yagi_hip_fdelay_##K q, const float *delay, const T *x, size_t n, T *y);  \
    int yagi_hip_fdelay_##K##_execute_track_dev(yagi_hip_fdelay_##K q, const float *delay_dev, const T *x_dev,       \
                                                size_t n, T *y_dev);
YAGI_FDELAY_API(rrrf, float)
YAGI_FDELAY_API(crcf, yagi_cf32)
YAGI_FDELAY_API(cccf, yagi_cf32)

/* ---- IIR design, low-pass second-order sections: src/filter/iir/design/mod.rs:567-717, butter.rs, cheby2.rs --------
 *   yagi_hip_iir_design_lowpass_sos(shape, order, fc, ap, as_, b, a)   iir_design() on its low-pass / SOS branch; b, a
 *                             hold 3 (L + r) floats, L = order / 2, r = order % 2 (the odd section last, b2 = a2 = 0).
 *                             No device needed.  fc outside (0, 0.5), ap <= 0, as_ <= 0 and order 0 are YAGI_ERR_CONFIG
 *                             as in the reference; YAGI_IIRDES_CHEBY1 / ELLIP / BESSEL are YAGI_ERR_CONFIG ("not built").
 *   iirfilt_*_create_prototype(shape, order, fc, ap, as_)   IirFilter::new_prototype :148-184 (Lowpass, SOS)
 *   iirfilt_*_create_lowpass(order, fc)                     IirFilter::new_lowpass :189-201 (Butterworth, 0.1, 60) */
#define YAGI_IIRDES_BUTTER 0
#define YAGI_IIRDES_CHEBY1 1
#define YAGI_IIRDES_CHEBY2 2
#define YAGI_IIRDES_ELLIP 3
#define YAGI_IIRDES_BESSEL 4
int yagi_hip_iir_design_lowpass_sos(int shape, size_t order, float fc, float ap, float as_, float *b, float *a);
int yagi_hip_iirfilt_rrrf_create_prototype(int shape, size_t order, float fc, float ap, float as_, yagi_hip_iirfilt_rrrf *q);
int yagi_hip_iirfilt_rrrf_create_lowpass(size_t order, float fc, yagi_hip_iirfilt_rrrf *q);
int yagi_hip_iirfilt_crcf_create_prototype(int shape, size_t order, float fc, float ap, float as_, yagi_hip_iirfilt_crcf *q);
int yagi_hip_iirfilt_crcf_create_lowpass(size_t order, float fc, yagi_hip_iirfilt_crcf *q);
int yagi_hip_iirfilt_cccf_create_prototype(int shape, size_t order, float fc, float ap, float as_, yagi_hip_iirfilt_cccf *q);
int yagi_hip_iirfilt_cccf_create_lowpass(size_t order, float fc, yagi_hip_iirfilt_cccf *q);

/* ---- IirDecimationFilter / IirInterpolationFilter: src/filter/iir/iirdecim.rs, iirinterp.rs ---------------------------
 * One IirFilter run over a virtual stream of n M filter steps:
 *   iirdecim   steps i M .. i M + M - 1 read x[i M ..], the output of step i M is kept (iirdecim.rs:128-137)
 *   iirinterp  step i M reads x[i], the M - 1 steps after it read +0.0, every output is kept (iirinterp.rs:93-103)
 *   create(M, b, nb, a, na)   new() (transfer function); create_sos(M, b, a, nsos): EXTENSION, external sections
 *   create_prototype(M, shape, order, fc, ap, as_)   new_prototype() (Lowpass, SOS); iirinterp sets the scale to M (:66-69)
 *   create_default(M, order)  iirdecim: Butterworth, fc 0.5/M (:63-75); iirinterp: Chebyshev-II, fc 0.5/M, 0.1, 60 (:34-46)
 *   execute                   iirdecim: x[0..M) -> one sample; iirinterp: one sample -> y[0..M); always on the host mirror
 *   execute_block(x, n, y)    n units: iirdecim reads n M samples and writes n, iirinterp reads n and writes n M.
 *                             Up to 32 filter steps run on the host mirror, longer slices stage through the device.
 *   execute_block_dev         device buffers, asynchronous on the object's stream; x and y overlapping is YAGI_ERR_CONFIG
 *   groupdelay                the filter's (iirinterp: divided by M, :118-120); get_decim / get_interp: M
 * M < 2 is YAGI_ERR_CONFIG as in the reference; M > 65536 is YAGI_ERR_CONFIG too (the kernels' 32-bit index split).
 * Every output word equals IirFilter's over the explicitly built stream. */
typedef struct yagi_hip_iirdecim_rrrf_s *yagi_hip_iirdecim_rrrf;
int yagi_hip_iirdecim_rrrf_create(size_t M, const float *b, size_t nb, const float *a, size_t na, yagi_hip_iirdecim_rrrf *q);
int yagi_hip_iirdecim_rrrf_create_sos(size_t M, const float *b, const float *a, size_t nsos, yagi_hip_iirdecim_rrrf *q);
int yagi_hip_iirdecim_rrrf_create_prototype(size_t M, int shape, size_t order, float fc, float ap, float as_, yagi_hip_iirdecim_rrrf *q);
int yagi_hip_iirdecim_rrrf_create_default(size_t M, size_t order, yagi_hip_iirdecim_rrrf *q);
int yagi_hip_iirdecim_rrrf_destroy(yagi_hip_iirdecim_rrrf q);
int yagi_hip_iirdecim_rrrf_clone(yagi_hip_iirdecim_rrrf q, yagi_hip_iirdecim_rrrf *out);
int yagi_hip_iirdecim_rrrf_set_stream(yagi_hip_iirdecim_rrrf q, yagi_stream_t s);
int yagi_hip_iirdecim_rrrf_reset(yagi_hip_iirdecim_rrrf q);
int yagi_hip_iirdecim_rrrf_execute(yagi_hip_iirdecim_rrrf q, const float *x, float *y);
int yagi_hip_iirdecim_rrrf_execute_block(yagi_hip_iirdecim_rrrf q, const float *x, size_t n, float *y);
int yagi_hip_iirdecim_rrrf_execute_block_dev(yagi_hip_iirdecim_rrrf q, const float *x_dev, size_t n, float *y_dev);
int yagi_hip_iirdecim_rrrf_groupdelay(yagi_hip_iirdecim_rrrf q, float fc, float *gd);
int yagi_hip_iirdecim_rrrf_get_decim(yagi_hip_iirdecim_rrrf q, size_t *M);
int yagi_hip_iirdecim_rrrf_set_scale(yagi_hip_iirdecim_rrrf q, float scale);
int yagi_hip_iirdecim_rrrf_get_scale(yagi_hip_iirdecim_rrrf q, float *scale);
typedef struct yagi_hip_iirdecim_crcf_s *yagi_hip_iirdecim_crcf;
int yagi_hip_iirdecim_crcf_create(size_t M, const float *b, size_t nb, const float *a, size_t na, yagi_hip_iirdecim_crcf *q);
int yagi_hip_iirdecim_crcf_create_sos(size_t M, const float *b, const float *a, size_t nsos, yagi_hip_iirdecim_crcf *q);
int yagi_hip_iirdecim_crcf_create_prototype(size_t M, int shape, size_t order, float fc, float ap, float as_, yagi_hip_iirdecim_crcf *q);
int yagi_hip_iirdecim_crcf_create_default(size_t M, size_t order, yagi_hip_iirdecim_crcf *q);
int yagi_hip_iirdecim_crcf_destroy(yagi_hip_iirdecim_crcf q);
int yagi_hip_iirdecim_crcf_clone(yagi_hip_iirdecim_crcf q, yagi_hip_iirdecim_crcf *out);
int yagi_hip_iirdecim_crcf_set_stream(yagi_hip_iirdecim_crcf q, yagi_stream_t s);
int yagi_hip_iirdecim_crcf_reset(yagi_hip_iirdecim_crcf q);
int yagi_hip_iirdecim_crcf_execute(yagi_hip_iirdecim_crcf q, const yagi_cf32 *x, yagi_cf32 *y);
int yagi_hip_iirdecim_crcf_execute_block(yagi_hip_iirdecim_crcf q, const yagi_cf32 *x, size_t n, yagi_cf32 *y);
int yagi_hip_iirdecim_crcf_execute_block_dev(yagi_hip_iirdecim_crcf q, const yagi_cf32 *x_dev, size_t n, yagi_cf32 *y_dev);
int yagi_hip_iirdecim_crcf_groupdelay(yagi_hip_iirdecim_crcf q, float fc, float *gd);
int yagi_hip_iirdecim_crcf_get_decim(yagi_hip_iirdecim_crcf q, size_t *M);
int yagi_hip_iirdecim_crcf_set_scale(yagi_hip_iirdecim_crcf q, float scale);
int yagi_hip_iirdecim_crcf_get_scale(yagi_hip_iirdecim_crcf q, float *scale);
typedef struct yagi_hip_iirdecim_cccf_s *yagi_hip_iirdecim_cccf;
int yagi_hip_iirdecim_cccf_create(size_t M, const yagi_cf32 *b, size_t nb, const yagi_cf32 *a, size_t na, yagi_hip_iirdecim_cccf *q);
int yagi_hip_iirdecim_cccf_create_sos(size_t M, const yagi_cf32 *b, const yagi_cf32 *a, size_t nsos, yagi_hip_iirdecim_cccf *q);
int yagi_hip_iirdecim_cccf_create_prototype(size_t M, int shape, size_t order, float fc, float ap, float as_, yagi_hip_iirdecim_cccf *q);
int yagi_hip_iirdecim_cccf_create_default(size_t M, size_t order, yagi_hip_iirdecim_cccf *q);
int yagi_hip_iirdecim_cccf_destroy(yagi_hip_iirdecim_cccf q);
int yagi_hip_iirdecim_cccf_clone(yagi_hip_iirdecim_cccf q, yagi_hip_iirdecim_cccf *out);
int yagi_hip_iirdecim_cccf_set_stream(yagi_hip_iirdecim_cccf q, yagi_stream_t s);
int yagi_hip_iirdecim_cccf_reset(yagi_hip_iirdecim_cccf q);
int yagi_hip_iirdecim_cccf_execute(yagi_hip_iirdecim_cccf q, const yagi_cf32 *x, yagi_cf32 *y);
int yagi_hip_iirdecim_cccf_execute_block(yagi_hip_iirdecim_cccf q, const yagi_cf32 *x, size_t n, yagi_cf32 *y);
int yagi_hip_iirdecim_cccf_execute_block_dev(yagi_hip_iirdecim_cccf q, const yagi_cf32 *x_dev, size_t n, yagi_cf32 *y_dev);
int yagi_hip_iirdecim_cccf_groupdelay(yagi_hip_iirdecim_cccf q, float fc, float *gd);
int yagi_hip_iirdecim_cccf_get_decim(yagi_hip_iirdecim_cccf q, size_t *M);
int yagi_hip_iirdecim_cccf_set_scale(yagi_hip_iirdecim_cccf q, yagi_cf32 scale);
int yagi_hip_iirdecim_cccf_get_scale(yagi_hip_iirdecim_cccf q, yagi_cf32 *scale);
typedef struct yagi_hip_iirinterp_rrrf_s *yagi_hip_iirinterp_rrrf;
int yagi_hip_iirinterp_rrrf_create(size_t M, const float *b, size_t nb, const float *a, size_t na, yagi_hip_iirinterp_rrrf *q);
int yagi_hip_iirinterp_rrrf_create_sos(size_t M, const float *b, const float *a, size_t nsos, yagi_hip_iirinterp_rrrf *q);
int yagi_hip_iirinterp_rrrf_create_prototype(size_t M, int shape, size_t order, float fc, float ap, float as_, yagi_hip_iirinterp_rrrf *q);
int yagi_hip_iirinterp_rrrf_create_default(size_t M, size_t order, yagi_hip_iirinterp_rrrf *q);
int yagi_hip_iirinterp_rrrf_destroy(yagi_hip_iirinterp_rrrf q);
int yagi_hip_iirinterp_rrrf_clone(yagi_hip_iirinterp_rrrf q, yagi_hip_iirinterp_rrrf *out);
int yagi_hip_iirinterp_rrrf_set_stream(yagi_hip_iirinterp_rrrf q, yagi_stream_t s);
int yagi_hip_iirinterp_rrrf_reset(yagi_hip_iirinterp_rrrf q);
int yagi_hip_iirinterp_rrrf_execute(yagi_hip_iirinterp_rrrf q, float x, float *y);
int yagi_hip_iirinterp_rrrf_execute_block(yagi_hip_iirinterp_rrrf q, const float *x, size_t n, float *y);
int yagi_hip_iirinterp_rrrf_execute_block_dev(yagi_hip_iirinterp_rrrf q, const float *x_dev, size_t n, float *y_dev);
int yagi_hip_iirinterp_rrrf_groupdelay(yagi_hip_iirinterp_rrrf q, float fc, float *gd);
int yagi_hip_iirinterp_rrrf_get_interp(yagi_hip_iirinterp_rrrf q, size_t *M);
int yagi_hip_iirinterp_rrrf_set_scale(yagi_hip_iirinterp_rrrf q, float scale);
int yagi_hip_iirinterp_rrrf_get_scale(yagi_hip_iirinterp_rrrf q, float *scale);
typedef struct yagi_hip_iirinterp_crcf_s *yagi_hip_iirinterp_crcf;
int yagi_hip_iirinterp_crcf_create(size_t M, const float *b, size_t nb, const float *a, size_t na, yagi_hip_iirinterp_crcf *q);
int yagi_hip_iirinterp_crcf_create_sos(size_t M, const float *b, const float *a, size_t nsos, yagi_hip_iirinterp_crcf *q);
int yagi_hip_iirinterp_crcf_create_prototype(size_t M, int shape, size_t order, float fc, float ap, float as_, yagi_hip_iirinterp_crcf *q);
int yagi_hip_iirinterp_crcf_create_default(size_t M, size_t order, yagi_hip_iirinterp_crcf *q);
int yagi_hip_iirinterp_crcf_destroy(yagi_hip_iirinterp_crcf q);
int yagi_hip_iirinterp_crcf_clone(yagi_hip_iirinterp_crcf q, yagi_hip_iirinterp_crcf *out);
int yagi_hip_iirinterp_crcf_set_stream(yagi_hip_iirinterp_crcf q, yagi_stream_t s);
int yagi_hip_iirinterp_crcf_reset(yagi_hip_iirinterp_crcf q);
int yagi_hip_iirinterp_crcf_execute(yagi_hip_iirinterp_crcf q, yagi_cf32 x, yagi_cf32 *y);
int yagi_hip_iirinterp_crcf_execute_block(yagi_hip_iirinterp_crcf q, const yagi_cf32 *x, size_t n, yagi_cf32 *y);
int yagi_hip_iirinterp_crcf_execute_block_dev(yagi_hip_iirinterp_crcf q, const yagi_cf32 *x_dev, size_t n, yagi_cf32 *y_dev);
int yagi_hip_iirinterp_crcf_groupdelay(yagi_hip_iirinterp_crcf q, float fc, float *gd);
int yagi_hip_iirinterp_crcf_get_interp(yagi_hip_iirinterp_crcf q, size_t *M);
int yagi_hip_iirinterp_crcf_set_scale(yagi_hip_iirinterp_crcf q, float scale);
int yagi_hip_iirinterp_crcf_get_scale(yagi_hip_iirinterp_crcf q, float *scale);
typedef struct yagi_hip_iirinterp_cccf_s *yagi_hip_iirinterp_cccf;
int yagi_hip_iirinterp_cccf_create(size_t M, const yagi_cf32 *b, size_t nb, const yagi_cf32 *a, size_t na, yagi_hip_iirinterp_cccf *q);
int yagi_hip_iirinterp_cccf_create_sos(size_t M, const yagi_cf32 *b, const yagi_cf32 *a, size_t nsos, yagi_hip_iirinterp_cccf *q);
int yagi_hip_iirinterp_cccf_create_prototype(size_t M, int shape, size_t order, float fc, float ap, float as_, yagi_hip_iirinterp_cccf *q);
int yagi_hip_iirinterp_cccf_create_default(size_t M, size_t order, yagi_hip_iirinterp_cccf *q);
int yagi_hip_iirinterp_cccf_destroy(yagi_hip_iirinterp_cccf q);
int yagi_hip_iirinterp_cccf_clone(yagi_hip_iirinterp_cccf q, yagi_hip_iirinterp_cccf *out);
int yagi_hip_iirinterp_cccf_set_stream(yagi_hip_iirinterp_cccf q, yagi_stream_t s);
int yagi_hip_iirinterp_cccf_reset(yagi_hip_iirinterp_cccf q);
int yagi_hip_iirinterp_cccf_execute(yagi_hip_iirinterp_cccf q, yagi_cf32 x, yagi_cf32 *y);
int yagi_hip_iirinterp_cccf_execute_block(yagi_hip_iirinterp_cccf q, const yagi_cf32 *x, size_t n, yagi_cf32 *y);
int yagi_hip_iirinterp_cccf_execute_block_dev(yagi_hip_iirinterp_cccf q, const yagi_cf32 *x_dev, size_t n, yagi_cf32 *y_dev);
int yagi_hip_iirinterp_cccf_groupdelay(yagi_hip_iirinterp_cccf q, float fc, float *gd);
int yagi_hip_iirinterp_cccf_get_interp(yagi_hip_iirinterp_cccf q, size_t *M);
int yagi_hip_iirinterp_cccf_set_scale(yagi_hip_iirinterp_cccf q, yagi_cf32 scale);
int yagi_hip_iirinterp_cccf_get_scale(yagi_hip_iirinterp_cccf q, yagi_cf32 *scale);

/* ---- IirHilbertFilter: src/filter/iir/iirhilb.rs (IIR Hilbert transform) -----------------------------------------------
 * The reference's two real filters with identical coefficients are one crcf filter over a complex stream (re -> filt_0,
 * im -> filt_1); the four modes are input / output maps of that stream selected by the 2-bit state.
 *   create(shape, n, ap, as_) new() :15-36  low-pass prototype at fc 0.25 in second-order sections; n == 0 is YAGI_ERR_CONFIG
 *   create_default(n)         new_default() :38-47  Butterworth, 0.1, 60
 *   create_sos(b, a, nsos)    EXTENSION: externally designed real sections
 *   clone / reset             derive(Clone) / reset() :49-53
 *   r2c / c2r / decim / interp _execute   :55-158 on the host mirror
 *   *_execute_block(x, n, y)  n units on host slices (decim: 2n real -> n complex; interp: n complex -> 2n real); up to
 *                             32 filter steps on the host mirror, longer slices stage through the device
 *   *_execute_block_dev       device buffers, asynchronous on the object's stream; the state advances on the host at
 *                             once.  decim and interp may run in place (x_dev == y_dev: the same bytes per unit); any
 *                             other overlap is YAGI_ERR_CONFIG.
 *   get_state                 EXTENSION: the 2-bit state
 * DIVERGENCE: decim / interp compute 1 - state on a u8, which underflows in the reference when r2c / c2r left the state
 * at 2 or 3; here that is YAGI_ERR_MODE ("reset first"). */
typedef struct yagi_hip_iirhilbf_s *yagi_hip_iirhilbf;
int yagi_hip_iirhilbf_create(int shape, size_t n, float ap, float as_, yagi_hip_iirhilbf *q);
int yagi_hip_iirhilbf_create_default(size_t n, yagi_hip_iirhilbf *q);
int yagi_hip_iirhilbf_create_sos(const float *b, const float *a, size_t nsos, yagi_hip_iirhilbf *q);
int yagi_hip_iirhilbf_destroy(yagi_hip_iirhilbf q);
int yagi_hip_iirhilbf_clone(yagi_hip_iirhilbf q, yagi_hip_iirhilbf *out);
int yagi_hip_iirhilbf_set_stream(yagi_hip_iirhilbf q, yagi_stream_t s);
int yagi_hip_iirhilbf_reset(yagi_hip_iirhilbf q);
int yagi_hip_iirhilbf_get_state(yagi_hip_iirhilbf q, int *state);
int yagi_hip_iirhilbf_r2c_execute(yagi_hip_iirhilbf q, float x, yagi_cf32 *y);
int yagi_hip_iirhilbf_c2r_execute(yagi_hip_iirhilbf q, yagi_cf32 x, float *y);
int yagi_hip_iirhilbf_decim_execute(yagi_hip_iirhilbf q, const float *x, yagi_cf32 *y);
int yagi_hip_iirhilbf_interp_execute(yagi_hip_iirhilbf q, yagi_cf32 x, float *y);
int yagi_hip_iirhilbf_r2c_execute_block(yagi_hip_iirhilbf q, const float *x, size_t n, yagi_cf32 *y);
int yagi_hip_iirhilbf_c2r_execute_block(yagi_hip_iirhilbf q, const yagi_cf32 *x, size_t n, float *y);
int yagi_hip_iirhilbf_decim_execute_block(yagi_hip_iirhilbf q, const float *x, size_t n, yagi_cf32 *y);
int yagi_hip_iirhilbf_interp_execute_block(yagi_hip_iirhilbf q, const yagi_cf32 *x, size_t n, float *y);
int yagi_hip_iirhilbf_r2c_execute_block_dev(yagi_hip_iirhilbf q, const float *x_dev, size_t n, yagi_cf32 *y_dev);
int yagi_hip_iirhilbf_c2r_execute_block_dev(yagi_hip_iirhilbf q, const yagi_cf32 *x_dev, size_t n, float *y_dev);
int yagi_hip_iirhilbf_decim_execute_block_dev(yagi_hip_iirhilbf q, const float *x_dev, size_t n, yagi_cf32 *y_dev);
int yagi_hip_iirhilbf_interp_execute_block_dev(yagi_hip_iirhilbf q, const yagi_cf32 *x_dev, size_t n, float *y_dev);

/* ---- Modem: src/modem/modem.rs:27-575, src/modem/modem/{psk,dpsk,ask,qam,bpsk,qpsk,ook,arb}.rs ----------------------------
 * Linear modulation and hard / soft demodulation.  Symbols are one byte each in the block forms (bps <= 8); soft bits
 * are bytes, bps per symbol, most significant bit first (0 = a certain 0, 255 = a certain 1).
 *   create(scheme)            Modem::new :151-207 for PSK2..256, DPSK2..256, ASK2..256, QAM4..256, BPSK, QPSK, OOK.
 *                             APSK*, SQAM32/128, V29, ARB*OPT, ARB64VT/UI and PI4DQPSK are YAGI_ERR_CONFIG: their
 *                             constellations are constants of the reference's source and are not part of this
 *                             library.  YAGI_MODEM_ARB and YAGI_MODEM_UNKNOWN are YAGI_ERR_CONFIG (use from_table).
 *   create_from_table(t, n)   Modem::from_table :209-216 (scheme ARB): n = 2, 4, .. 256 points, balanced to zero mean
 *                             and scaled to unit energy (arb.rs:76-94); anything else is YAGI_ERR_CONFIG.  The mean, the
 *                             energy and the division are computed in double and rounded to f32 at the end, where the
 *                             reference sums in f32: each point is within an ulp of the exact balanced, scaled point
 *   get_constellation         extension: the M points, map[s] = modulate(s) (DPSK: map[k] = polar(1, k 2 pi / M))
 *   get_neighbours            extension: the soft demodulator's table, *p entries per symbol (0: the scheme has none),
 *                             nbr[s * p + i]; nbr may be NULL to ask for p alone, else cap >= M * p.  Built as
 *                             init_demod_soft_tab :465-511, except that the "empty" mark cannot collide with symbol
 *                             0 at M = 256 (the reference's `M as u8` does): every list is the p nearest other points
 *   modulate / demodulate / demodulate_soft / get_demodulator_{sample,phase_error,evm}   :243-283 on the host mirror.
 *                             modulate of a symbol >= M is YAGI_ERR_RANGE
 *   modulate_block            n symbols -> n samples.  A symbol >= M anywhere fails the call with YAGI_ERR_RANGE and y
 *                             is not written (host form: checked on the host; _dev form: checked on the device through
 *                             a flag that the call waits for and reads back)
 *   demodulate_block          n samples -> n symbols; xhat (may be NULL) receives the re-modulated decisions (x_hat)
 *   demodulate_soft_block     n samples -> n symbols and n * bps soft bytes
 * After a demodulating block call the object's r / x_hat (get_demodulator_*) are those of the block's last sample; DPSK's
 * phase carries across per-sample and block calls in any mixture.  The _dev forms take device pointers of any byte
 * alignment for symbols and soft bits, run on the object's stream (demodulation asynchronously), and their operands
 * must not overlap (YAGI_ERR_CONFIG).  The decisions, soft bits and x_hat equal the reference's f32 arithmetic operation
 * by operation; Arb's hard decision compares squared distances where the reference compares hypot().
 * Deviation, DPSK modulation: the reference adds sym 2 pi / M into an f32 phase sample by sample and wraps at 2 pi
 * (dpsk.rs:55-60), whose rounding drifts with the stream's length.  Here the state is the exact running index
 * k_n = (k_{n-1} + gray_decode(s_n)) mod M and the output map[k_n]: no drift, and a block form.  The modulator's k and
 * the demodulator's phase are separate states (the reference shares one field between them).
 * random_symbol is not provided.  Device form: modem_kernels.hip. */
typedef enum {
    YAGI_MODEM_UNKNOWN = 0, YAGI_MODEM_PSK2 = 1, YAGI_MODEM_PSK4 = 2, YAGI_MODEM_PSK8 = 3,
    YAGI_MODEM_PSK16 = 4, YAGI_MODEM_PSK32 = 5, YAGI_MODEM_PSK64 = 6, YAGI_MODEM_PSK128 = 7,
    YAGI_MODEM_PSK256 = 8, YAGI_MODEM_DPSK2 = 9, YAGI_MODEM_DPSK4 = 10, YAGI_MODEM_DPSK8 = 11,
    YAGI_MODEM_DPSK16 = 12, YAGI_MODEM_DPSK32 = 13, YAGI_MODEM_DPSK64 = 14, YAGI_MODEM_DPSK128 = 15,
    YAGI_MODEM_DPSK256 = 16, YAGI_MODEM_ASK2 = 17, YAGI_MODEM_ASK4 = 18, YAGI_MODEM_ASK8 = 19,
    YAGI_MODEM_ASK16 = 20, YAGI_MODEM_ASK32 = 21, YAGI_MODEM_ASK64 = 22, YAGI_MODEM_ASK128 = 23,
    YAGI_MODEM_ASK256 = 24, YAGI_MODEM_QAM4 = 25, YAGI_MODEM_QAM8 = 26, YAGI_MODEM_QAM16 = 27,
    YAGI_MODEM_QAM32 = 28, YAGI_MODEM_QAM64 = 29, YAGI_MODEM_QAM128 = 30, YAGI_MODEM_QAM256 = 31,
    YAGI_MODEM_APSK4 = 32, YAGI_MODEM_APSK8 = 33, YAGI_MODEM_APSK16 = 34, YAGI_MODEM_APSK32 = 35,
    YAGI_MODEM_APSK64 = 36, YAGI_MODEM_APSK128 = 37, YAGI_MODEM_APSK256 = 38, YAGI_MODEM_BPSK = 39,
    YAGI_MODEM_QPSK = 40, YAGI_MODEM_OOK = 41, YAGI_MODEM_SQAM32 = 42, YAGI_MODEM_SQAM128 = 43,
    YAGI_MODEM_V29 = 44, YAGI_MODEM_ARB16OPT = 45, YAGI_MODEM_ARB32OPT = 46, YAGI_MODEM_ARB64OPT = 47,
    YAGI_MODEM_ARB128OPT = 48, YAGI_MODEM_ARB256OPT = 49, YAGI_MODEM_ARB64VT = 50, YAGI_MODEM_ARB64UI = 51,
    YAGI_MODEM_PI4DQPSK = 52, YAGI_MODEM_ARB = 53
} yagi_modem_scheme;
typedef struct yagi_hip_modem_s *yagi_hip_modem;
int yagi_hip_modem_create(int scheme, yagi_hip_modem *q);
int yagi_hip_modem_create_from_table(const yagi_cf32 *table, size_t n, yagi_hip_modem *q);
int yagi_hip_modem_destroy(yagi_hip_modem q);
int yagi_hip_modem_clone(yagi_hip_modem q, yagi_hip_modem *out);
int yagi_hip_modem_set_stream(yagi_hip_modem q, yagi_stream_t s);
int yagi_hip_modem_reset(yagi_hip_modem q);
int yagi_hip_modem_get_bps(yagi_hip_modem q, size_t *bps);
int yagi_hip_modem_get_scheme(yagi_hip_modem q, int *scheme);
int yagi_hip_modem_get_constellation_size(yagi_hip_modem q, size_t *m);
int yagi_hip_modem_get_constellation(yagi_hip_modem q, yagi_cf32 *map);
int yagi_hip_modem_get_neighbours(yagi_hip_modem q, uint8_t *nbr, size_t cap, size_t *p);
int yagi_hip_modem_modulate(yagi_hip_modem q, unsigned sym, yagi_cf32 *y);
int yagi_hip_modem_demodulate(yagi_hip_modem q, yagi_cf32 x, unsigned *sym);
int yagi_hip_modem_demodulate_soft(yagi_hip_modem q, yagi_cf32 x, unsigned *sym, uint8_t *soft);
int yagi_hip_modem_get_demodulator_sample(yagi_hip_modem q, yagi_cf32 *x_hat);
int yagi_hip_modem_get_demodulator_phase_error(yagi_hip_modem q, float *e);
int yagi_hip_modem_get_demodulator_evm(yagi_hip_modem q, float *evm);
int yagi_hip_modem_modulate_block(yagi_hip_modem q, const uint8_t *sym, size_t n, yagi_cf32 *y);
int yagi_hip_modem_modulate_block_dev(yagi_hip_modem q, const uint8_t *sym_dev, size_t n, yagi_cf32 *y_dev);
int yagi_hip_modem_demodulate_block(yagi_hip_modem q, const yagi_cf32 *x, size_t n, uint8_t *sym, yagi_cf32 *xhat);
int yagi_hip_modem_demodulate_block_dev(yagi_hip_modem q, const yagi_cf32 *x_dev, size_t n, uint8_t *sym_dev,
                                        yagi_cf32 *xhat_dev);
int yagi_hip_modem_demodulate_soft_block(yagi_hip_modem q, const yagi_cf32 *x, size_t n, uint8_t *sym, uint8_t *soft);
int yagi_hip_modem_demodulate_soft_block_dev(yagi_hip_modem q, const yagi_cf32 *x_dev, size_t n, uint8_t *sym_dev,
                                             uint8_t *soft_dev);

/* ---- OrdFilt: src/filter/ordfilt.rs:1-66 (order-statistic / median filter over the last n samples) ------------------
 * Only f32 (rrrf): Complex has no PartialOrd, so the reference's generic T admits nothing else.
 *   create(n, k)              new() :16-30  n == 0 and k >= n are YAGI_ERR_CONFIG with the reference's messages;
 *                             n > YAGI_ORDFILT_NMAX is YAGI_ERR_CONFIG too (the device form's LDS tile, a limit of this
 *                             build; the message names it)
 *   create_medfilt(m)         new_medfilt() :32-34 = create(2m + 1, m)
 *   clone / reset             derive(Clone) / reset() :36-38 (the window of n samples is all +0.0)
 *   get_n / get_k             the window length and the 0-based ascending rank
 *   push / write              :40-46 on the host mirror, no launch
 *   execute / execute_one     :48-58 on the host mirror, no launch: a stable sort of a copy of the window (oldest
 *                             first) under the order below, element k
 *   execute_block             :60-65 on host slices (n samples in, n out), staged through the device
 *   execute_block_dev         device buffers, asynchronous on the object's stream.  x_dev and y_dev MUST NOT OVERLAP:
 *                             a workgroup reads the n - 1 samples in front of its tile while another stores there;
 *                             overlapping ranges are YAGI_ERR_CONFIG.  n = 0 samples is a no-op.
 * Every output is a copy of one input sample (or of the +0.0 the window starts with), and equals the reference's
 * sequential loop bit for bit: -0.0 and +0.0 compare equal and the stable sort keeps the older one first, so which zero
 * comes out depends on its place in the window, here as there.
 * THE ONE DEVIATION, NaN.  The reference sorts under partial_cmp(..).unwrap_or(Equal), which is no total order once a NaN
 * is in the window: Rust's sort may then return any order, or panic.  This build compares a monotone u32 key of the
 * bits: -0.0 is folded onto +0.0, then negative floats are bit-inverted and non-negative ones get the top bit set.
 * For windows without NaN that is partial_cmp exactly.  A NaN with the sign bit clear sorts above +inf, one with it set
 * below -inf (among themselves by payload), and equal keys keep their age order.  Every window then has exactly one
 * sample of rank k whatever the input.
 *   set_kernel(choice)        which kernel the block calls run: 0 auto, 1 the LDS form (any n), 2 the register-resident
 *                             form (2 <= n <= YAGI_ORDFILT_REG_NMAX, else YAGI_ERR_CONFIG).  The forms give the same bits.
 * Device forms: ordfilt_kernels.hip; a workgroup computes YAGI_ORDFILT_TILE outputs. */
#define YAGI_ORDFILT_NMAX 1025
#define YAGI_ORDFILT_TILE 4096
#define YAGI_ORDFILT_REG_NMAX 9
typedef struct yagi_hip_ordfilt_rrrf_s *yagi_hip_ordfilt_rrrf;
int yagi_hip_ordfilt_rrrf_create(size_t n, size_t k, yagi_hip_ordfilt_rrrf *q);
int yagi_hip_ordfilt_rrrf_create_medfilt(size_t m, yagi_hip_ordfilt_rrrf *q);
int yagi_hip_ordfilt_rrrf_destroy(yagi_hip_ordfilt_rrrf q);
int yagi_hip_ordfilt_rrrf_clone(yagi_hip_ordfilt_rrrf q, yagi_hip_ordfilt_rrrf *out);
int yagi_hip_ordfilt_rrrf_set_stream(yagi_hip_ordfilt_rrrf q, yagi_stream_t s);
int yagi_hip_ordfilt_rrrf_reset(yagi_hip_ordfilt_rrrf q);
int yagi_hip_ordfilt_rrrf_set_kernel(yagi_hip_ordfilt_rrrf q, int choice);
int yagi_hip_ordfilt_rrrf_get_n(yagi_hip_ordfilt_rrrf q, size_t *n);
int yagi_hip_ordfilt_rrrf_get_k(yagi_hip_ordfilt_rrrf q, size_t *k);
int yagi_hip_ordfilt_rrrf_push(yagi_hip_ordfilt_rrrf q, float x);
int yagi_hip_ordfilt_rrrf_write(yagi_hip_ordfilt_rrrf q, const float *x, size_t n);
int yagi_hip_ordfilt_rrrf_execute(yagi_hip_ordfilt_rrrf q, float *y);
int yagi_hip_ordfilt_rrrf_execute_one(yagi_hip_ordfilt_rrrf q, float x, float *y);
int yagi_hip_ordfilt_rrrf_execute_block(yagi_hip_ordfilt_rrrf q, const float *x, size_t n, float *y);
int yagi_hip_ordfilt_rrrf_execute_block_dev(yagi_hip_ordfilt_rrrf q, const float *x_dev, size_t n, float *y_dev);

/* ---- MSequence: src/sequence/msequence.rs:41-164 (maximal-length shift-register sequence) --------------------------
 * The state is one 32-bit word on the host; no call reads anything back from the device.
 *   create(m, g, a)           new() :55-67  m outside 2..31 is YAGI_ERR_CONFIG; n = 2^m - 1.  The state starts as a,
 *                             NOT masked: like the reference, the first advance() forms its bit from the whole of the
 *                             state and the whole of g and only then masks with n.  set_state does not mask either.
 *   create_genpoly(g)         :69-77  m = the bit length of g (below 2, or 32: YAGI_ERR_CONFIG), a = 1
 *   create_default(m)         LEFT OUT: its table of generator polynomials exists only as constants of the reference's
 *                             source, which this library does not copy.  Callers pass g.
 *   clone / reset             derive(Clone) / :133-135 (the state becomes a again)
 *   advance / generate_symbol :116-131 on the host.  generate_symbol(bps), MSB first; bps > 32 is YAGI_ERR_CONFIG
 *   set_state / get_state / get_genpoly / get_genpoly_length / get_length      :138-145
 *   measure_period            :147-158, a plain host loop (the state advances by the period it returns)
 *   skip(k)                   NOT IN THE REFERENCE: the state becomes what k calls of advance() would leave, in
 *                             O(log k) on the host.  advance() is linear over GF(2) on the state word, so the object
 *                             keeps T^(2^b), b = 0 .. 63, as 32 column words each and applies those of k's set bits.
 *   generate_bits_block       n calls of advance(), one bit per byte, on a host slice (staged through the device)
 *   generate_symbols_block    sym[i] = generate_symbol(bps), bps in 1..8 (else YAGI_ERR_CONFIG): one symbol per byte,
 *                             the layout yagi_hip_modem_modulate_block_dev reads
 *   *_block_dev               the same into device buffers, asynchronous on the object's stream.  n = 0 is a no-op.
 * After a block the host state is advanced by n * bps with the same matrices, so scalar and block calls interleave
 * freely and stay on the reference's stream of bits.
 * Device form: sequence_kernels.hip; a workgroup generates YAGI_MSEQUENCE_TILE symbols. */
#define YAGI_MSEQUENCE_TILE 8192
typedef struct yagi_hip_msequence_s *yagi_hip_msequence;
int yagi_hip_msequence_create(unsigned m, unsigned g, unsigned a, yagi_hip_msequence *q);
int yagi_hip_msequence_create_genpoly(unsigned g, yagi_hip_msequence *q);
int yagi_hip_msequence_destroy(yagi_hip_msequence q);
int yagi_hip_msequence_clone(yagi_hip_msequence q, yagi_hip_msequence *out);
int yagi_hip_msequence_set_stream(yagi_hip_msequence q, yagi_stream_t s);
int yagi_hip_msequence_reset(yagi_hip_msequence q);
int yagi_hip_msequence_advance(yagi_hip_msequence q, unsigned *bit);
int yagi_hip_msequence_generate_symbol(yagi_hip_msequence q, unsigned bps, unsigned *sym);
int yagi_hip_msequence_set_state(yagi_hip_msequence q, unsigned a);
int yagi_hip_msequence_get_state(yagi_hip_msequence q, unsigned *state);
int yagi_hip_msequence_get_genpoly(yagi_hip_msequence q, unsigned *g);
int yagi_hip_msequence_get_genpoly_length(yagi_hip_msequence q, unsigned *m);
int yagi_hip_msequence_get_length(yagi_hip_msequence q, unsigned *n);
int yagi_hip_msequence_measure_period(yagi_hip_msequence q, unsigned *period);
int yagi_hip_msequence_skip(yagi_hip_msequence q, uint64_t k);
int yagi_hip_msequence_generate_bits_block(yagi_hip_msequence q, size_t n, uint8_t *bits);
int yagi_hip_msequence_generate_bits_block_dev(yagi_hip_msequence q, size_t n, uint8_t *bits_dev);
int yagi_hip_msequence_generate_symbols_block(yagi_hip_msequence q, unsigned bps, size_t n, uint8_t *sym);
int yagi_hip_msequence_generate_symbols_block_dev(yagi_hip_msequence q, unsigned bps, size_t n, uint8_t *sym_dev);

/* ---- BSequence: src/sequence/bsequence.rs:8-195 (binary sequence, sliding bit correlator) --------------------------
 * The state is the reference's word array: (num_bits + 31) / 32 words, word 0 the oldest bits and masked to the
 * num_bits_msb bits it holds, the newest bit at bit 0 of the last word.  Scalar calls run on a host mirror, the block
 * call on a device copy; the two are synchronised lazily.
 *   create(num_bits)          new() :16-30  0 is YAGI_ERR_CONFIG (the reference would index an empty vector), and so
 *                             is more than YAGI_BSEQUENCE_NMAX = 8192 bits: a limit of this library (the device
 *                             form's LDS tile), which covers the 8191 bits of m = 13
 *   create_from_msequence(ms) :81-88  ms.get_length() bits, ms advanced by as many
 *   create_ccodes(qa, qb)     :34-79  complementary codes by doubling; unequal lengths, fewer than 8 bits and a
 *                             length that is no multiple of 8 are YAGI_ERR_CONFIG
 *   clone / reset             derive(Clone) / :90-92
 *   init(v, nbytes)           :95-108  pushes num_bits bits of v, MSB first; nbytes < (num_bits + 7) / 8 is
 *                             YAGI_ERR_CONFIG (the reference would index past the slice)
 *   push / circshift          :115-134
 *   correlate(a, b, rxy)      :137-150  a is the receiver: unequal WORD counts (not bit counts) are YAGI_ERR_CONFIG, and
 *                             the correction term 32 - num_bits_msb is a's
 *   add / mul (a, b, out)     :153-176  word-wise xor / and into out; unequal word counts are YAGI_ERR_CONFIG
 *   accumulate / index / get_length    :179-194  index(i >= num_bits) is YAGI_ERR_CONFIG
 *   push_correlate_block(q, ref, sym, n, bps, rxy)   means exactly
 *                                 for i in 0..n:
 *                                     for j in bps-1 down to 0:  q.push((sym[i] >> j) & 1)
 *                                     rxy[i] = ref.correlate(q)
 *                             bps in 1..8 (else YAGI_ERR_CONFIG); bits of sym[i] above bps are ignored; ref is read as it
 *                             stands when the call is made; ref and q must have equal word counts and ref == q is
 *                             rejected (both YAGI_ERR_CONFIG).  rxy may be NULL: the call then only pushes.
 *   push_correlate_block_dev  the same on device buffers (sym_dev: n bytes, rxy_dev: n int32, not overlapping),
 *                             asynchronous on q's stream.  n = 0 is a no-op.
 * Device form: sequence_kernels.hip; a workgroup computes YAGI_BSEQUENCE_TILE outputs. */
#define YAGI_BSEQUENCE_TILE 4096
#define YAGI_BSEQUENCE_NMAX 8192
typedef struct yagi_hip_bsequence_s *yagi_hip_bsequence;
int yagi_hip_bsequence_create(size_t num_bits, yagi_hip_bsequence *q);
int yagi_hip_bsequence_create_from_msequence(yagi_hip_msequence ms, yagi_hip_bsequence *q);
int yagi_hip_bsequence_create_ccodes(yagi_hip_bsequence qa, yagi_hip_bsequence qb);
int yagi_hip_bsequence_destroy(yagi_hip_bsequence q);
int yagi_hip_bsequence_clone(yagi_hip_bsequence q, yagi_hip_bsequence *out);
int yagi_hip_bsequence_set_stream(yagi_hip_bsequence q, yagi_stream_t s);
int yagi_hip_bsequence_reset(yagi_hip_bsequence q);
int yagi_hip_bsequence_init(yagi_hip_bsequence q, const uint8_t *v, size_t nbytes);
int yagi_hip_bsequence_push(yagi_hip_bsequence q, unsigned bit);
int yagi_hip_bsequence_circshift(yagi_hip_bsequence q);
int yagi_hip_bsequence_correlate(yagi_hip_bsequence a, yagi_hip_bsequence b, int32_t *rxy);
int yagi_hip_bsequence_add(yagi_hip_bsequence a, yagi_hip_bsequence b, yagi_hip_bsequence out);
int yagi_hip_bsequence_mul(yagi_hip_bsequence a, yagi_hip_bsequence b, yagi_hip_bsequence out);
int yagi_hip_bsequence_accumulate(yagi_hip_bsequence q, unsigned *count);
int yagi_hip_bsequence_index(yagi_hip_bsequence q, size_t i, unsigned *bit);
int yagi_hip_bsequence_get_length(yagi_hip_bsequence q, size_t *num_bits);
int yagi_hip_bsequence_push_correlate_block(yagi_hip_bsequence q, yagi_hip_bsequence ref, const uint8_t *sym, size_t n,
                                            unsigned bps, int32_t *rxy);
int yagi_hip_bsequence_push_correlate_block_dev(yagi_hip_bsequence q, yagi_hip_bsequence ref, const uint8_t *sym_dev,
                                                size_t n, unsigned bps, int32_t *rxy_dev);

/* ---- Autocorr: sliding delay-conjugate correlator and window energy (src/filter/autocorr.rs is an empty file) ---------
 * The reference declares the object and leaves it empty; this library defines it as a composition of the reference's
 * buffer::Window and dotprod.  With X the stream since reset() and X[k] = 0 for k < 0, after
 * sample n was pushed
 *     w[i] = X[n - W + 1 + i],   v[i] = conj(X[n - W + 1 + i - d]),   i = 0 .. W-1
 *     rxx[n]    = dotprod(w, v): the sequential sum over i from +0.0, every product and every add rounded on its own
 *                 (no FMA), the complex product num-complex's (a.re b.re - a.im b.im, a.re b.im + a.im b.re)
 *     energy[n] = sum over i, in the same order from +0.0, of fl(fl(w[i].re^2) + fl(w[i].im^2))   (rrrf: fl(w[i]^2))
 * and every output word equals that composition bit for bit.  cccf = Complex<f32>, rrrf = f32 (conj is the identity).
 *   create(window_size, delay)  1 <= window_size <= YAGI_AUTOCORR_WMAX and delay <= YAGI_AUTOCORR_DMAX, else
 *                             YAGI_ERR_CONFIG (limits of this build: the device form's LDS tile, the carried history)
 *   clone / reset             a copy of the state / the stream starts again (all history +0.0)
 *   get_window_size / get_delay
 *   push / write              on the host mirror, no launch
 *   execute / get_energy      rxx and energy of the window as it stands, on the host mirror, no launch
 *   execute_block(x, n, rxx, energy)      pushes n samples and writes rxx[i], energy[i] after each; host slices, staged
 *                             through the device.  energy may be NULL.
 *   execute_block_dev         the same on device buffers (x_dev, rxx_dev: n elements; energy_dev: n float or NULL),
 *                             asynchronous on the object's stream.  The buffers MUST NOT OVERLAP (YAGI_ERR_CONFIG):
 *                             a workgroup reads samples in front of its tile while another stores.  n = 0 is a no-op.
 * The state is the last window_size + delay samples, carried on the device between block calls.
 * Device form: autocorr_kernels.hip; a workgroup computes YAGI_AUTOCORR_TILE outputs. */
#define YAGI_AUTOCORR_WMAX 1024
#define YAGI_AUTOCORR_DMAX 65536
#define YAGI_AUTOCORR_TILE 2048
typedef struct yagi_hip_autocorr_cccf_s *yagi_hip_autocorr_cccf;
typedef struct yagi_hip_autocorr_rrrf_s *yagi_hip_autocorr_rrrf;
#define YAGI_AUTOCORR_API(K, T)                                                                                       \
    int yagi_hip_autocorr_##K##_create(size_t window_size, size_t delay, yagi_hip_autocorr_##K *q);                    \
    int yagi_hip_autocorr_##K##_destroy(yagi_hip_autocorr_##K q);                                                      \
    int yagi_hip_autocorr_##K##_clone(yagi_hip_autocorr_##K q, yagi_hip_autocorr_##K *out);                            \
    int yagi_hip_autocorr_##K##_set_stream(yagi_hip_autocorr_##K q, yagi_stream_t s);                                  \
    int yagi_hip_autocorr_##K##_reset(yagi_hip_autocorr_##K q);                                                        \
    int yagi_hip_autocorr_##K##_get_window_size(yagi_hip_autocorr_##K q, size_t *window_size);                         \
    int yagi_hip_autocorr_##K##_get_delay(yagi_hip_autocorr_##K q, size_t *delay);                                     \
    int yagi_hip_autocorr_##K##_push(yagi_hip_autocorr_##K q, T x);                                                    \
    int yagi_hip_autocorr_##K##_write(yagi_hip_autocorr_##K q, const T *x, size_t n);                                  \
    int yagi_hip_autocorr_##K##_execute(yagi_hip_autocorr_##K q, T *rxx);                                              \
    int yagi_hip_autocorr_##K##_get_energy(yagi_hip_autocorr_##K q, float *energy);                                    \
    int yagi_hip_autocorr_##K##_execute_block(yagi_hip_autocorr_##K q, const T *x, size_t n, T *rxx, float *energy);   \
    int yagi_hip_autocorr_##K##_execute_block_dev(yagi_hip_autocorr_##K q, const T *x_dev, size_t n, T *rxx_dev,       \
                                                  float *energy_dev);
YAGI_AUTOCORR_API(cccf, yagi_cf32)
YAGI_AUTOCORR_API(rrrf, float)
#undef YAGI_AUTOCORR_API

/* ---- BurstDetector: Autocorr, a normalised threshold and run / peak extraction in one object ------------------------
 * Absent from the reference; defined by composition of what this library already pins.
 * BurstDetector<T>(W, d, threshold, energy_floor, min_length), T = Complex<f32> (cccf) or f32 (rrrf).  Let rxx[n] and
 * energy[n] be Autocorr(W, d)'s outputs on the stream since reset(), n the absolute sample index (the first sample is
 * 0), and thr2 = fl(threshold * threshold), formed once on the host.  All arithmetic is f32; every product, add and
 * quotient is rounded on its own (no FMA):
 *     m[n]   = fl(fl(re^2) + fl(im^2)) of rxx[n]                 (rrrf: fl(rxx^2))
 *     q[n]   = fl(energy[n]^2)
 *     hit[n] = energy[n] > energy_floor && m[n] > fl(thr2 * q[n])  strict, so a NaN anywhere gives no hit; at W = 1,
 *                                                                d = 0, where m = q, a threshold >= 1 never fires
 *     r[n]   = m[n] / q[n]                                       IEEE division, looked at only where hit[n]
 * A run is a maximal set of consecutive hits; its peak is the index of its largest r, the earliest on ties (+Inf
 * included).  The first non-hit after a run closes it; a run whose last hit is the last sample seen so far is pending,
 * and a later call extends or closes it.  An event is a closed run with length >= min_length.  A block call returns the
 * events its samples close, ordered by start.  However a stream is cut into calls, the concatenated list is the same,
 * but for:
 * Capacity.  Inside a call the device sees runs cut at its tiles (YAGI_AUTOCORR_TILE consecutive samples counted from
 * the call's first); call those pieces segments.  A call may hold tiles + YAGI_BURSTDET_SEGMAX segments: a burst of any
 * length costs one per tile, and SEGMAX more are free.  A call with more still pushes its samples, reports
 * overflow = 1, writes no events and drops the pending run; a run that continues into the next call starts there.
 * Events buffer.  The call reports the number of events and writes the first cap of them, as snprintf does.
 *   create(W, d, threshold, energy_floor, min_length)   W and d as for Autocorr; threshold finite and > 0, energy_floor
 *                             finite and >= 0, min_length >= 1; anything else is YAGI_ERR_CONFIG
 *   clone / reset             a copy of history, pending run and sample counter / all three cleared
 *   get_window_size / get_delay / get_threshold / get_energy_floor / get_min_length / get_position
 *   get_pending(&has, &ev)    the pending run so far (length and peak up to the last sample seen); synchronises
 *   detect_block(x, n, events, cap, &count, &overflow)   host slices, staged through the device
 *   detect_block_dev(x_dev, n, events_dev, cap, status_dev)   status_dev = uint32_t[2] {count, overflow}; asynchronous on
 *                             the object's stream, no host synchronisation.  n = 0 writes {0, 0}.  events_dev may be
 *                             NULL where cap = 0.
 *   flush(events, cap, &count)   closes the pending run, an event if it is long enough; the sample counter stays
 *   detect_host(...)          the definition on the host alone (no device needed), one call on a stream from reset():
 *                             the sequential state machine over Autocorr's host arithmetic, the capacity rule included
 * Not built: merging runs across gaps, a per-sample push, soft outputs, sharding.  A known-preamble
 * cross-correlation front end is another object: PreambleDetector, below.
 * Device form: burstdet_kernels.hip: a tile kernel and a one-workgroup stitch kernel per call; the stitch walks a
 * call's segments one by one, about 0.3 us each on an MI355X, so a block that is all burst costs milliseconds. */
#define YAGI_BURSTDET_SEGMAX 8192
typedef struct yagi_burst_event {
    uint64_t start, length, peak;            /* absolute sample indices */
    float ratio, energy, rxx_re, rxx_im;     /* r, energy and rxx at the peak; rrrf: rxx_im = +0.0 */
} yagi_burst_event;
typedef struct yagi_hip_burstdet_cccf_s *yagi_hip_burstdet_cccf;
typedef struct yagi_hip_burstdet_rrrf_s *yagi_hip_burstdet_rrrf;
#define YAGI_BURSTDET_API(K, T)                                                                                       \
    int yagi_hip_burstdet_##K##_create(size_t window_size, size_t delay, float threshold, float energy_floor,         \
                                       uint64_t min_length, yagi_hip_burstdet_##K *q);                                \
    int yagi_hip_burstdet_##K##_destroy(yagi_hip_burstdet_##K q);                                                      \
    int yagi_hip_burstdet_##K##_clone(yagi_hip_burstdet_##K q, yagi_hip_burstdet_##K *out);                            \
    int yagi_hip_burstdet_##K##_set_stream(yagi_hip_burstdet_##K q, yagi_stream_t s);                                  \
    int yagi_hip_burstdet_##K##_reset(yagi_hip_burstdet_##K q);                                                        \
    int yagi_hip_burstdet_##K##_get_window_size(yagi_hip_burstdet_##K q, size_t *window_size);                         \
    int yagi_hip_burstdet_##K##_get_delay(yagi_hip_burstdet_##K q, size_t *delay);                                     \
    int yagi_hip_burstdet_##K##_get_threshold(yagi_hip_burstdet_##K q, float *threshold);                              \
    int yagi_hip_burstdet_##K##_get_energy_floor(yagi_hip_burstdet_##K q, float *energy_floor);                        \
    int yagi_hip_burstdet_##K##_get_min_length(yagi_hip_burstdet_##K q, uint64_t *min_length);                         \
    int yagi_hip_burstdet_##K##_get_position(yagi_hip_burstdet_##K q, uint64_t *position);                             \
    int yagi_hip_burstdet_##K##_get_pending(yagi_hip_burstdet_##K q, int *has_pending, yagi_burst_event *ev);          \
    int yagi_hip_burstdet_##K##_detect_block(yagi_hip_burstdet_##K q, const T *x, size_t n, yagi_burst_event *events,  \
                                             size_t cap, size_t *count, int *overflow);                               \
    int yagi_hip_burstdet_##K##_detect_block_dev(yagi_hip_burstdet_##K q, const T *x_dev, size_t n,                    \
                                                 yagi_burst_event *events_dev, size_t cap, uint32_t *status_dev);     \
    int yagi_hip_burstdet_##K##_flush(yagi_hip_burstdet_##K q, yagi_burst_event *events, size_t cap, size_t *count);   \
    int yagi_hip_burstdet_##K##_detect_host(size_t window_size, size_t delay, float threshold, float energy_floor,    \
                                            uint64_t min_length, const T *x, size_t n, yagi_burst_event *events,      \
                                            size_t cap, size_t *count, int *overflow, int *has_pending,               \
                                            yagi_burst_event *pending);
YAGI_BURSTDET_API(cccf, yagi_cf32)
YAGI_BURSTDET_API(rrrf, float)
#undef YAGI_BURSTDET_API

/* ---- PreambleDetector: a bank of known-preamble correlators, a normalised threshold and run / peak extraction ---------
 * Absent from the reference; defined by composition of what this library already pins.
 * PreambleDetector(p[L], dphi[K], threshold, energy_floor, min_length), Complex<f32> only (cccf).  It correlates the
 * stream with the preamble p under K carrier-offset hypotheses dphi_k (radians per sample, used in the caller's order,
 * duplicates allowed) and returns events, not samples.
 * Templates, built once on the host: theta = (double)dphi_k (double)i and v_k[i] = conj(p[i]) e^{-j theta}, the four
 * products and two sums in f64 from the f32 parts of p and cos / sin of theta, each component rounded once to f32
 * (dphi_k = 0 gives conj(p) exactly).  yagi_hip_pdet_templates builds the same words without a device.
 *     thr2 = fl(threshold * threshold), formed once on the host
 *     ep   = sum over i = 0 .. L-1, from +0.0, of fl(fl(p.re^2) + fl(p.im^2)); it must be finite and > 0
 * With X the stream since reset(), X[j] = 0 for j < 0, n the absolute sample index and w[i] = X[n - L + 1 + i], all in
 * f32 and every product, add and quotient rounded on its own (no FMA):
 *     rxy_k[n]  = dotprod(w, v_k): the sequential sum over i from +0.0 of num-complex's product,
 *                 re += fl(w.re v.re) - fl(w.im v.im),  im += fl(w.re v.im) + fl(w.im v.re)
 *     energy[n] = sum over i, in the same order from +0.0, of fl(fl(w[i].re^2) + fl(w[i].im^2))   (Autocorr(L, 0)'s)
 *     m_k[n]    = fl(fl(re^2) + fl(im^2)) of rxy_k[n]
 *     kb        = 0; for k = 1 .. K-1 in order kb = k where m_k > m_kb (strict: ties keep the lowest k, a NaN m_0 stays)
 *     q[n]      = fl(energy[n] * ep)
 *     hit[n]    = energy[n] > energy_floor && m_kb > fl(thr2 * q[n])   strict, so a NaN gives no hit
 *     r[n]      = m_kb / q[n]                                         IEEE division, looked at only where hit[n]
 * r <= 1 up to rounding (Cauchy-Schwarz), so sensible thresholds lie in (0, 1).  Runs, peaks, pending run, events, the
 * chunking property, the capacity rule (tiles of YAGI_PDET_TILE samples, YAGI_PDET_SEGMAX segments beyond one per tile)
 * and the events buffer are BurstDetector's, word for word.  An event's ratio, energy, rxy and hypothesis (kb) are taken
 * at its peak: peak - (L - 1) is where the preamble starts, dphi[hypothesis] the coarse carrier offset, arg(rxy) the
 * carrier phase.
 *   create(p, L, dphi, K, threshold, energy_floor, min_length)   1 <= L <= YAGI_PDET_LMAX, 1 <= K <= YAGI_PDET_KMAX, dphi
 *                             finite, ep finite and > 0, threshold finite and > 0, energy_floor finite and >= 0,
 *                             min_length >= 1; anything else is YAGI_ERR_CONFIG, decided before any device is asked for
 *   clone / reset             a copy of history, pending run and sample counter / all three cleared
 *   get_length / get_hypotheses / get_threshold / get_energy_floor / get_min_length / get_preamble_energy (ep)
 *   get_dphi(out[K]) / get_templates(out[K L])   the hypotheses and the templates, row k = v_k
 *   get_position / get_pending(&has, &ev)   as BurstDetector's; they synchronise
 *   detect_block(x, n, events, cap, &count, &overflow)   host slices, staged through the device
 *   detect_block_dev(x_dev, n, events_dev, cap, status_dev)   status_dev = uint32_t[2] {count, overflow}; asynchronous on
 *                             the object's stream, no host synchronisation.  n = 0 writes {0, 0}.  events_dev may be
 *                             NULL where cap = 0.  The buffers MUST NOT OVERLAP (YAGI_ERR_CONFIG).
 *   correlate_block(x, n, rxy, energy)   the bank's raw output: pushes n samples like any block call (the sample counter
 *                             advances, a pending run is dropped: it could not be continued) and writes
 *                             rxy[k n + i] = rxy_k and energy[i] after sample i; energy may be NULL
 *   correlate_block_dev       the same on device buffers, which MUST NOT OVERLAP (YAGI_ERR_CONFIG); n = 0 is a no-op
 *   flush(events, cap, &count)   closes the pending run, an event if it is long enough; the sample counter stays
 *   detect_host(...)          the definition on the host alone (no device needed), one call on a stream from reset()
 * Not built: an rrrf kind, fine interpolation of timing and frequency, an FFT / overlap-save or
 * MFMA correlator, L beyond LMAX, a per-sample push, hysteresis, sharding.
 * Device form: pdet_kernels.hip: a tile kernel and a one-workgroup stitch kernel per call. */
#define YAGI_PDET_LMAX 1024
#define YAGI_PDET_KMAX 32
#define YAGI_PDET_TILE 2048
#define YAGI_PDET_SEGMAX 8192
typedef struct yagi_preamble_event {
    uint64_t start, length, peak;            /* absolute sample indices */
    float ratio, energy, rxy_re, rxy_im;     /* r, energy and rxy of the best hypothesis at the peak */
    uint32_t hypothesis, pad;                /* kb at the peak; pad = 0 */
} yagi_preamble_event;
typedef struct yagi_hip_pdet_cccf_s *yagi_hip_pdet_cccf;
int yagi_hip_pdet_templates(const yagi_cf32 *p, size_t L, const float *dphi, size_t K, yagi_cf32 *out);
int yagi_hip_pdet_cccf_create(const yagi_cf32 *p, size_t L, const float *dphi, size_t K, float threshold,
                              float energy_floor, uint64_t min_length, yagi_hip_pdet_cccf *q);
int yagi_hip_pdet_cccf_destroy(yagi_hip_pdet_cccf q);
int yagi_hip_pdet_cccf_clone(yagi_hip_pdet_cccf q, yagi_hip_pdet_cccf *out);
int yagi_hip_pdet_cccf_set_stream(yagi_hip_pdet_cccf q, yagi_stream_t s);
int yagi_hip_pdet_cccf_reset(yagi_hip_pdet_cccf q);
int yagi_hip_pdet_cccf_get_length(yagi_hip_pdet_cccf q, size_t *length);
int yagi_hip_pdet_cccf_get_hypotheses(yagi_hip_pdet_cccf q, size_t *hypotheses);
int yagi_hip_pdet_cccf_get_threshold(yagi_hip_pdet_cccf q, float *threshold);
int yagi_hip_pdet_cccf_get_energy_floor(yagi_hip_pdet_cccf q, float *energy_floor);
int yagi_hip_pdet_cccf_get_min_length(yagi_hip_pdet_cccf q, uint64_t *min_length);
int yagi_hip_pdet_cccf_get_preamble_energy(yagi_hip_pdet_cccf q, float *ep);
int yagi_hip_pdet_cccf_get_dphi(yagi_hip_pdet_cccf q, float *dphi);
int yagi_hip_pdet_cccf_get_templates(yagi_hip_pdet_cccf q, yagi_cf32 *templates);
int yagi_hip_pdet_cccf_get_position(yagi_hip_pdet_cccf q, uint64_t *position);
int yagi_hip_pdet_cccf_get_pending(yagi_hip_pdet_cccf q, int *has_pending, yagi_preamble_event *ev);
int yagi_hip_pdet_cccf_detect_block(yagi_hip_pdet_cccf q, const yagi_cf32 *x, size_t n, yagi_preamble_event *events,
                                    size_t cap, size_t *count, int *overflow);
int yagi_hip_pdet_cccf_detect_block_dev(yagi_hip_pdet_cccf q, const yagi_cf32 *x_dev, size_t n,
                                        yagi_preamble_event *events_dev, size_t cap, uint32_t *status_dev);
int yagi_hip_pdet_cccf_correlate_block(yagi_hip_pdet_cccf q, const yagi_cf32 *x, size_t n, yagi_cf32 *rxy, float *energy);
int yagi_hip_pdet_cccf_correlate_block_dev(yagi_hip_pdet_cccf q, const yagi_cf32 *x_dev, size_t n, yagi_cf32 *rxy_dev,
                                           float *energy_dev);
int yagi_hip_pdet_cccf_flush(yagi_hip_pdet_cccf q, yagi_preamble_event *events, size_t cap, size_t *count);
int yagi_hip_pdet_cccf_detect_host(const yagi_cf32 *p, size_t L, const float *dphi, size_t K, float threshold,
                                   float energy_floor, uint64_t min_length, const yagi_cf32 *x, size_t n,
                                   yagi_preamble_event *events, size_t cap, size_t *count, int *overflow,
                                   int *has_pending, yagi_preamble_event *pending);

/* ---- SymSync: symbol timing recovery for a bank of channels (src/filter/symsync.rs) ---------------------------------
 * SymSync(channels, k, npfb, h[h_len]): `channels` independent Symsync<Complex32> objects of one design (crcf only).
 * A block is x[s x_pitch + c], step s < n, channel c < channels; per channel the call writes the outputs the reference's
 * execute would write for that channel's samples, y[j y_pitch + c] for j < ny[c], bit for bit its sequential loop:
 *     new (:37-110)        dh = central differences of h with the wrap at both ends, hdh_max by the `|| i == 0` rule,
 *                          dh *= fl(0.06 / hdh_max); two FirPfbFilter::new(npfb, ., h_len) banks over one window, Ls =
 *                          h_len div npfb taps per branch; then reset(), set_lf_bw(0.01), unlock()
 *     step (:230-266)      push; while b < npfb { mf = row b . window; y = mf / Complex(k, 0) (num-complex's division);
 *                          where decim_counter == k_out: decim_counter = 0 and, unless locked, dmf = derivative row b .
 *                          window, q = clamp(Re(conj(mf) dmf), -1, 1), q_hat = the loop filter's execute_df2(q), rate +=
 *                          rate_adjustment q_hat, del = rate + q_hat, tau_decim = tau; then decim_counter += 1, tau +=
 *                          del, bf = tau npfb, b = round(bf) as usize }; tau -= 1, bf -= npfb, b -= npfb
 * all in f32, every product, add and quotient rounded on its own; the sums run oldest first from +0.0 (the sum
 * FirPfbFilter::execute forms).  reset() clears the matched filter's window and NOT the derivative filter's, as the
 * reference does (:160-172).
 * Capacity (absent from the reference, which panics where y is too short or a NaN reaches the loop): a channel writes at
 * most ycap outputs per call.  An inner-loop iteration about to store output number ycap does not run: the channel is
 * stalled (its first ycap outputs of that call are the sequential loop's).  A stalled channel ignores the rest of the
 * call's input and all later input, writes nothing, reports ny = 0, keeps get_tau, and stays so until reset() or
 * reset_channel(c).  A call returns YAGI_OK whether or not channels stalled.
 * Deviation: where hdh_max is 0 or not finite, create returns YAGI_ERR_CONFIG (the reference would build NaN taps).
 *   create(channels, k, npfb, h, h_len)   k >= 2, npfb >= 1, h_len >= 2, (h_len - 1) mod npfb = 0; limits below;
 *                             anything else is YAGI_ERR_CONFIG, decided before any device is asked for
 *   create_rnyquist(channels, ftype, k, m, beta, npfb)   (:112-131) the shapes yagi_hip_fir_design_prototype builds
 *   create_kaiser(channels, k, m, beta, npfb)            (:133-158) fc = 0.75, 40 dB, taps x fl(2 fc)
 *   rnyquist_taps / kaiser_taps   the prototypes those two design, 2 npfb k m + 1 taps; no device needed
 *   destroy / clone / set_stream / reset / reset_channel(c)
 *   lock / unlock / is_locked
 *   set_output_rate(k_out)    sets rate and del at once, for every channel
 *   set_lf_bw(bw)             (:196-213) in f32, the coefficients normalised by a0
 *   get_channels / get_branch_length (Ls)
 *   get_tau(tau[channels]) / get_stalled(stalled[channels])   they synchronise
 *   execute(x, x_pitch, n, y, y_pitch, ycap, ny[channels], stalled[channels])   host slices, staged through the device
 *   execute_dev(x_dev, x_pitch, n, y_dev, y_pitch, ycap, status_dev)   status_dev = uint32_t[2 channels]: ny, then
 *                             stalled; asynchronous on the object's stream; n = 0 writes zeros for ny
 *   execute_host(channels, k, npfb, h, h_len, k_out, bw, locked, x, x_pitch, n, y, y_pitch, ycap, ny, stalled, tau)
 *                             the definition on the host alone, one call from reset(), no device needed; tau may be NULL
 * Rows >= ny[c] of a channel are not touched.  The pitches are in samples and >= channels, so a sub-band c0 .. c0 + C of
 * an analyzer's output runs in place with pointer + c0 and pitch M.  n and ycap are below 2^31.  x and y must not overlap.
 * Not built: rrrf, per-channel designs or bandwidths, a per-channel lock mask, four lanes per
 * channel, a time-parallel form for locked objects, sharding.
 * Device form: symsync_kernels.hip: one lane per channel, one wave per workgroup. */
#define YAGI_SYMSYNC_NPFB_MAX 128
#define YAGI_SYMSYNC_LS_MAX 128
#define YAGI_SYMSYNC_CHANNELS_MAX 1048576
typedef struct yagi_hip_symsync_crcf_s *yagi_hip_symsync_crcf;
int yagi_hip_symsync_crcf_create(size_t channels, size_t k, size_t npfb, const float *h, size_t h_len,
                                 yagi_hip_symsync_crcf *q);
int yagi_hip_symsync_crcf_create_rnyquist(size_t channels, int ftype, size_t k, size_t m, float beta, size_t npfb,
                                          yagi_hip_symsync_crcf *q);
int yagi_hip_symsync_crcf_create_kaiser(size_t channels, size_t k, size_t m, float beta, size_t npfb,
                                        yagi_hip_symsync_crcf *q);
int yagi_hip_symsync_crcf_rnyquist_taps(int ftype, size_t k, size_t m, float beta, size_t npfb, float *h);
int yagi_hip_symsync_crcf_kaiser_taps(size_t k, size_t m, float beta, size_t npfb, float *h);
int yagi_hip_symsync_crcf_destroy(yagi_hip_symsync_crcf q);
int yagi_hip_symsync_crcf_clone(yagi_hip_symsync_crcf q, yagi_hip_symsync_crcf *out);
int yagi_hip_symsync_crcf_set_stream(yagi_hip_symsync_crcf q, yagi_stream_t s);
int yagi_hip_symsync_crcf_reset(yagi_hip_symsync_crcf q);
int yagi_hip_symsync_crcf_reset_channel(yagi_hip_symsync_crcf q, size_t c);
int yagi_hip_symsync_crcf_lock(yagi_hip_symsync_crcf q);
int yagi_hip_symsync_crcf_unlock(yagi_hip_symsync_crcf q);
int yagi_hip_symsync_crcf_is_locked(yagi_hip_symsync_crcf q, int *locked);
int yagi_hip_symsync_crcf_set_output_rate(yagi_hip_symsync_crcf q, size_t k_out);
int yagi_hip_symsync_crcf_set_lf_bw(yagi_hip_symsync_crcf q, float bw);
int yagi_hip_symsync_crcf_get_channels(yagi_hip_symsync_crcf q, size_t *channels);
int yagi_hip_symsync_crcf_get_branch_length(yagi_hip_symsync_crcf q, size_t *Ls);
int yagi_hip_symsync_crcf_get_tau(yagi_hip_symsync_crcf q, float *tau);
int yagi_hip_symsync_crcf_get_stalled(yagi_hip_symsync_crcf q, uint32_t *stalled);
int yagi_hip_symsync_crcf_execute(yagi_hip_symsync_crcf q, const yagi_cf32 *x, size_t x_pitch, size_t n, yagi_cf32 *y,
                                  size_t y_pitch, size_t ycap, uint32_t *ny, uint32_t *stalled);
int yagi_hip_symsync_crcf_execute_dev(yagi_hip_symsync_crcf q, const yagi_cf32 *x_dev, size_t x_pitch, size_t n,
                                      yagi_cf32 *y_dev, size_t y_pitch, size_t ycap, uint32_t *status_dev);
int yagi_hip_symsync_crcf_execute_host(size_t channels, size_t k, size_t npfb, const float *h, size_t h_len, size_t k_out,
                                       float bw, int locked, const yagi_cf32 *x, size_t x_pitch, size_t n, yagi_cf32 *y,
                                       size_t y_pitch, size_t ycap, uint32_t *ny, uint32_t *stalled, float *tau);

/* ---- EqLms: LMS equalizer for a bank of channels (src/equalization/eqlms.rs) -----------------------------------------
 * EqLms(channels, h[h_len] or NULL): `channels` independent Eqlms<Complex32> objects of one design (cccf only).  A block
 * is x[s x_pitch + c], step s, channel c < channels; per channel every output word and every weight equals the
 * reference's sequential loop, in f32 with every product, sum and quotient rounded on its own:
 *     execute (:137-140)   y = sum_i conj(w0[i]) r[i] over the window oldest first, num-complex's product (re = a.re b.re
 *                          - a.im b.im, im = a.re b.im + a.im b.re with a = (w.re, -w.im)), folded from Complex(0, 0)
 *     push(x) (:125-129)   the window takes x; x2_n = x.re x.re - x.im (-x.im); x2_sum += x2_n - x2_0, x2_0 the value
 *                          pushed h_len pushes earlier (the same expression on the sample that leaves the window, which
 *                          is how the device forms it); x2_sum is a running f32 sum and part of the state, never
 *                          recomputed from the window; count += 1
 *     step(d, d_hat) (:170-187)   nothing while count < h_len; else alpha = d - d_hat and, for every tap, w0[i] = w0[i] +
 *                          ((mu conj(alpha)) r[i]) / x2_sum: an f32-times-complex scaling, the full complex product, a
 *                          true IEEE division per component.  x2_sum = 0 or NaN gives that channel Inf / NaN weights
 *     step_blind(d_hat) (:189-192)   d = d_hat / |d_hat| componentwise, then step(d, d_hat); d_hat = 0 gives NaN
 * Deviation 1, |z|: the reference calls the platform's hypotf, which is not one fixed word.  The library defines
 * |z| = (float)sqrt((double)re (double)re + (double)im (double)im), on the device and on the host (DESIGN.md section 4
 * records how often that differs from this platform's hypotf).
 * Deviation 2, DECISION: the desired symbol is table[j], j the FIRST index that minimises (y.re - t.re)^2 + (y.im -
 * t.im)^2 with unfused terms, only a strictly smaller value replacing the best.  It is the library's own rule, the one
 * Modem's Arb hard decision uses, NOT the reference's Modem::get_demodulator_sample.
 *   create(channels, h, h_len)   h0[i] = conj(h[h_len - 1 - i]); h = NULL: h0[h_len / 2] = 1.  h_len = 0 is
 *                             YAGI_ERR_CONFIG as in the reference; limits below; decided before any device is asked for
 *   create_rnyquist(channels, ftype, k, m, beta, dt)   (:51-76) k >= 2, m >= 1, beta in [0, 1], dt in [-1, 1];
 *                             h = fir_design_prototype(ftype, k, m, beta, dt) / fl(k), h_len = 2 k m + 1
 *   create_lowpass(channels, h_len, fc)   (:78-90) h_len >= 1, fc in [0, 0.5]; h = fir_design_kaiser(h_len, fc, 40, 0)
 *                             x 2 x fc, the imaginary part the reference's (h 0) fc
 *   destroy / clone / set_stream / reset / reset_channel(c)
 *   set_bw(mu) / get_bw       mu < 0 is YAGI_ERR_CONFIG; one value for the bank, 0.5 after create
 *   get_length / get_channels
 *   get_coefficients(out[channels][h_len])   w0;   get_weights: w0 reversed and conjugated.  They synchronise
 *   set_constellation(table, M)   DECISION's table, 1 <= M <= YAGI_EQLMS_TABLE_MAX, copied
 *   execute_block(k, x, x_pitch, n, y, y_pitch)   (:153-168) per row: push, y[s] = execute(), and step_blind(y[s]) where
 *                             (count + k - 1) mod k = 0; count carries across calls.  k >= 1
 *   decim_block(k, mode, x, x_pitch, n, d, d_pitch, y, y_pitch)   n rows in, a multiple of k; per symbol i < n / k:
 *                             decim_execute (:142-151: push x[i k], y[i] = execute(), push the other k - 1 rows), THEN one
 *                             update, so the gradient uses the shifted window and the later x2_sum (the order of the
 *                             reference's testbench).  mode: YAGI_EQLMS_NONE no update; TRAIN step(d[i d_pitch + c], y);
 *                             BLIND step_blind(y); DECISION step(table[j], y).  d is read by TRAIN only
 *   execute_block_dev / decim_block_dev   the same on device pointers, asynchronous on the object's stream
 *   execute_host(channels, h, h_len, mu, call, k, x, x_pitch, n, d, d_pitch, table, M, y, y_pitch, w0)   the definition on
 *                             the host alone, one call from reset(), no device needed; call = a mode for decim_block or
 *                             YAGI_EQLMS_EXECUTE for execute_block; w0[channels][h_len] may be NULL
 * Every result is independent of how the stream is cut into calls.  The pitches are in samples and >= channels; n is below
 * 2^31.  x, d and y must not overlap.
 * Not built: rrrf, per-channel designs or step sizes, sharding.
 * Device form: eqlms_kernels.hip: one lane per channel, one wave per workgroup. */
#define YAGI_EQLMS_LEN_MAX 128
#define YAGI_EQLMS_CHANNELS_MAX 1048576
#define YAGI_EQLMS_TABLE_MAX 256
enum { YAGI_EQLMS_NONE = 0, YAGI_EQLMS_TRAIN = 1, YAGI_EQLMS_BLIND = 2, YAGI_EQLMS_DECISION = 3, YAGI_EQLMS_EXECUTE = 4 };
typedef struct yagi_hip_eqlms_cccf_s *yagi_hip_eqlms_cccf;
int yagi_hip_eqlms_cccf_create(size_t channels, const yagi_cf32 *h, size_t h_len, yagi_hip_eqlms_cccf *q);
int yagi_hip_eqlms_cccf_create_rnyquist(size_t channels, int ftype, size_t k, size_t m, float beta, float dt,
                                        yagi_hip_eqlms_cccf *q);
int yagi_hip_eqlms_cccf_create_lowpass(size_t channels, size_t h_len, float fc, yagi_hip_eqlms_cccf *q);
int yagi_hip_eqlms_cccf_destroy(yagi_hip_eqlms_cccf q);
int yagi_hip_eqlms_cccf_clone(yagi_hip_eqlms_cccf q, yagi_hip_eqlms_cccf *out);
int yagi_hip_eqlms_cccf_set_stream(yagi_hip_eqlms_cccf q, yagi_stream_t s);
int yagi_hip_eqlms_cccf_reset(yagi_hip_eqlms_cccf q);
int yagi_hip_eqlms_cccf_reset_channel(yagi_hip_eqlms_cccf q, size_t c);
int yagi_hip_eqlms_cccf_set_bw(yagi_hip_eqlms_cccf q, float mu);
int yagi_hip_eqlms_cccf_get_bw(yagi_hip_eqlms_cccf q, float *mu);
int yagi_hip_eqlms_cccf_get_length(yagi_hip_eqlms_cccf q, size_t *h_len);
int yagi_hip_eqlms_cccf_get_channels(yagi_hip_eqlms_cccf q, size_t *channels);
int yagi_hip_eqlms_cccf_get_coefficients(yagi_hip_eqlms_cccf q, yagi_cf32 *w0);
int yagi_hip_eqlms_cccf_get_weights(yagi_hip_eqlms_cccf q, yagi_cf32 *w);
int yagi_hip_eqlms_cccf_set_constellation(yagi_hip_eqlms_cccf q, const yagi_cf32 *table, size_t M);
int yagi_hip_eqlms_cccf_execute_block(yagi_hip_eqlms_cccf q, size_t k, const yagi_cf32 *x, size_t x_pitch, size_t n,
                                      yagi_cf32 *y, size_t y_pitch);
int yagi_hip_eqlms_cccf_execute_block_dev(yagi_hip_eqlms_cccf q, size_t k, const yagi_cf32 *x_dev, size_t x_pitch, size_t n,
                                          yagi_cf32 *y_dev, size_t y_pitch);
int yagi_hip_eqlms_cccf_decim_block(yagi_hip_eqlms_cccf q, size_t k, int mode, const yagi_cf32 *x, size_t x_pitch, size_t n,
                                    const yagi_cf32 *d, size_t d_pitch, yagi_cf32 *y, size_t y_pitch);
int yagi_hip_eqlms_cccf_decim_block_dev(yagi_hip_eqlms_cccf q, size_t k, int mode, const yagi_cf32 *x_dev, size_t x_pitch,
                                        size_t n, const yagi_cf32 *d_dev, size_t d_pitch, yagi_cf32 *y_dev, size_t y_pitch);
int yagi_hip_eqlms_cccf_execute_host(size_t channels, const yagi_cf32 *h, size_t h_len, float mu, int call, size_t k,
                                     const yagi_cf32 *x, size_t x_pitch, size_t n, const yagi_cf32 *d, size_t d_pitch,
                                     const yagi_cf32 *table, size_t M, yagi_cf32 *y, size_t y_pitch, yagi_cf32 *w0);

/* ---- EqRls: recursive-least-squares equalizer for a bank of channels (src/equalization/eqrls.rs) --------------------
 * EqRls(channels, h[p] or NULL, p): `channels` independent Eqrls<Complex32> objects of one design (cccf only).  A block is
 * x[s x_pitch + c], step s, channel c < channels; per channel every output word and every word of w0, w1 and P0 equals
 * the reference's sequential loop, in f32 with every product, sum and quotient rounded on its own (no FMA).  Products
 * and quotients are num-complex's: a b = (a.re b.re - a.im b.im, a.re b.im + a.im b.re); a / b = ((a.re b.re + a.im b.im)
 * / n, (a.im b.re - a.re b.im) / n) with n = b.re b.re + b.im b.im; sums fold from Complex(0, 0).
 *     new (:31-62)         h0 = h as given (no reversal, no conjugate, unlike Eqlms); h = NULL: h0[p - 1] = 1;
 *                          lambda = 0.99f, delta = 0.1f, w1 = 0
 *     reset (:76-88)       P0 = diag(1.0f / 0.1f), w0 = h0, the window zeroed; w1 is NOT touched
 *     execute (:106-110)   y = sum_i w0[i] r[i] over the window oldest first, NO conjugate
 *     step(d, d_hat) (:112-146)   no buf_full gate, it updates from the first sample.  x = the window, oldest first:
 *                          alpha = d - d_hat;  xp0[c] = sum_r x[r] P0[r][c];  zeta = (sum_c xp0[c] conj(x[c])) +
 *                          Complex(lambda, 0);  g[r] = (sum_c P0[r][c] conj(x[c])) / zeta;  gxl[r][c] = (g[r] x[c]) /
 *                          Complex(lambda, 0), the full complex quotient (n = lambda lambda + 0 0, re = (a.re lambda +
 *                          a.im 0) / n), not a.re / lambda;  gxlp0[r][c] = sum_i gxl[r][i] P0[i][c], the p^3 term, never
 *                          regrouped;  P1 = P0 / Complex(lambda, 0) - gxlp0;  w1[i] = w0[i] + alpha g[i];  w0 = w1, P0 = P1
 * Every division is a true IEEE f32 division.  A NaN or Inf sample or a singular zeta changes its own channel only; there
 * is no stall state.
 *   create(channels, h, p)    p = 0 is YAGI_ERR_CONFIG as in the reference; 1 <= p <= YAGI_EQRLS_LEN_MAX, 1 <= channels <=
 *                             YAGI_EQRLS_CHANNELS_MAX and channels p p <= 2^26 (512 MiB of P), decided before any device
 *                             is asked for
 *   recreate(h, p)            (:64-74) the same p: h0 = h where h is given, NOTHING else changes (no reset); another p: a
 *                             new object of the same channel count, stream and constellation (lambda back to 0.99f)
 *   destroy / clone / set_stream / reset / reset_channel(c)
 *   set_bw(lambda) / get_bw   lambda outside [0, 1] or NaN is YAGI_ERR_CONFIG; lambda = 0 is accepted and gives the bank
 *                             Inf / NaN, as in the reference; one value for the bank
 *   get_length / get_channels
 *   get_coefficients(out[channels][p])   w0.   get_weights(out[channels][p])   w1 REVERSED (:148-156), not w0: zero between
 *                             create and the first update, and after reset() still the weights from before the reset.
 *                             The library reproduces this.   get_matrix(out[channels][p][p])   P0.   They synchronise
 *   set_constellation(table, M)   DECISION's table, 1 <= M <= YAGI_EQLMS_TABLE_MAX, copied
 *   step_block(k, mode, x, x_pitch, n, d, d_pitch, y, y_pitch)   n rows in, a multiple of k >= 1; per symbol i < n / k:
 *                             push x[i k], y[i] = execute(), the update, THEN push the other k - 1 rows.  The update
 *                             comes BEFORE the trailing pushes, because the gain must be formed from the window that
 *                             produced d_hat (the reference's train, :169-173, is push, execute, step).  This differs
 *                             from EqLms.decim_block, which updates after them.  mode: YAGI_EQRLS_NONE no update; TRAIN
 *                             step(d[i d_pitch + c], y); DECISION step(table[j], y) with EqLms's decision rule (its
 *                             deviation 2).  d is read by TRAIN only
 *   train(w[channels][p], x, x_pitch, n, d, d_pitch)   (:158-176) n < p is YAGI_ERR_CONFIG; reset(), w0[i] = w[p - 1 - i],
 *                             n TRAIN steps at k = 1 (the outputs are dropped), get_weights written back into w
 *   step_block_dev / train_dev   the same on device pointers, asynchronous on the object's stream; train_dev's w is a
 *                             HOST array, read before the launch, and is not written: call get_weights afterwards
 *   execute_host(channels, h, p, lambda, mode, k, x, x_pitch, n, d, d_pitch, table, M, y, y_pitch, w0, w1, P0)   the
 *                             definition on the host alone, one call from reset(), no device needed; w0, w1[channels][p]
 *                             and P0[channels][p][p] may be NULL
 *   plan(channels, p, L, lds_bytes, admissible)   the launch shape: L lanes share one channel's step (a power of two), a
 *                             wave holds 64 / L channels in lds_bytes of LDS; bit b of admissible = (L = 2^b may be set)
 *   set_lanes(L) / get_lanes  override the planner; 0 gives the choice back to it.  For every admissible L the results
 *                             are the same words
 * Every result is independent of how the stream is cut into calls.  The pitches are in samples and >= channels; n is below
 * 2^31.  x, d and y must not overlap.
 * Not built: rrrf, blind (CM) updates, per-channel lambda or designs, an O(p^2) regrouped recursion (it changes the
 * words), SymTrack with an RLS equalizer, sharding.
 * Device form: eqrls_kernels.hip: L lanes per channel, one wave per workgroup. */
#define YAGI_EQRLS_LEN_MAX 32
#define YAGI_EQRLS_CHANNELS_MAX 1048576
#define YAGI_EQRLS_MATRIX_MAX 67108864 /* channels p p */
enum { YAGI_EQRLS_NONE = 0, YAGI_EQRLS_TRAIN = 1, YAGI_EQRLS_DECISION = 3 };   /* numbered as YAGI_EQLMS_* */
typedef struct yagi_hip_eqrls_cccf_s *yagi_hip_eqrls_cccf;
int yagi_hip_eqrls_cccf_create(size_t channels, const yagi_cf32 *h, size_t p, yagi_hip_eqrls_cccf *q);
int yagi_hip_eqrls_cccf_recreate(yagi_hip_eqrls_cccf q, const yagi_cf32 *h, size_t p);
int yagi_hip_eqrls_cccf_destroy(yagi_hip_eqrls_cccf q);
int yagi_hip_eqrls_cccf_clone(yagi_hip_eqrls_cccf q, yagi_hip_eqrls_cccf *out);
int yagi_hip_eqrls_cccf_set_stream(yagi_hip_eqrls_cccf q, yagi_stream_t s);
int yagi_hip_eqrls_cccf_reset(yagi_hip_eqrls_cccf q);
int yagi_hip_eqrls_cccf_reset_channel(yagi_hip_eqrls_cccf q, size_t c);
int yagi_hip_eqrls_cccf_set_bw(yagi_hip_eqrls_cccf q, float lambda);
int yagi_hip_eqrls_cccf_get_bw(yagi_hip_eqrls_cccf q, float *lambda);
int yagi_hip_eqrls_cccf_get_length(yagi_hip_eqrls_cccf q, size_t *p);
int yagi_hip_eqrls_cccf_get_channels(yagi_hip_eqrls_cccf q, size_t *channels);
int yagi_hip_eqrls_cccf_get_coefficients(yagi_hip_eqrls_cccf q, yagi_cf32 *w0);
int yagi_hip_eqrls_cccf_get_weights(yagi_hip_eqrls_cccf q, yagi_cf32 *w);
int yagi_hip_eqrls_cccf_get_matrix(yagi_hip_eqrls_cccf q, yagi_cf32 *P0);
int yagi_hip_eqrls_cccf_set_constellation(yagi_hip_eqrls_cccf q, const yagi_cf32 *table, size_t M);
int yagi_hip_eqrls_cccf_set_lanes(yagi_hip_eqrls_cccf q, size_t L);
int yagi_hip_eqrls_cccf_get_lanes(yagi_hip_eqrls_cccf q, size_t *L);
int yagi_hip_eqrls_cccf_step_block(yagi_hip_eqrls_cccf q, size_t k, int mode, const yagi_cf32 *x, size_t x_pitch, size_t n,
                                   const yagi_cf32 *d, size_t d_pitch, yagi_cf32 *y, size_t y_pitch);
int yagi_hip_eqrls_cccf_step_block_dev(yagi_hip_eqrls_cccf q, size_t k, int mode, const yagi_cf32 *x_dev, size_t x_pitch,
                                       size_t n, const yagi_cf32 *d_dev, size_t d_pitch, yagi_cf32 *y_dev, size_t y_pitch);
int yagi_hip_eqrls_cccf_train(yagi_hip_eqrls_cccf q, yagi_cf32 *w, const yagi_cf32 *x, size_t x_pitch, size_t n,
                              const yagi_cf32 *d, size_t d_pitch);
int yagi_hip_eqrls_cccf_train_dev(yagi_hip_eqrls_cccf q, const yagi_cf32 *w, const yagi_cf32 *x_dev, size_t x_pitch, size_t n,
                                  const yagi_cf32 *d_dev, size_t d_pitch);
int yagi_hip_eqrls_cccf_execute_host(size_t channels, const yagi_cf32 *h, size_t p, float lambda, int mode, size_t k,
                                     const yagi_cf32 *x, size_t x_pitch, size_t n, const yagi_cf32 *d, size_t d_pitch,
                                     const yagi_cf32 *table, size_t M, yagi_cf32 *y, size_t y_pitch, yagi_cf32 *w0,
                                     yagi_cf32 *w1, yagi_cf32 *P0);
int yagi_hip_eqrls_plan(size_t channels, size_t p, size_t *L, size_t *lds_bytes, unsigned *admissible);

/* ---- Agc: automatic gain control for a bank of channels (src/agc/agc.rs) ---------------------------------------------
 * Agc(channels): `channels` independent Agc<T> objects of one set of settings, T = Complex<f32> (crcf) or f32 (rrrf).  A
 * block is x[s x_pitch + c], step s < n, channel c < channels; per channel every output word, gain and squelch mode
 * equals the reference's sequential loop, in f32 with every product and sum rounded on its own:
 *     execute (:71-89)     y = x g (both components); y2 = (y conj y).re = re re - im (-im) (rrrf: y y);
 *                          y2' = (1 - alpha) y2' + alpha y2;
 *                          locked: the output is y, NOT scaled (the reference returns before `* scale`), nothing else
 *                          changes; else where y2' > 1e-6: g = g yg_expf(-0.5 alpha yg_lnf(y2')), the argument formed
 *                          left to right in f32; g = minNum(g, 1e6) (Rust's f32::min: a NaN g would become 1e6);
 *                          squelch_update_mode; the output is y scale
 *     squelch_update_mode (:212-248)   hi = (-20 yg_log10f(g) > threshold); Enabled -> hi ? Rise : Enabled; Rise -> hi ?
 *                          SignalHi : Fall; SignalHi -> hi ? SignalHi : Fall; Fall -> timer = timeout, hi ? SignalHi :
 *                          SignalLo; SignalLo -> timer -= 1, timer = 0 ? Timeout : hi ? SignalHi : SignalLo; Timeout ->
 *                          Enabled; Disabled stays
 *     reset (:60-69)       g = 1, y2' = 1, unlocked, mode -> Enabled unless Disabled
 *     init(x) (:171-178)   per channel the f32 sum of |x|^2 (the expression of y2) in row order from +0; then
 *                          g = 1 / (sqrt(sum / fl(n)) + 1e-16) in f32, y2' = 1
 * The three words.  The reference calls the platform's ln, exp and log10, which are not fixed words.  The library
 * defines each as the f32 rounding of an f64 evaluation made of IEEE f64 + - * / only, each rounded on its own and none
 * fused, integer and bit operations on the exponent, and the f64 literals below (agc_words.hpp; the same source runs on
 * the host and on the device, and tests/agc_ref.py restates it in Python floats):
 *     ln64(x), x a positive finite f32 as f64:  x = 2^e m with m in [1, 2) from the bits; where m >= fl(sqrt 2): m = m / 2,
 *         e = e + 1.  s = (m - 1) / (m + 1); z = s s; p = 1/23; then for k = 21, 19, .. 3, 1: p = p z + fl(1 / k).
 *         ln64 = fl(e) LN2 + (2 s) p, LN2 = 0x1.62e42fefa39efp-1
 *     yg_lnf(x) = (float)ln64(x); yg_log10f(x) = (float)(ln64(x) 0x1.bcb7b1526e50ep-2).  Special arguments of both: a
 *         NaN or x < 0 gives NaN; either zero gives -inf; +inf gives +inf; subnormal f32 are normal f64
 *     exp64(x), x not a NaN:  x = min(max(x, -110), 95) (beyond the clamp the f32 word is 0 or inf anyway, and 2^k stays
 *         a normal f64); t = x 0x1.71547652b82fep+0 + 0.5; k = floor(t); r = (x - k HI) - k LO with HI =
 *         0x1.62e42feep-1, LO = 0x1.a39ef35793c76p-33; p = fl(1 / 14!); then for j = 13, 12, .. 1, 0: p = p r + fl(1 / j!).
 *         exp64 = p 2^k (exact)
 *     yg_expf(x) = (float)exp64(x); NaN gives NaN, -inf gives +0, +inf gives +inf; subnormal results come from the one
 *         f64 -> f32 rounding
 *     set_rssi's 10^(-rssi / 20) = (float)exp64((double)fl32(-rssi / 20) 0x1.26bb1bbb55516p+1), host only
 * yagi_hip_lnf / expf / log10f(x, n, y) run the words over arrays on the host.
 * Deviations: squelch_set_timeout(0) is YAGI_ERR_CONFIG (the reference's usize timer would underflow in SignalLo) and
 * timeouts are below 2^32.  set_gain, set_gains, set_signal_level and set_scale accept v > 0 only, so a NaN is
 * YAGI_ERR_CONFIG too (the reference tests `v <= 0.0`, which lets a NaN through); set_bandwidth rejects a NaN as the
 * reference does.  Otherwise non-finite samples follow the loop as written: a NaN in y2' stays there and
 * freezes g; such samples change only their own channel.
 *   create(channels)          bandwidth 0.01, scale 1, squelch disabled, threshold 0, timeout 100 (:37-58);
 *                             1 <= channels <= YAGI_AGC_CHANNELS_MAX, decided before any device is asked for
 *   destroy / clone / set_stream / reset / reset_channel(c)
 *   lock / unlock             every channel;  is_locked: 1 where every channel is locked
 *   set_locked(locked[channels]) / get_locked(locked[channels])   per channel, nonzero = locked
 *   set_bandwidth(bt) / get_bandwidth   bt in [0, 1], alpha = bt;  set_scale / get_scale   scale > 0
 *   set_gain(g) (g > 0; y2' stays) / set_signal_level(x2) (x2 > 0: g = 1 / x2, y2' = 1) / set_rssi(rssi) (g =
 *                             maxNum(10^(-rssi / 20), 1e-16), y2' = 1): every channel
 *   set_gains(g[channels])    per channel, all > 0
 *   get_gain(g[channels]) / get_signal_level (1 / g) / get_rssi (-20 yg_log10f(g))   they synchronise
 *   squelch_enable (every mode = Enabled) / squelch_disable / squelch_is_enabled
 *   squelch_set_threshold / squelch_get_threshold, squelch_set_timeout / squelch_get_timeout
 *   squelch_get_status(mode[channels])   YAGI_AGC_SQUELCH_*; synchronises
 *   init(x, x_pitch, n) / init_dev   n = 0 is YAGI_ERR_CONFIG; they synchronise
 *   execute_block(x, x_pitch, n, y, y_pitch, status, status_pitch)   host slices, staged through the device
 *   execute_block_dev(...)    device pointers, asynchronous on the object's stream.  status = uint8_t [n][status_pitch],
 *                             the squelch mode after each sample, or NULL
 *   execute_host(channels, bandwidth, scale, g0, locked, squelch, threshold, timeout, x, x_pitch, n, y, y_pitch, status,
 *                status_pitch, g_out, mode_out)   the definition on the host alone, one call from reset() followed by
 *                             set_gain(g0); no device needed; status, g_out[channels], mode_out[channels] may be NULL
 * The pitches are in elements and >= channels; n is below 2^31; n = 0 touches nothing.  y == x with y_pitch == x_pitch
 * runs in place; any other overlap of x and y, and any overlap of the status plane with x or y, is YAGI_ERR_CONFIG.
 * Not built: per-channel bandwidths or thresholds, a time-parallel form.
 * Device form: agc_kernels.hip: one lane per channel, one wave per workgroup. */
#define YAGI_AGC_CHANNELS_MAX 1048576
enum {
    YAGI_AGC_SQUELCH_DISABLED = 0, YAGI_AGC_SQUELCH_ENABLED, YAGI_AGC_SQUELCH_RISE, YAGI_AGC_SQUELCH_SIGNALHI,
    YAGI_AGC_SQUELCH_FALL, YAGI_AGC_SQUELCH_SIGNALLO, YAGI_AGC_SQUELCH_TIMEOUT
};
int yagi_hip_lnf(const float *x, size_t n, float *y);
int yagi_hip_expf(const float *x, size_t n, float *y);
int yagi_hip_log10f(const float *x, size_t n, float *y);
#define YAGI_HIP_AGC_DECL(K, T)                                                                                          \
    typedef struct yagi_hip_agc_##K##_s *yagi_hip_agc_##K;                                                               \
    int yagi_hip_agc_##K##_create(size_t channels, yagi_hip_agc_##K *q);                                                 \
    int yagi_hip_agc_##K##_destroy(yagi_hip_agc_##K q);                                                                  \
    int yagi_hip_agc_##K##_clone(yagi_hip_agc_##K q, yagi_hip_agc_##K *out);                                             \
    int yagi_hip_agc_##K##_set_stream(yagi_hip_agc_##K q, yagi_stream_t s);                                              \
    int yagi_hip_agc_##K##_reset(yagi_hip_agc_##K q);                                                                    \
    int yagi_hip_agc_##K##_reset_channel(yagi_hip_agc_##K q, size_t c);                                                  \
    int yagi_hip_agc_##K##_lock(yagi_hip_agc_##K q);                                                                     \
    int yagi_hip_agc_##K##_unlock(yagi_hip_agc_##K q);                                                                   \
    int yagi_hip_agc_##K##_is_locked(yagi_hip_agc_##K q, int *locked);                                                   \
    int yagi_hip_agc_##K##_set_locked(yagi_hip_agc_##K q, const uint8_t *locked);                                        \
    int yagi_hip_agc_##K##_get_locked(yagi_hip_agc_##K q, uint8_t *locked);                                              \
    int yagi_hip_agc_##K##_set_bandwidth(yagi_hip_agc_##K q, float bt);                                                  \
    int yagi_hip_agc_##K##_get_bandwidth(yagi_hip_agc_##K q, float *bt);                                                 \
    int yagi_hip_agc_##K##_set_scale(yagi_hip_agc_##K q, float scale);                                                   \
    int yagi_hip_agc_##K##_get_scale(yagi_hip_agc_##K q, float *scale);                                                  \
    int yagi_hip_agc_##K##_set_gain(yagi_hip_agc_##K q, float gain);                                                     \
    int yagi_hip_agc_##K##_set_signal_level(yagi_hip_agc_##K q, float x2);                                               \
    int yagi_hip_agc_##K##_set_rssi(yagi_hip_agc_##K q, float rssi);                                                     \
    int yagi_hip_agc_##K##_set_gains(yagi_hip_agc_##K q, const float *gain);                                             \
    int yagi_hip_agc_##K##_get_gain(yagi_hip_agc_##K q, float *gain);                                                    \
    int yagi_hip_agc_##K##_get_signal_level(yagi_hip_agc_##K q, float *level);                                           \
    int yagi_hip_agc_##K##_get_rssi(yagi_hip_agc_##K q, float *rssi);                                                    \
    int yagi_hip_agc_##K##_get_channels(yagi_hip_agc_##K q, size_t *channels);                                           \
    int yagi_hip_agc_##K##_squelch_enable(yagi_hip_agc_##K q);                                                           \
    int yagi_hip_agc_##K##_squelch_disable(yagi_hip_agc_##K q);                                                          \
    int yagi_hip_agc_##K##_squelch_is_enabled(yagi_hip_agc_##K q, int *enabled);                                         \
    int yagi_hip_agc_##K##_squelch_set_threshold(yagi_hip_agc_##K q, float threshold);                                   \
    int yagi_hip_agc_##K##_squelch_get_threshold(yagi_hip_agc_##K q, float *threshold);                                  \
    int yagi_hip_agc_##K##_squelch_set_timeout(yagi_hip_agc_##K q, uint64_t timeout);                                    \
    int yagi_hip_agc_##K##_squelch_get_timeout(yagi_hip_agc_##K q, uint64_t *timeout);                                   \
    int yagi_hip_agc_##K##_squelch_get_status(yagi_hip_agc_##K q, uint8_t *mode);                                        \
    int yagi_hip_agc_##K##_init(yagi_hip_agc_##K q, const T *x, size_t x_pitch, size_t n);                               \
    int yagi_hip_agc_##K##_init_dev(yagi_hip_agc_##K q, const T *x_dev, size_t x_pitch, size_t n);                       \
    int yagi_hip_agc_##K##_execute_block(yagi_hip_agc_##K q, const T *x, size_t x_pitch, size_t n, T *y, size_t y_pitch, \
                                         uint8_t *status, size_t status_pitch);                                          \
    int yagi_hip_agc_##K##_execute_block_dev(yagi_hip_agc_##K q, const T *x_dev, size_t x_pitch, size_t n, T *y_dev,     \
                                             size_t y_pitch, uint8_t *status_dev, size_t status_pitch);                  \
    int yagi_hip_agc_##K##_execute_host(size_t channels, float bandwidth, float scale, float g0, int locked, int squelch, \
                                        float threshold, uint64_t timeout, const T *x, size_t x_pitch, size_t n, T *y,   \
                                        size_t y_pitch, uint8_t *status, size_t status_pitch, float *g_out,              \
                                        uint8_t *mode_out);
YAGI_HIP_AGC_DECL(crcf, yagi_cf32)
YAGI_HIP_AGC_DECL(rrrf, float)
#undef YAGI_HIP_AGC_DECL

/* ---- SymTrack: agc, timing, carrier and equalizer loops for a bank of channels (src/framing/symtrack.rs is an empty file)
 * SymTrack(channels, ftype, k, m, beta, scheme, osc_scheme, npfb, eq_len): `channels` independent receivers of one design
 * (cccf only).  The reference file is empty, so the object is defined by composition of objects this library pins to the
 * reference.  It follows liquid-dsp's symtrack as recalled; that is a note, not a parity claim.
 * SymTrack: the definition.  Per channel the object owns
 *     agc    Agc<Complex32> as after new() (crcf), squelch disabled
 *     sync   Symsync<Complex32>::new_rnyquist(ftype, k, m, beta, npfb), then set_output_rate(2)
 *     nco    Osc::new(osc_scheme), YAGI_OSC_NCO or YAGI_OSC_VCO, phase and frequency 0
 *     eq     Eqlms<Complex32>::new_lowpass(eq_len, 0.45)
 *     demod  Modem of `scheme` (or of a table)
 * set_bandwidth(bw), bw >= 0, 0.9 at creation: agc.set_bandwidth(0.02 bw), sync.set_lf_bw(0.001 bw), eq.set_bw(0.02 bw),
 * nco.pll_set_bandwidth(0.001 bw), the products formed in f32; a value one of the four setters refuses is YAGI_ERR_CONFIG.
 * execute over one input sample x of a channel:
 *     v = agc.execute(x)
 *     for each output s the synchroniser's step(v) produces, in order (0, 1 or more):
 *         u = nco.mix_down(s); nco.step()
 *         eq.push(u)
 *         j = sync_index; sync_index += 1
 *         if j is odd: continue                      (outputs 0, 2, 4, .. since reset are the symbol instants)
 *         d_hat = eq.execute()
 *         sym = demod.demodulate(d_hat); x_hat = demod.get_demodulator_sample()
 *         e = demod.get_demodulator_phase_error()    ((d_hat conj(x_hat)).im, num-complex's product, unfused)
 *         nco.pll_step(e)                            (adjust_frequency(e alpha); adjust_phase(e beta), through constrain())
 *         if num_syms > eq_holdoff and strategy != OFF:
 *             d = d_hat / |d_hat| (CM: EqLms's own |.| word and quotients) or x_hat (DD)
 *             eq.step(d, d_hat)                      (behind eq's own count >= h_len gate)
 *         num_syms += 1
 *         emit (d_hat, sym)
 * eq_holdoff is 200 and the strategy CM at creation.  All in f32 with the words of the parts: Agc's own ln and exp, SymSync's
 * sums and quotients, Osc's table lookup, EqLms's sums, |.| and quotients, Modem's hard decision.
 * Schemes: BPSK, QPSK, OOK, ASK2 .. ASK256, QAM4 .. QAM256 and tables of 2 .. 256 points (a power of two).  PSK and DPSK
 * decide through the device library's atan2f / sincosf, which are not fixed words: create returns YAGI_ERR_CONFIG for them.
 * Hard decisions only.
 * Deviations:
 *   capacity   a channel writes at most ycap symbols per call.  An iteration about to emit symbol number ycap does not run:
 *              the channel is stalled, reason YAGI_SYMTRACK_STALL_CAPACITY (SymSync's rule; the sample's agc step and the
 *              synchroniser's push have run).  The inner loop is counted, so it ends whatever the state holds.
 *   constrain  the reference never returns for an infinity or a magnitude at which +- 2 pi makes no progress.  A pll_step
 *              whose argument e alpha or e beta has magnitude >= YAGI_SYMTRACK_PLL_ARG_MAX does not run, nor anything
 *              behind it in that iteration (no eq.step, no count, no output): the channel is stalled, reason
 *              YAGI_SYMTRACK_STALL_PLL.  Below the bound constrain is the reference's loops, NaN -> 0 as Rust's cast.
 *   stalled    a stalled channel ignores all further input, reports ny = 0, keeps its getters and revives on reset() or
 *              reset_channel(c).  A call returns YAGI_OK either way.  Non-finite samples otherwise follow the loops as
 *              written and touch only their own channel.
 *   create(channels, ftype, k, m, beta, scheme, osc_scheme, npfb, eq_len)   channels <= YAGI_SYMTRACK_CHANNELS_MAX, k >= 2,
 *                             npfb and 2 k m within SymSync's limits, 1 <= eq_len <= YAGI_EQLMS_LEN_MAX, and the LDS of the
 *                             lane-strided tiles (the synchroniser's window, the equalizer's window and weights, the staged
 *                             rows) plus the oscillator table and the constellation within 160 KiB; anything else is
 *                             YAGI_ERR_CONFIG, decided before any device is asked for
 *   create_from_table(channels, ftype, k, m, beta, table, M, osc_scheme, npfb, eq_len)
 *   destroy / clone / set_stream / reset / reset_channel(c)
 *   set_bandwidth(bw) / get_bandwidth
 *   set_bandwidths(agc, sync, eq, pll)   the four setters one by one (get_bandwidth then reports NaN)
 *   set_eq_strategy(YAGI_SYMTRACK_EQ_OFF | _CM | _DD) / set_eq_holdoff(nsyms)
 *   set_nco(c, frequency, phase) / set_nco_all(frequency[channels], phase[channels])   through constrain(): YAGI_ERR_CONFIG
 *                             where the reference's loops would not end
 *   get_channels; and, synchronising, [channels] each: get_tau, get_gain, get_rssi, get_nco_frequency, get_nco_phase
 *                             (Osc's f32 formulas), get_nco_state(theta, d_theta) (the raw words), get_num_syms (uint64_t),
 *                             get_stalled (the reason, 0 = running); get_weights(w[channels][eq_len]) as EqLms's
 *   execute(x, x_pitch, n, y, y_pitch, sym, sym_pitch, ycap, ny[channels], stalled[channels])   host slices; sym may be NULL
 *   execute_dev(x_dev, x_pitch, n, y_dev, y_pitch, sym_dev, sym_pitch, ycap, status_dev)   status_dev = uint32_t[3 channels]:
 *                             ny, then the stall reason, then the low word of num_syms; asynchronous on the object's
 *                             stream; n = 0 writes zeros for ny; sym_dev may be NULL
 *   execute_host(channels, ftype, k, m, beta, scheme, table, M, osc_scheme, npfb, eq_len, bw, strategy, holdoff,
 *                nco_frequency, nco_phase, x, x_pitch, n, y, y_pitch, sym, sym_pitch, ycap, ny, stalled)
 *                             the definition on the host alone, one call from reset(), no device needed; table = NULL takes
 *                             `scheme`; nco_frequency / nco_phase [channels] may be NULL (zeros)
 * y[j y_pitch + c] = d_hat and sym[j sym_pitch + c] = the symbol as one byte, j < ny[c]; rows >= ny[c] of a channel are not
 * touched.  The pitches are in elements and >= channels.  n and ycap are below 2^31.  x and y must not overlap.
 * Not built: PSK / DPSK and soft bits, rrrf, per-channel designs or bandwidths, squelch, several
 * lanes per channel, a fused channelizer -> SymTrack, sharding, Eqrls.
 * Device form: symtrack_kernels.hip: one lane per channel, one wave per workgroup. */
#define YAGI_SYMTRACK_CHANNELS_MAX 1048576
#define YAGI_SYMTRACK_PLL_ARG_MAX 256.0f
enum { YAGI_SYMTRACK_EQ_OFF = 0, YAGI_SYMTRACK_EQ_CM = 1, YAGI_SYMTRACK_EQ_DD = 2 };
enum { YAGI_SYMTRACK_STALL_NONE = 0, YAGI_SYMTRACK_STALL_CAPACITY = 1, YAGI_SYMTRACK_STALL_PLL = 2 };
typedef struct yagi_hip_symtrack_cccf_s *yagi_hip_symtrack_cccf;
int yagi_hip_symtrack_cccf_create(size_t channels, int ftype, size_t k, size_t m, float beta, int scheme, int osc_scheme,
                                  size_t npfb, size_t eq_len, yagi_hip_symtrack_cccf *q);
int yagi_hip_symtrack_cccf_create_from_table(size_t channels, int ftype, size_t k, size_t m, float beta,
                                             const yagi_cf32 *table, size_t M, int osc_scheme, size_t npfb, size_t eq_len,
                                             yagi_hip_symtrack_cccf *q);
int yagi_hip_symtrack_cccf_destroy(yagi_hip_symtrack_cccf q);
int yagi_hip_symtrack_cccf_clone(yagi_hip_symtrack_cccf q, yagi_hip_symtrack_cccf *out);
int yagi_hip_symtrack_cccf_set_stream(yagi_hip_symtrack_cccf q, yagi_stream_t s);
int yagi_hip_symtrack_cccf_reset(yagi_hip_symtrack_cccf q);
int yagi_hip_symtrack_cccf_reset_channel(yagi_hip_symtrack_cccf q, size_t c);
int yagi_hip_symtrack_cccf_set_bandwidth(yagi_hip_symtrack_cccf q, float bw);
int yagi_hip_symtrack_cccf_get_bandwidth(yagi_hip_symtrack_cccf q, float *bw);
int yagi_hip_symtrack_cccf_set_bandwidths(yagi_hip_symtrack_cccf q, float agc, float sync, float eq, float pll);
int yagi_hip_symtrack_cccf_set_eq_strategy(yagi_hip_symtrack_cccf q, int strategy);
int yagi_hip_symtrack_cccf_set_eq_holdoff(yagi_hip_symtrack_cccf q, uint64_t nsyms);
int yagi_hip_symtrack_cccf_set_nco(yagi_hip_symtrack_cccf q, size_t c, float frequency, float phase);
int yagi_hip_symtrack_cccf_set_nco_all(yagi_hip_symtrack_cccf q, const float *frequency, const float *phase);
int yagi_hip_symtrack_cccf_get_channels(yagi_hip_symtrack_cccf q, size_t *channels);
int yagi_hip_symtrack_cccf_get_tau(yagi_hip_symtrack_cccf q, float *tau);
int yagi_hip_symtrack_cccf_get_gain(yagi_hip_symtrack_cccf q, float *gain);
int yagi_hip_symtrack_cccf_get_rssi(yagi_hip_symtrack_cccf q, float *rssi);
int yagi_hip_symtrack_cccf_get_nco_frequency(yagi_hip_symtrack_cccf q, float *frequency);
int yagi_hip_symtrack_cccf_get_nco_phase(yagi_hip_symtrack_cccf q, float *phase);
int yagi_hip_symtrack_cccf_get_nco_state(yagi_hip_symtrack_cccf q, uint32_t *theta, uint32_t *d_theta);
int yagi_hip_symtrack_cccf_get_weights(yagi_hip_symtrack_cccf q, yagi_cf32 *w);
int yagi_hip_symtrack_cccf_get_num_syms(yagi_hip_symtrack_cccf q, uint64_t *num_syms);
int yagi_hip_symtrack_cccf_get_stalled(yagi_hip_symtrack_cccf q, uint32_t *stalled);
int yagi_hip_symtrack_cccf_execute(yagi_hip_symtrack_cccf q, const yagi_cf32 *x, size_t x_pitch, size_t n, yagi_cf32 *y,
                                   size_t y_pitch, uint8_t *sym, size_t sym_pitch, size_t ycap, uint32_t *ny,
                                   uint32_t *stalled);
int yagi_hip_symtrack_cccf_execute_dev(yagi_hip_symtrack_cccf q, const yagi_cf32 *x_dev, size_t x_pitch, size_t n,
                                       yagi_cf32 *y_dev, size_t y_pitch, uint8_t *sym_dev, size_t sym_pitch, size_t ycap,
                                       uint32_t *status_dev);
int yagi_hip_symtrack_cccf_execute_host(size_t channels, int ftype, size_t k, size_t m, float beta, int scheme,
                                        const yagi_cf32 *table, size_t M, int osc_scheme, size_t npfb, size_t eq_len, float bw,
                                        int strategy, uint64_t holdoff, const float *nco_frequency, const float *nco_phase,
                                        const yagi_cf32 *x, size_t x_pitch, size_t n, yagi_cf32 *y, size_t y_pitch,
                                        uint8_t *sym, size_t sym_pitch, size_t ycap, uint32_t *ny, uint32_t *stalled);

/* ---- Channel (channel_cccf): multipath, carrier offset and AWGN for a bank of links ----------------------------------
 * The reference's src/channel/mod.rs is an empty module, so the object is defined here from parts this library already
 * pins.  Channel(channels, L, osc_scheme) is `channels` independent links of one shape; the input is x[s x_pitch + c],
 * the output y[s y_pitch + c], one output per input; the broadcast form reads one stream x[s] for every link.
 * Channel: the definition.  Per link c, per input sample x at that link's sample counter t (a u64, 0 after reset):
 *     win.push(x)                                   Window<Complex32> of length L, zero after reset
 *     v = sum_{j=0..L-1} hrev_c[j] * win.read()[j]  hrev_c[j] = h_c[L-1-j]; oldest sample first; sequential from 0;
 *                                                   num-complex's product (hr xr - hi xi, hr xi + hi xr); every product
 *                                                   and add rounded on its own in f32
 *     w = nco_c.mix_up(v); nco_c.step()             Osc's words (NCO or VCO, fixed at creation); the phase of sample j of
 *                                                   a call is theta_c + (u32)j d_theta_c
 *     y.re = w.re gamma_c + nstd_c (R C)
 *     y.im = w.im gamma_c + nstd_c (R S)            four products, two adds, each rounded on its own
 *     t += 1
 * The order (multipath, carrier offset, gain and noise) follows liquid-dsp's channel_cccf as recalled; that could not be
 * checked against its source, so this is a note and no parity claim.
 * The noise words (channel_words.hpp, one source for host and device; tests/channel_ref.py restates them):
 *     seed_c = splitmix64_at(seed, c)               the synthetic-input generator's function (splitmix.hpp)
 *     a = splitmix64_at(seed_c, 2t), b = splitmix64_at(seed_c, 2t+1)       u64 arithmetic, wrapping
 *     k1 = (a >> 40) + 1 in [1, 2^24];  k2 = b >> 40 in [0, 2^24)
 *     R = (float)sqrt(-ln64((double)k1 2^-24))      ln64 of the Agc block; an f64 root; k1 = 2^24 gives -0, which is kept
 *     (C, S) = the f32 roundings of f64 evaluations of cos and sin(2 pi k2 / 2^24):  oct = k2 >> 21, r = k2 & (2^21 - 1),
 *         m = 2^21 - r in an odd octant, else r;  x = fl(m) 0x1.921fb54442d18p-22;  z = x x;
 *         p = fl(-1/15!); then p = p z + c for c = fl(1/13!), fl(-1/11!), fl(1/9!), fl(-1/7!), fl(1/5!), fl(-1/3!);
 *         sn = x + (x z) p;  q = fl(1/16!); then q = q z + c for c = fl(-1/14!), fl(1/12!), fl(-1/10!), fl(1/8!),
 *         fl(-1/6!), fl(1/4!), -1/2;  cs = 1 + z q;  ss = 0 - sn in an odd octant, else sn;  quad = ((oct + 1) >> 1) & 3:
 *         (C, S) = (cs, ss), (0 - ss, cs), (0 - cs, 0 - ss), (ss, 0 - cs) for quad = 0, 1, 2, 3.
 *         Every operation is an IEEE f64 + - * rounded on its own; the f64 error is at most E = 2^-45
 *         (YAGI_CHANNEL_COSSIN_E); k2 = 0, 2^22, 2^23, 3 2^22 give exactly (1, 0), (0, 1), (-1, 0), (0, -1).
 *     With these words E|R (C + jS)|^2 = 1, so nstd^2 is the noise power.
 * Where nstd_c is zero and both w gamma_c parts are nonzero the noise term is a signed zero that changes no bit; the
 * implementation skips the draw there.  Non-finite samples follow the words as written: they touch only their own link
 * and only the L outputs whose window holds them.
 *   create(channels, L, osc_scheme)   1 <= channels <= YAGI_CHANNEL_CHANNELS_MAX, 1 <= L <= YAGI_CHANNEL_TAPS_MAX,
 *                             YAGI_OSC_NCO or YAGI_OSC_VCO; anything else is YAGI_ERR_CONFIG, decided before any device is
 *                             asked for.  h_c = (1, 0, .., 0), gamma 1, nstd 0, offset and phase 0, seed 0, t = 0
 *   destroy / clone / set_stream    a clone writes what its original would write
 *   reset / reset_channel(c)  clears the window, t = 0, the oscillator back to the phi last set; the parameters stay
 *   set_awgn(c, n0_db, snr_db) / set_awgn_all(n0_db[channels], snr_db[channels])   nstd = p10(n0_db / 20), gamma =
 *                             p10((snr_db + n0_db) / 20), the argument formed in f32, p10(t) = (float)exp64((double)t LN10),
 *                             LN10 = 0x1.26bb1bbb55516p+1 (Agc's set_rssi word); a NaN argument gives a NaN word
 *   set_gain_noise(c, gamma, nstd) / set_gain_noise_all   the raw words, any f32
 *   set_carrier_offset(c, dphi, phi) / set_carrier_offset_all   Osc's set_frequency and set_phase, constrain() included:
 *                             YAGI_ERR_CONFIG where the reference's loops would not end; then nothing is changed
 *   set_multipath(c, h[L]) / set_multipath_all(h[channels][L]) / get_multipath(h[channels][L])
 *   set_seed(seed) / get_seed;  set_position(c, t) / set_position_all(t[channels])   seek the noise, t a u64
 *   get_gain_noise(gamma[channels], nstd[channels]) / get_osc_state(theta[channels], d_theta[channels]) /
 *   get_position(t[channels]) / get_channels / get_taps (L)   either output pointer of a pair may be NULL
 *   execute(x, x_pitch, n, y, y_pitch) / execute_dev   host slices staged through the device / device pointers,
 *                             asynchronous on the object's stream
 *   execute_bcast(x[n], n, y, y_pitch) / execute_bcast_dev   one input stream goes to every link
 *   execute_host(channels, L, osc_scheme, bcast, seed, h[channels][L], gamma, nstd, theta, d_theta, t (each [channels]),
 *                x, x_pitch, n, y, y_pitch)   the definition on the host alone, one call from reset() with the raw words
 *                             given; no device needed; x_pitch is ignored where bcast
 *   set_shape(links, rows) / get_shape / yagi_hip_channel_plan   the launch arrangement: a workgroup of 256 lanes is
 *                             `links` links wide (a power of two, 1 .. 64) and 256 / links steps deep, and a lane writes
 *                             `rows` outputs (1, 2, 4, 8, 16).  set_shape(0, 0) returns to the planner.  Every
 *                             admissible arrangement gives the same words.  plan reports the arrangement, the steps per
 *                             tile and the LDS bytes of a call (bcast or not) of n steps.
 * The pitches are in elements and >= channels; n is below 2^31; n = 0 touches nothing; x and y must not overlap; device
 * sample pointers are 8-byte aligned.
 * Not built: shadowing, time-varying taps, per-link L, rrrf, fusion with SymStream or Agc.
 * Device form: channel_kernels.hip. */
#define YAGI_CHANNEL_CHANNELS_MAX 1048576
#define YAGI_CHANNEL_TAPS_MAX 64      /* (16 rows x 256 lanes + 63 halo rows x 64 links + 64 x 64 taps) x 8 B + 16 KiB: 112 KiB of LDS */
#define YAGI_CHANNEL_COSSIN_E 0x1p-45
typedef struct yagi_hip_channel_cccf_s *yagi_hip_channel_cccf;
typedef struct {
    unsigned links, rows;        /* links per workgroup row; outputs per lane */
    size_t tile_steps, lds_bytes;
} yagi_hip_channel_shape;
int yagi_hip_channel_plan(size_t channels, size_t L, size_t n, int osc_scheme, int bcast, yagi_hip_channel_shape *plan);
int yagi_hip_channel_cccf_create(size_t channels, size_t L, int osc_scheme, yagi_hip_channel_cccf *q);
int yagi_hip_channel_cccf_destroy(yagi_hip_channel_cccf q);
int yagi_hip_channel_cccf_clone(yagi_hip_channel_cccf q, yagi_hip_channel_cccf *out);
int yagi_hip_channel_cccf_set_stream(yagi_hip_channel_cccf q, yagi_stream_t s);
int yagi_hip_channel_cccf_reset(yagi_hip_channel_cccf q);
int yagi_hip_channel_cccf_reset_channel(yagi_hip_channel_cccf q, size_t c);
int yagi_hip_channel_cccf_set_awgn(yagi_hip_channel_cccf q, size_t c, float n0_db, float snr_db);
int yagi_hip_channel_cccf_set_awgn_all(yagi_hip_channel_cccf q, const float *n0_db, const float *snr_db);
int yagi_hip_channel_cccf_set_gain_noise(yagi_hip_channel_cccf q, size_t c, float gamma, float nstd);
int yagi_hip_channel_cccf_set_gain_noise_all(yagi_hip_channel_cccf q, const float *gamma, const float *nstd);
int yagi_hip_channel_cccf_set_carrier_offset(yagi_hip_channel_cccf q, size_t c, float dphi, float phi);
int yagi_hip_channel_cccf_set_carrier_offset_all(yagi_hip_channel_cccf q, const float *dphi, const float *phi);
int yagi_hip_channel_cccf_set_multipath(yagi_hip_channel_cccf q, size_t c, const yagi_cf32 *h);
int yagi_hip_channel_cccf_set_multipath_all(yagi_hip_channel_cccf q, const yagi_cf32 *h);
int yagi_hip_channel_cccf_get_multipath(yagi_hip_channel_cccf q, yagi_cf32 *h);
int yagi_hip_channel_cccf_set_seed(yagi_hip_channel_cccf q, uint64_t seed);
int yagi_hip_channel_cccf_get_seed(yagi_hip_channel_cccf q, uint64_t *seed);
int yagi_hip_channel_cccf_set_position(yagi_hip_channel_cccf q, size_t c, uint64_t t);
int yagi_hip_channel_cccf_set_position_all(yagi_hip_channel_cccf q, const uint64_t *t);
int yagi_hip_channel_cccf_get_position(yagi_hip_channel_cccf q, uint64_t *t);
int yagi_hip_channel_cccf_get_gain_noise(yagi_hip_channel_cccf q, float *gamma, float *nstd);
int yagi_hip_channel_cccf_get_osc_state(yagi_hip_channel_cccf q, uint32_t *theta, uint32_t *d_theta);
int yagi_hip_channel_cccf_get_channels(yagi_hip_channel_cccf q, size_t *channels);
int yagi_hip_channel_cccf_get_taps(yagi_hip_channel_cccf q, size_t *L);
int yagi_hip_channel_cccf_set_shape(yagi_hip_channel_cccf q, unsigned links, unsigned rows);
int yagi_hip_channel_cccf_get_shape(yagi_hip_channel_cccf q, size_t n, int bcast, yagi_hip_channel_shape *shape);
int yagi_hip_channel_cccf_execute(yagi_hip_channel_cccf q, const yagi_cf32 *x, size_t x_pitch, size_t n, yagi_cf32 *y,
                                  size_t y_pitch);
int yagi_hip_channel_cccf_execute_dev(yagi_hip_channel_cccf q, const yagi_cf32 *x_dev, size_t x_pitch, size_t n,
                                      yagi_cf32 *y_dev, size_t y_pitch);
int yagi_hip_channel_cccf_execute_bcast(yagi_hip_channel_cccf q, const yagi_cf32 *x, size_t n, yagi_cf32 *y, size_t y_pitch);
int yagi_hip_channel_cccf_execute_bcast_dev(yagi_hip_channel_cccf q, const yagi_cf32 *x_dev, size_t n, yagi_cf32 *y_dev,
                                            size_t y_pitch);
int yagi_hip_channel_cccf_execute_host(size_t channels, size_t L, int osc_scheme, int bcast, uint64_t seed, const yagi_cf32 *h,
                                       const float *gamma, const float *nstd, const uint32_t *theta, const uint32_t *d_theta,
                                       const uint64_t *t, const yagi_cf32 *x, size_t x_pitch, size_t n, yagi_cf32 *y,
                                       size_t y_pitch);
/* the words on arrays, host only: awgn's (gamma, nstd); (C, S)[k2] as f64 before the f32 rounding; R[k1]; the noise of
 * (seed, link) at counters first .. first + n - 1 */
int yagi_hip_channel_awgn_words(float n0_db, float snr_db, float *gamma, float *nstd);
int yagi_hip_channel_cos_sin(const uint32_t *k2, size_t n, double *c, double *s);
int yagi_hip_channel_radius(const uint32_t *k1, size_t n, float *r);
int yagi_hip_channel_noise(uint64_t seed, uint64_t link, uint64_t first, size_t n, yagi_cf32 *out);
int yagi_hip_channel_constrain(float phi, uint32_t *word);      /* Osc's constrain(): the word of a phase or frequency */

/* ---- ConvCode: convolutional encoder and Viterbi decoder for a bank of frames ------------------------------------------
 * The reference's src/fec/mod.rs is an empty module, so the object is defined here.  ConvCode(K, g[R], P[R][p],
 * terminated) holds a code; every call works on F frames, one per row: frame f starts at byte f * pitch.  No call
 * carries state from one call to the next.
 * ConvCode: the definition.  3 <= K <= 9, S = 2^(K-1) states; 2 <= R <= 4 generator words, 0 < g[r] < 2^K.
 *   encoder     sr = 0; per input bit b: sr = ((sr << 1) | b) & (2^K - 1); output bit r = parity(sr & g[r]), r = 0 .. R-1.
 *               Message bits come most significant bit first from packed bytes; `terminated` appends K - 1 zero bits:
 *               T = n + K - 1 trellis steps, else T = n.
 *   puncturing  optional R x p matrix of 0 / 1 (row r = generator r, p <= 32), given row major; bit (step t, output r) is
 *               kept iff P[r][t mod p] == 1; every column keeps at least one bit; kept bits follow in (t, r) order.
 *               ncoded(n) = (T / p) kp + (kept bits of the columns below T mod p), kp the kept bits of a period.
 *   coded       one byte per kept bit: the encoder writes 0 or 1; the decoder reads soft bytes s = 0 .. 255, 255 a
 *               confident 1 (Modem's soft bits).
 *   decoder     path metrics are u32, the smallest wins; pm[0] = 0, pm[s] = 2^30 otherwise.  At step t the new state ns has
 *               input bit b = ns & 1 and the predecessors p0 = ns >> 1, p1 = p0 | 2^(K-2).  The branch cost from p is the
 *               sum over the kept outputs r of (e ? 255 - s : s), e = parity(((p << 1) | b) & g[r]), s that position's
 *               soft byte; punctured positions add nothing.  m0 = pm[p0] + c0, m1 = pm[p1] + c1; d[t][ns] = (m1 < m0)
 *               (a tie keeps p0); pm'[ns] = d ? m1 : m0.  The end state is 0 where terminated, else the state of the
 *               smallest metric, the lowest index on a tie.  Traceback from the end state e for t = T-1 .. 0: bit t =
 *               e & 1; e = (e >> 1) | (d[t][e] << (K-2)).  The first n bits are the message, packed most significant
 *               bit first into ceil(n / 8) bytes, pad bits zero.  metric = the end state's pm.  T <= 65536 and a step
 *               adds at most 1020, so no sum reaches 2^31 and nothing is renormalised.
 * Catastrophic codes are not detected.
 *   create(K, g, R, puncture, p, terminated)   puncture may be NULL (then p is ignored); anything outside the limits
 *                             above is YAGI_ERR_CONFIG, decided before any device is asked for
 *   destroy / clone / set_stream
 *   get_K / get_R / get_rate(kept, p) (kp kept bits per p steps; R and 1 where not punctured) / get_ncoded(n, &count) /
 *   get_nmax   the longest message: the decisions of a frame, T S / 8 bytes, fit YAGI_CONVCODE_DECISION_BYTES and
 *                             T <= YAGI_CONVCODE_STEPS_MAX; a longer frame, or n = 0, is YAGI_ERR_CONFIG
 *   encode_block(msg, msg_pitch, n, F, coded, coded_pitch)   F rows of ceil(n / 8) message bytes (pad bits ignored) ->
 *                             F rows of ncoded(n) bytes
 *   decode_block(soft, soft_pitch, n, F, msg, msg_pitch, metric)   F rows of ncoded(n) soft bytes -> F rows of
 *                             ceil(n / 8) bytes; metric, where not NULL, receives one u32 per frame
 *   encode_block_dev / decode_block_dev   device pointers, asynchronous on the object's stream
 *   encode_host / decode_host   the definition's sequential loops on the host alone; no device needed
 *   set_shape(frames_per_wave, waves) / get_shape / yagi_hip_convcode_plan   the decoder's launch arrangement.  A lane
 *                             holds states_per_lane = max(1, S / 64) states; a wave holds frames_per_wave frames (a power
 *                             of two, max(1, 8 / S) .. max(1, 64 / S)); a workgroup is 1, 2 or 4 waves; the soft bytes are
 *                             staged chunk_steps steps at a time.  set_shape(0, 0) returns to the planner.  Every
 *                             admissible arrangement gives the same bytes; one whose LDS does not hold a call's frames
 *                             is YAGI_ERR_CONFIG at that call.
 * The pitches are in bytes and at least the row length; F <= YAGI_CONVCODE_FRAMES_MAX; F = 0 touches nothing; the
 * operands of a _dev call must not overlap; a device metric pointer is 4-byte aligned.  The decoder loads the soft bytes
 * as the aligned 4-byte words that contain them.
 * Not built: lane-per-frame arrangement, decisions in global memory, sliding-window traceback,
 * parallel traceback, tail-biting, [step][channel] soft input, block codes.  Descrambling, interleaving and a CRC fused
 * around this code are Packetizer's (below).
 * Device form: convcode_kernels.hip. */
#define YAGI_CONVCODE_DECISION_BYTES 131072
#define YAGI_CONVCODE_STEPS_MAX 65536
#define YAGI_CONVCODE_FRAMES_MAX 1048576
#define YAGI_CONVCODE_PERIOD_MAX 32
typedef struct yagi_hip_convcode_s *yagi_hip_convcode;
typedef struct {
    unsigned frames_per_wave, waves, states_per_lane, chunk_steps;
    size_t frames_per_wg, lds_bytes;
} yagi_hip_convcode_shape;
int yagi_hip_convcode_plan(int K, int terminated, size_t n, size_t F, yagi_hip_convcode_shape *plan);
int yagi_hip_convcode_create(int K, const unsigned *g, int R, const uint8_t *puncture, int p, int terminated,
                             yagi_hip_convcode *q);
int yagi_hip_convcode_destroy(yagi_hip_convcode q);
int yagi_hip_convcode_clone(yagi_hip_convcode q, yagi_hip_convcode *out);
int yagi_hip_convcode_set_stream(yagi_hip_convcode q, yagi_stream_t s);
int yagi_hip_convcode_get_K(yagi_hip_convcode q, int *K);
int yagi_hip_convcode_get_R(yagi_hip_convcode q, int *R);
int yagi_hip_convcode_get_rate(yagi_hip_convcode q, size_t *kept, size_t *p);
int yagi_hip_convcode_get_ncoded(yagi_hip_convcode q, size_t n, size_t *ncoded);
int yagi_hip_convcode_get_nmax(yagi_hip_convcode q, size_t *nmax);
int yagi_hip_convcode_set_shape(yagi_hip_convcode q, unsigned frames_per_wave, unsigned waves);
int yagi_hip_convcode_get_shape(yagi_hip_convcode q, size_t n, size_t F, yagi_hip_convcode_shape *shape);
int yagi_hip_convcode_encode_block(yagi_hip_convcode q, const uint8_t *msg, size_t msg_pitch, size_t n, size_t F,
                                   uint8_t *coded, size_t coded_pitch);
int yagi_hip_convcode_encode_block_dev(yagi_hip_convcode q, const uint8_t *msg_dev, size_t msg_pitch, size_t n, size_t F,
                                       uint8_t *coded_dev, size_t coded_pitch);
int yagi_hip_convcode_decode_block(yagi_hip_convcode q, const uint8_t *soft, size_t soft_pitch, size_t n, size_t F,
                                   uint8_t *msg, size_t msg_pitch, uint32_t *metric);
int yagi_hip_convcode_decode_block_dev(yagi_hip_convcode q, const uint8_t *soft_dev, size_t soft_pitch, size_t n, size_t F,
                                       uint8_t *msg_dev, size_t msg_pitch, uint32_t *metric_dev);
int yagi_hip_convcode_encode_host(int K, const unsigned *g, int R, const uint8_t *puncture, int p, int terminated,
                                  const uint8_t *msg, size_t msg_pitch, size_t n, size_t F, uint8_t *coded,
                                  size_t coded_pitch);
int yagi_hip_convcode_decode_host(int K, const unsigned *g, int R, const uint8_t *puncture, int p, int terminated,
                                  const uint8_t *soft, size_t soft_pitch, size_t n, size_t F, uint8_t *msg, size_t msg_pitch,
                                  uint32_t *metric);
/* ncoded(n) and nmax of a code on the host alone; either output pointer may be NULL (n is checked only for ncoded) */
int yagi_hip_convcode_ncoded_host(int K, int R, const uint8_t *puncture, int p, int terminated, size_t n, size_t *ncoded,
                                  size_t *nmax);

/* ---- Packetizer: CRC, ConvCode, block interleaver and scrambler for a bank of frames, one launch per direction ------------
 * The reference has the scrambler (src/random/scramble.rs: scramble_data, unscramble_data, unscramble_data_soft) and an
 * empty fec module, so the rest is defined here.  Packetizer(n, crc, K, g[R], P[R][p], terminated, columns, scramble) turns
 * n >= 1 payload bytes per frame into a plane of transmit bits and soft bytes back into payloads with a `valid` flag; every
 * call works on F frames, one per row: frame f starts at byte f * pitch.  No call carries state.  All of it is integer
 * arithmetic: there is no tolerance anywhere.
 * Packetizer: the definition.
 *   CRC         five schemes in the Rocksoft model (width, poly, init, reflected in and out, xorout; the value on the nine
 *               bytes "123456789"):
 *                 YAGI_CRC_NONE   0   -            -            -    -            -
 *                 YAGI_CRC_8      8   0x07         0x00         no   0x00         0xF4
 *                 YAGI_CRC_16    16   0x1021       0xFFFF       no   0x0000       0x29B1
 *                 YAGI_CRC_24    24   0x864CFB     0xB704CE     no   0x000000     0x21CF02
 *                 YAGI_CRC_32    32   0x04C11DB7   0xFFFFFFFF   yes  0xFFFFFFFF   0xCBF43926
 *               The CRC of the n payload bytes follows them as w = width / 8 bytes, most significant byte first.  The
 *               message is these 8 (n + w) bits, most significant bit first; more than the code's get_nmax is
 *               YAGI_ERR_CONFIG.
 *   code        ConvCode's definition, unchanged: K, g, puncturing, terminated.  N = ncoded(8 (n + w)) coded bits in coder
 *               order i = 0 .. N-1.
 *   interleaver 1 <= columns = C <= YAGI_PACKETIZER_COLUMNS_MAX.  Coder-order bit i sits at row i div C, column i mod C of a
 *               matrix of C columns; transmission is column by column; the cells the last row lacks are skipped.  With
 *               q = N div C, r = N mod C the transmit position is pi(i) = (i mod C) q + min(i mod C, r) + i div C; its
 *               inverse, for j < r (q + 1): c = j div (q + 1), rho = j mod (q + 1); else c = r + (j - r (q + 1)) div q,
 *               rho = (j - r (q + 1)) mod q; i = rho C + c.  C = 1 and C >= N are the identity.  N = 7, C = 3 transmits
 *               0 3 6 1 4 2 5.
 *   scrambler   where scramble != 0, transmit bit j is XORed with m(j) = (MASK[(j div 8) mod 4] >> (7 - j mod 8)) & 1,
 *               MASK = CA CC 53 5F (scramble.rs :2-5); the receiver replaces the soft byte s at j by 255 - s where
 *               m(j) = 1.  On packed bytes this is scramble_data, on whole groups of eight soft bytes
 *               unscramble_data_soft.  The reference's soft routine leaves a trailing group of fewer than eight bytes
 *               alone (chunks_exact) while its packed routine masks the last byte whole; the Packetizer masks every bit
 *               j < N, so its two directions agree at every N.
 *   transmit    encode_block(payload, bps), 1 <= bps <= 8, writes nsym(bps) = ceil(N / bps) bytes per frame, each holding
 *               bps consecutive transmit bits, the first uppermost; the missing bits of the last symbol are 0.  bps = 1 is
 *               ConvCode's byte per bit; bps = 2 is what Modem(Qpsk).modulate_block takes.
 *   receive     decode_block(soft): rows of at least N soft bytes (0 .. 255, 255 a confident 1: Modem's soft bits) in
 *               transmit order; bytes from N on are never read.  payload[F][n] receives the first n decoded bytes and
 *               nothing beyond them; valid[F] (u8) is 1 where the CRC of the decoded payload equals the decoded CRC field,
 *               always 1 with YAGI_CRC_NONE; crc[F] (u32, may be NULL) is the CRC computed over the decoded payload, 0 for
 *               NONE; metric[F] (u32, may be NULL) is ConvCode's.
 *   create(n, crc, K, g, R, puncture, p, terminated, columns, scramble)   anything outside the limits is YAGI_ERR_CONFIG,
 *                             decided before any device is asked for
 *   destroy / clone / set_stream
 *   get_payload_len (n) / get_crc_len (w) / get_msg_bits (8 (n + w)) / get_enc_len (N) / get_nsym(bps, &count) / get_columns
 *   set_shape / get_shape(F) / yagi_hip_packetizer_plan   ConvCode's arrangement: the same admissible set, the same planner
 *                             (on the steps of the message) and the same yagi_hip_convcode_shape; lds_bytes is what the
 *                             Packetizer's decoder allocates (no staged raw words; a 2 KiB table where there is a CRC)
 *   encode_block / decode_block, encode_block_dev / decode_block_dev (device pointers, asynchronous on the object's stream)
 *   encode_host / decode_host   the definition's sequential loops on the host alone, around ConvCode's; no device needed
 *   yagi_hip_crc_host(scheme, data, n, &crc) / yagi_hip_packetizer_permutation(N, columns, pi)   pi[i] for i < N
 *   yagi_hip_scramble_data / yagi_hip_unscramble_data / yagi_hip_unscramble_data_soft   the reference's three functions
 *                             exactly, in place, the chunks_exact behaviour of the soft one included
 * The pitches are in bytes and at least the row length; F <= YAGI_CONVCODE_FRAMES_MAX; F = 0 touches nothing; the operands
 * of a _dev call must not overlap; device crc and metric pointers are 4-byte aligned.  The decoder loads soft bytes one by
 * one, so nothing outside a row's first N bytes is read.
 * Not built: custom CRC polynomials, block codes and a second (outer) code, convolutional or
 * per-symbol interleavers, [step][channel] soft input, a payload length per frame, a stand-alone device CRC or
 * interleaver object, Modem fused into either side.
 * Device form: packetizer_kernels.hip, convcode_body.hpp. */
#define YAGI_CRC_NONE 0
#define YAGI_CRC_8 1
#define YAGI_CRC_16 2
#define YAGI_CRC_24 3
#define YAGI_CRC_32 4
#define YAGI_PACKETIZER_COLUMNS_MAX 1048576
typedef struct yagi_hip_packetizer_s *yagi_hip_packetizer;
int yagi_hip_packetizer_plan(int K, int terminated, size_t n, int crc, size_t F, yagi_hip_convcode_shape *plan);
int yagi_hip_packetizer_create(size_t n, int crc, int K, const unsigned *g, int R, const uint8_t *puncture, int p, int terminated,
                               size_t columns, int scramble, yagi_hip_packetizer *q);
int yagi_hip_packetizer_destroy(yagi_hip_packetizer q);
int yagi_hip_packetizer_clone(yagi_hip_packetizer q, yagi_hip_packetizer *out);
int yagi_hip_packetizer_set_stream(yagi_hip_packetizer q, yagi_stream_t s);
int yagi_hip_packetizer_get_payload_len(yagi_hip_packetizer q, size_t *n);
int yagi_hip_packetizer_get_crc_len(yagi_hip_packetizer q, size_t *w);
int yagi_hip_packetizer_get_msg_bits(yagi_hip_packetizer q, size_t *bits);
int yagi_hip_packetizer_get_enc_len(yagi_hip_packetizer q, size_t *N);
int yagi_hip_packetizer_get_nsym(yagi_hip_packetizer q, unsigned bps, size_t *nsym);
int yagi_hip_packetizer_get_columns(yagi_hip_packetizer q, size_t *columns);
int yagi_hip_packetizer_set_shape(yagi_hip_packetizer q, unsigned frames_per_wave, unsigned waves);
int yagi_hip_packetizer_get_shape(yagi_hip_packetizer q, size_t F, yagi_hip_convcode_shape *shape);
int yagi_hip_packetizer_encode_block(yagi_hip_packetizer q, const uint8_t *payload, size_t payload_pitch, size_t F, unsigned bps,
                                     uint8_t *tx, size_t tx_pitch);
int yagi_hip_packetizer_encode_block_dev(yagi_hip_packetizer q, const uint8_t *payload_dev, size_t payload_pitch, size_t F,
                                         unsigned bps, uint8_t *tx_dev, size_t tx_pitch);
int yagi_hip_packetizer_decode_block(yagi_hip_packetizer q, const uint8_t *soft, size_t soft_pitch, size_t F, uint8_t *payload,
                                     size_t payload_pitch, uint8_t *valid, uint32_t *crc, uint32_t *metric);
int yagi_hip_packetizer_decode_block_dev(yagi_hip_packetizer q, const uint8_t *soft_dev, size_t soft_pitch, size_t F,
                                         uint8_t *payload_dev, size_t payload_pitch, uint8_t *valid_dev, uint32_t *crc_dev,
                                         uint32_t *metric_dev);
int yagi_hip_packetizer_encode_host(size_t n, int crc, int K, const unsigned *g, int R, const uint8_t *puncture, int p,
                                    int terminated, size_t columns, int scramble, const uint8_t *payload, size_t payload_pitch,
                                    size_t F, unsigned bps, uint8_t *tx, size_t tx_pitch);
int yagi_hip_packetizer_decode_host(size_t n, int crc, int K, const unsigned *g, int R, const uint8_t *puncture, int p,
                                    int terminated, size_t columns, int scramble, const uint8_t *soft, size_t soft_pitch, size_t F,
                                    uint8_t *payload, size_t payload_pitch, uint8_t *valid, uint32_t *crc_out, uint32_t *metric);
int yagi_hip_crc_host(int scheme, const uint8_t *data, size_t n, uint32_t *crc);
int yagi_hip_packetizer_permutation(size_t N, size_t columns, uint32_t *pi);
int yagi_hip_scramble_data(uint8_t *x, size_t n);
int yagi_hip_unscramble_data(uint8_t *x, size_t n);
int yagi_hip_unscramble_data_soft(uint8_t *x, size_t n);

/* ---- design helpers exposed for hosts that want the taps; no device needed ---------------- */
int yagi_hip_fir_design_kaiser(size_t n, float fc, float as_, float mu, float *h);      /* kaiser.rs:16-51 */

/* (Root-)Nyquist prototypes: src/filter/fir/design/mod.rs:392-451, single precision like the reference.
 *   estimate_req_filter_stopband_attenuation(df, n, &as_)   design/mod.rs:161-184: twenty bisections of [0.01, 200] dB on
 *                             the Kaiser length estimate (as_ - 7.95) / (14.26 df) (:228-238); df outside (0, 0.5] is
 *                             YAGI_ERR_CONFIG
 *   fir_design_prototype(ftype, k, m, beta, dt, h)   h receives 2km+1 taps.  ftype is numbered as FirFilterShape
 *                             (design/mod.rs:41-77).  Built here:
 *                               KAISER    fir_design_kaiser(2km+1, 0.5/k, as_, dt), as_ from the estimate at df = beta/k
 *                               RCOS      rcos.rs:17-51     k, m >= 1, beta in [0, 1]
 *                               RRCOS     rrcos.rs:15-63    the same ranges; both special branches (z = 0, 16 beta^2 z^2 = 1)
 *                               ARKAISER  rkaiser.rs:49-93  k >= 2, m >= 1, beta in (0, 1), dt in [-1, 1]; sum h^2 = k
 *                             The estimate runs first for every shape, as in the reference, so beta = 0 (df = 0) is
 *                             YAGI_ERR_CONFIG for all of them, and KAISER takes dt in (-0.5, 0.5] (kaiser.rs:18).  k = 0
 *                             and m = 0 are YAGI_ERR_CONFIG for every shape (the reference would divide by zero).
 *                             Every other shape (PM, FEXP, FSECH, FARCSECH, RKAISER, HM3, GMSKTX, GMSKRX, RFEXP, RFSECH,
 *                             RFARCSECH) is YAGI_ERR_CONFIG ("not built").  ARKAISER: where the closed-form bandwidth
 *                             correction rho_hat (rkaiser.rs:65-69) leaves (0, 1) the reference falls back on a table of
 *                             fitted constants (:105-144) that is not part of this library; that is YAGI_ERR_CONFIG here
 *                             (for example m = 1, beta = 0.05).  k 2..12, m 4..31, beta 0.2..0.35 stay inside. */
enum yagi_fir_shape {
    YAGI_FIR_SHAPE_KAISER = 0, YAGI_FIR_SHAPE_PM, YAGI_FIR_SHAPE_RCOS, YAGI_FIR_SHAPE_FEXP, YAGI_FIR_SHAPE_FSECH,
    YAGI_FIR_SHAPE_FARCSECH, YAGI_FIR_SHAPE_ARKAISER, YAGI_FIR_SHAPE_RKAISER, YAGI_FIR_SHAPE_RRCOS, YAGI_FIR_SHAPE_HM3,
    YAGI_FIR_SHAPE_GMSKTX, YAGI_FIR_SHAPE_GMSKRX, YAGI_FIR_SHAPE_RFEXP, YAGI_FIR_SHAPE_RFSECH, YAGI_FIR_SHAPE_RFARCSECH,
    YAGI_FIR_SHAPE_UNKNOWN = -1   /* no reference counterpart: what a SymStream made from external taps reports */
};
int yagi_hip_estimate_req_filter_stopband_attenuation(float df, size_t n, float *as_);
int yagi_hip_fir_design_prototype(int ftype, size_t k, size_t m, float beta, float dt, float *h /* 2km+1 */);

/* ---- SymStream (symstreamcf): src/framing/symstream.rs:6-122 (symbol source -> modulator -> pulse shaper) -----------------
 * The reference draws its symbols from Modem::random_symbol, a generator nobody can reproduce (its own clone test is
 * disabled for that reason, :330-333).  Here the symbol source is an LFSR: a private copy of an MSequence taken at
 * creation.  Everything else is the reference's object: ftype, k, m, beta, a Modem, a gain, a FirInterpolationFilter
 * <Complex<f32>, f32> of k branches with Ls = 2m+1 taps each and scale 1, and buf_index in [0, k).
 *
 * Definition.  Sample t of the stream since creation or reset() is branch t mod k of the interpolator after symbol
 * floor(t / k) was pushed (write_samples :111-121).  The pushed value is v = modulate(s) * gain, two f32 products
 * (re gain, im gain) (:104-109); s = source.generate_symbol(bps) is drawn when the symbol's first sample is written;
 * gain, scheme and bps are read at that moment and the interpolator's window keeps VALUES, so set_gain / set_scheme
 * between calls affect later symbols only.  Every output word equals MSequence.generate_symbols_block ->
 * Modem.modulate_block -> x gain per component -> FirInterpolationFilter(crcf).execute_block run one after the other,
 * at any n, any cut of the stream into calls and any mix of the entry points.
 *   create_linear(ftype, k, m, beta, scheme, src)   new_linear() :24-59 plus the source.  k < 2, m == 0 and beta outside
 *                             [0, 1] are YAGI_ERR_CONFIG; scheme errors are Modem's, design errors those of
 *                             yagi_hip_fir_design_prototype (dt = 0).  src is copied at its current state (its state
 *                             word, m, g and jump tables) and not touched afterwards.
 *   create_taps(k, h, h_len, scheme, src)   extension: externally designed taps, as yagi_hip_firinterp_crcf_create(k, h,
 *                             h_len) takes them (Ls = ceil(h_len / k)).  get_ftype reports YAGI_FIR_SHAPE_UNKNOWN, get_beta
 *                             0, and get_m floor((Ls - 1) / 2): the m of a 2km+1-tap prototype, so get_delay stays k m.
 *   destroy / clone / set_stream      clone copies everything: source state, window, buf_index, the modem with its DPSK
 *                             index, gain.  A clone and its original then write equal streams.
 *   reset()                   :61-65  the modem, the interpolator's window and buf_index.  The source stays where it
 *                             stands, as the reference leaves its generator.
 *   source_set_state(a) / source_get_state(&a)   extension: rewind or read the source's state word (not masked, as
 *                             MSequence::set_state).  After any calls the state equals (symbols drawn) x bps advance()s.
 *   get_ftype / get_k / get_m / get_beta / get_scheme / get_gain / get_delay (= k m)      :67-102
 *   set_scheme(scheme)        :83-86  builds a new modem: DPSK index 0, new bps
 *   set_modem(mod)            extension: a copy of the caller's Modem at its current state (the way to an arbitrary
 *                             constellation, yagi_hip_modem_create_from_table); get_scheme then reports its scheme
 *   set_gain(gain)            :92-94  any float
 *   write_samples(y, n)       :111-121  any n; a call may start and end inside a symbol, buf_index carries over.  Host
 *                             pointer, staged through the device.  n = 0 is a no-op.
 *   write_samples_dev(y_dev, n)   the same on a device buffer, asynchronous on the object's stream
 *   modulate_symbols(sym, nsym, y) / _dev   extension: the caller's symbol bytes instead of the source, nsym symbols ->
 *                             nsym k samples; the source does not advance.  A symbol >= M anywhere is YAGI_ERR_RANGE: y is
 *                             not written and no state moves (as yagi_hip_modem_modulate_block).  Allowed only on a symbol
 *                             boundary (buf_index == 0), else YAGI_ERR_MODE.  The _dev form reads the range flag back, so it
 *                             returns after the check has run; sym_dev and y_dev must not overlap (YAGI_ERR_CONFIG).
 *   is_fused(&fused)          read-only: 1 where a block call of the object as it stands runs the fused kernel, 0 where it
 *                             runs the three launches of the parts (DPSK schemes; shapes whose bank plan is
 *                             YAGI_PLAN_PFB_NONE or whose span + tables exceed 64 KiB of LDS).  The words are the same.
 * Device pointers: y_dev 8-byte aligned.
 * Device form: symstream_kernels.hip: one launch per call; a workgroup jumps the LFSR to its tile,
 * stages gain x constellation points in LDS and runs the bank kernels' sums. */
typedef struct yagi_hip_symstreamcf_s *yagi_hip_symstreamcf;
int yagi_hip_symstreamcf_create_linear(int ftype, size_t k, size_t m, float beta, int scheme, yagi_hip_msequence src,
                                       yagi_hip_symstreamcf *q);
int yagi_hip_symstreamcf_create_taps(size_t k, const float *h, size_t h_len, int scheme, yagi_hip_msequence src,
                                     yagi_hip_symstreamcf *q);
int yagi_hip_symstreamcf_destroy(yagi_hip_symstreamcf q);
int yagi_hip_symstreamcf_clone(yagi_hip_symstreamcf q, yagi_hip_symstreamcf *out);
int yagi_hip_symstreamcf_set_stream(yagi_hip_symstreamcf q, yagi_stream_t s);
int yagi_hip_symstreamcf_reset(yagi_hip_symstreamcf q);
int yagi_hip_symstreamcf_source_set_state(yagi_hip_symstreamcf q, unsigned a);
int yagi_hip_symstreamcf_source_get_state(yagi_hip_symstreamcf q, unsigned *a);
int yagi_hip_symstreamcf_get_ftype(yagi_hip_symstreamcf q, int *ftype);
int yagi_hip_symstreamcf_get_k(yagi_hip_symstreamcf q, size_t *k);
int yagi_hip_symstreamcf_get_m(yagi_hip_symstreamcf q, size_t *m);
int yagi_hip_symstreamcf_get_beta(yagi_hip_symstreamcf q, float *beta);
int yagi_hip_symstreamcf_get_scheme(yagi_hip_symstreamcf q, int *scheme);
int yagi_hip_symstreamcf_get_gain(yagi_hip_symstreamcf q, float *gain);
int yagi_hip_symstreamcf_get_delay(yagi_hip_symstreamcf q, size_t *delay);
int yagi_hip_symstreamcf_get_buf_index(yagi_hip_symstreamcf q, size_t *buf_index);
int yagi_hip_symstreamcf_set_scheme(yagi_hip_symstreamcf q, int scheme);
int yagi_hip_symstreamcf_set_modem(yagi_hip_symstreamcf q, yagi_hip_modem mod);
int yagi_hip_symstreamcf_set_gain(yagi_hip_symstreamcf q, float gain);
int yagi_hip_symstreamcf_is_fused(yagi_hip_symstreamcf q, int *fused);
int yagi_hip_symstreamcf_write_samples(yagi_hip_symstreamcf q, yagi_cf32 *y, size_t n);
int yagi_hip_symstreamcf_write_samples_dev(yagi_hip_symstreamcf q, yagi_cf32 *y_dev, size_t n);
int yagi_hip_symstreamcf_modulate_symbols(yagi_hip_symstreamcf q, const uint8_t *sym, size_t nsym, yagi_cf32 *y);
int yagi_hip_symstreamcf_modulate_symbols_dev(yagi_hip_symstreamcf q, const uint8_t *sym_dev, size_t nsym,
                                              yagi_cf32 *y_dev);

/* ---- SymStreamR (symstreamrcf): src/framing/symstreamr.rs:9-129 (SymStream at any bandwidth) ---------------------------
 * Definition: S = symstreamcf_create_linear(ftype, k = 2, m, beta, scheme, src) pushed one sample at a time through
 * R = msresamp_crcf_create(rate = 0.5f / bw, as = 60): the arbitrary Resamp(rate_arb, 7, min(0.515 rate_arb, 0.49), 60,
 * 256) first, then S half-band interpolator stages (0 .. 8; bw >= 0.25 has none, and the decimator chain never occurs).
 * With s[] the samples of S since reset() and y[] the concatenation of what R.execute returns for them, write_samples(n)
 * returns y[P .. P + n) and advances P.  A sample is pushed only when every output so far has been taken (fill_buffer
 * :101-116), so after any call the number pushed is the smallest N with outputs(N) >= P; the outputs of the last pushed
 * sample beyond P (at most 2 * 2^S) stay on the device and are served first by the next call.  The schedule is a closed
 * form on the Resamp's integer phase p0: q = ceil(missing / 2^S) arbitrary-stage outputs need
 * ((p0 + (q - 1) step) >> 24) + 1 samples (0 for q = 0), so no call reads anything back.  Consequences, bit for bit: the
 * stream does not depend on how it is cut into calls; source_get_state stands where an MSequence stands after the bits
 * of ceil(N / 2) symbols; set_gain / set_scheme reach only symbols drawn later.
 *   create_linear(ftype, bw, m, beta, scheme, src)   :23-53 plus the source.  bw outside [0.001, 1] or not finite, a null
 *                             source and whatever symstreamcf_create_linear refuses are YAGI_ERR_CONFIG.
 *   destroy / clone / set_stream      clone copies everything, the outputs not yet taken included
 *   reset()                   :55-60  S, R, P and the outputs not yet taken; the source stays where it stands
 *   get_bw                    :66-68  1 / (rate k) in f32 -- not the argument echoed back
 *   get_delay                 :94-99  (k m + R.get_delay()) rate in f32
 *   get_ftype / get_m / get_beta / get_scheme / get_gain / set_scheme / set_gain      :62-92, S's
 *   set_modem / source_set_state / source_get_state      extensions, as symstreamcf's
 *   get_params(&interp, &stages, &rate_arbitrary)   R's; any pointer may be null
 *   get_pending(&n)           outputs pushed and not yet taken
 *   write_samples(y, n) / write_samples_dev(y_dev, n)    :118-128  any n.  The _dev form is asynchronous on the object's
 *                             stream; a call the pending outputs cover launches no kernel.
 *   is_fused(&fused)          1 where a call runs symstreamr_kernels.hip (S and the arbitrary Resamp in one launch that
 *                             reads no sample, then R's half-band chain), 0 where it runs S.write_samples_dev into
 *                             scratch and R's two parts (DPSK schemes, modems S does not run fused, shapes whose LDS
 *                             does not fit).  The words are the same.
 * Device pointers: y_dev 8-byte aligned.
 * plan_symstreamr(bw, m, n, p0): what a call that misses n outputs with the Resamp at phase p0 does, without a device:
 * the split of the rate, the Resamp's step, the fused kernel's tile (arbitrary-stage outputs per tile), the most tiles
 * a workgroup stages and the tiles per workgroup of this call (0: the shape is not served fused for any constellation),
 * its dynamic LDS with a 256-point constellation, q, need, the outputs of the arbitrary stage and of the chain, the
 * leftover and the phase after the call. */
typedef struct yagi_hip_symstreamrcf_s *yagi_hip_symstreamrcf;
int yagi_hip_symstreamrcf_create_linear(int ftype, float bw, size_t m, float beta, int scheme, yagi_hip_msequence src,
                                        yagi_hip_symstreamrcf *q);
int yagi_hip_symstreamrcf_destroy(yagi_hip_symstreamrcf q);
int yagi_hip_symstreamrcf_clone(yagi_hip_symstreamrcf q, yagi_hip_symstreamrcf *out);
int yagi_hip_symstreamrcf_set_stream(yagi_hip_symstreamrcf q, yagi_stream_t s);
int yagi_hip_symstreamrcf_reset(yagi_hip_symstreamrcf q);
int yagi_hip_symstreamrcf_source_set_state(yagi_hip_symstreamrcf q, unsigned a);
int yagi_hip_symstreamrcf_source_get_state(yagi_hip_symstreamrcf q, unsigned *a);
int yagi_hip_symstreamrcf_get_ftype(yagi_hip_symstreamrcf q, int *ftype);
int yagi_hip_symstreamrcf_get_bw(yagi_hip_symstreamrcf q, float *bw);
int yagi_hip_symstreamrcf_get_m(yagi_hip_symstreamrcf q, size_t *m);
int yagi_hip_symstreamrcf_get_beta(yagi_hip_symstreamrcf q, float *beta);
int yagi_hip_symstreamrcf_get_scheme(yagi_hip_symstreamrcf q, int *scheme);
int yagi_hip_symstreamrcf_get_gain(yagi_hip_symstreamrcf q, float *gain);
int yagi_hip_symstreamrcf_get_delay(yagi_hip_symstreamrcf q, float *delay);
int yagi_hip_symstreamrcf_get_pending(yagi_hip_symstreamrcf q, size_t *n);
int yagi_hip_symstreamrcf_get_params(yagi_hip_symstreamrcf q, int *interp, size_t *num_halfband_stages,
                                     float *rate_arbitrary);
int yagi_hip_symstreamrcf_set_scheme(yagi_hip_symstreamrcf q, int scheme);
int yagi_hip_symstreamrcf_set_modem(yagi_hip_symstreamrcf q, yagi_hip_modem mod);
int yagi_hip_symstreamrcf_set_gain(yagi_hip_symstreamrcf q, float gain);
int yagi_hip_symstreamrcf_is_fused(yagi_hip_symstreamrcf q, int *fused);
int yagi_hip_symstreamrcf_write_samples(yagi_hip_symstreamrcf q, yagi_cf32 *y, size_t n);
int yagi_hip_symstreamrcf_write_samples_dev(yagi_hip_symstreamrcf q, yagi_cf32 *y_dev, size_t n);

typedef struct {
    int interp;            /* R's type: 1 where rate > 1 */
    int tile;              /* arbitrary-stage outputs per tile (plan_resamp's) */
    int max_wg_tiles;      /* most tiles a workgroup stages; 0: not served fused */
    int wg_tiles;          /* tiles per workgroup of this call */
    uint32_t step;         /* round(2^24 / rate_arb) */
    uint32_t phase_next;   /* the Resamp's phase after the call */
    float rate, rate_arb;
    size_t stages;         /* half-band interpolator stages S */
    size_t lds;            /* dynamic LDS of the fused launch, M = 256 */
    size_t q;              /* ceil(n / 2^S) */
    size_t need;           /* samples of the SymStream the call pushes */
    size_t outputs_arb;    /* outputs of the arbitrary stage for them */
    size_t outputs;        /* outputs_arb * 2^S */
    size_t leftover;       /* outputs - n */
} yagi_hip_symstreamr_plan;
int yagi_hip_plan_symstreamr(float bw, size_t m, size_t n, uint32_t p0, yagi_hip_symstreamr_plan *out);

#ifdef __cplusplus
}
#endif
#endif /* YAGI_HIP_H */
