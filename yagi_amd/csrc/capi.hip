// capi.hip -- the extern "C" surface of libyagi_hip.so (include/yagi_hip.h): stateful objects that
// mirror yagi's FirFilter / FirDecimationFilter / FirPfbFilter / Fft (+ the channelizers and the
// fused FIR->FFT stream) with all arithmetic on the device.
//
// State model.  The reference keeps a Window<T>/VecDeque<T> of the last L samples inside each
// object (firfilt.rs:13, firdecim.rs:15, firpfb.rs:12).  Here that window lives in HBM as L
// samples, oldest first (a ring of three buffers so an update never races the kernel reading it),
// with a host mirror for the per-sample calls: push() / execute() / execute_one() run on the host
// mirror with the reference's own sequential sums (host.cpp: tens of nanoseconds per call, no
// launch), block calls run the FIR kernels on the device window; the two copies are synchronised
// lazily when the caller switches between the two kinds of call (DevWindow).  clone() copies the
// state; reset() zeroes it.
#include <cmath>
#include <cstdlib>
#include <complex>
#include <memory>

#include <algorithm>
#include <atomic>

#include "kernels.hpp"
#include "objstate.hpp"
#include "stream_tables.hpp"

namespace yagi {

int design_kaiser(size_t n, float fc, float as_, float mu, std::vector<float> &h);   // host.cpp
int window_value(int type, size_t i, size_t wlen, float arg, float *out);            // host.cpp
int design_notch(size_t m, float f0, float as_, std::vector<float> &h);                // host.cpp
int design_prototype(int ftype, size_t k, size_t m, float beta, float dt, std::vector<float> &h);   // host.cpp

static int require_device() {
    static int ok = -1;
    if (ok < 0) {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        ok = (e == hipSuccess && n > 0) ? 1 : 0;
    }
    if (!ok) return fail(YAGI_ERR_DEVICE, "no HIP device available: libyagi_hip has no CPU fallback");
    return YAGI_OK;
}

template <class V> static V one_of();
template <> float one_of<float>() { return 1.0f; }
template <> cf32 one_of<cf32>() { return cf32{1.0f, 0.0f}; }
static cf32 to_c(float v, cf32 *) { return cf32{v, 0.0f}; }
static float to_c(float v, float *) { return v; }

// Pipelined block calls (yagi_hip_firfft_crcf_set_pipeline, yagi_hip_firfilt_*_set_pipeline).  Consecutive blocks of the stream depend on each other
// only through the L-sample filter window, and that window is INPUT data (the previous block's last L samples), which
// the pipelined contract keeps intact until the join: block b + 1 reads it straight from the previous call's x, so it
// needs nothing block b computes.  The block kernels alternate between two streams (lanes); call b does
//     caller's stream: record `in`           lane b % 2: wait(in), block kernel b, record done[b % 2]
// so block b + 1 ramps up while block b drains (on one stream every kernel waits for the complete drain of the one
// before it: ~4 us of a 61 us block).  The caller's stream is NOT made to wait per call (its next `in` would inherit
// that wait and serialise the blocks); it joins the lanes in *_join (DevWindow::join), which every other use of the
// object's window goes through first and which also copies the last block's tail into the object's window.
struct StreamPipe {
    bool on = false;
    // two lanes (a device exposes four hardware queues, the caller's stream and the null stream take two): in the bench
    // three lanes read the same, four lose 8 %
    static constexpr int kLanes = 2;
    hipStream_t lane[kLanes] = {};
    hipEvent_t in = nullptr, done[kLanes] = {};
    bool busy[kLanes] = {};
    unsigned calls = 0;
    const void *prev_tail = nullptr;      // last L samples of the previous pipelined block (null: use the object's window)
    int init() {
        if (lane[0]) return YAGI_OK;
        for (auto &s : lane) YG_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        YG_HIP(hipEventCreateWithFlags(&in, hipEventDisableTiming));
        for (auto &e : done) YG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return YAGI_OK;
    }
    ~StreamPipe() {
        for (auto &s : lane)
            if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
        if (in) (void)hipEventDestroy(in);
        for (auto &e : done) if (e) (void)hipEventDestroy(e);
    }
};

// ---------------------------------------------------------------------------------------------
// Device window of the last `len` samples + host push queue
// ---------------------------------------------------------------------------------------------
template <class T>
struct DevWindow {
    int len = 0;
    static constexpr int kBufs = 3;   // a ring of three: kernels write window b+1 into next() while block b reads dev()
    PingPong<kBufs> ring;
    // Host mirror for the per-sample calls (push / execute / execute_one: firfilt.rs:220-261, firpfb.rs:255-286,
    // firdecim.rs:179-191).  hbuf[hend - len, hend) = the last len samples, oldest first -- Window<T>::read()'s layout
    // (window.rs:77-85): a push appends, and when the slack behind the window is used up the window moves back to the
    // front.  The two copies are synchronised lazily: a per-sample call after a block call downloads the device window
    // once (ensure_host), a block call after per-sample calls uploads the host window once (ensure_dev); in between,
    // per-sample calls cost a sequential dot product on the host and no launch.
    static constexpr size_t kSlack = 4096;
    std::vector<T> hbuf;
    size_t hend = 0;
    Mirror mirror;
    uint64_t npush = 0;               // samples pushed since the window was made: the ring position of FirFilter's VecDeque
    StreamPipe pipe;                  // pipelined block calls (objects that offer set_pipeline)

    // the caller's stream waits for every block handed to the lanes, then takes over the filter window (the last block's
    // tail); every other access to the window comes through here first
    int join(hipStream_t st) {
        for (int i = 0; i < StreamPipe::kLanes; ++i) {
            if (pipe.busy[i]) YG_HIP(hipStreamWaitEvent(st, pipe.done[i], 0));
            pipe.busy[i] = false;
        }
        if (pipe.prev_tail) {
            YG_TRY(launch_update_window<T>(dev(), static_cast<const T *>(pipe.prev_tail), (size_t)len, len, next(), st));
            flip();
            pipe.prev_tail = nullptr;
        }
        return YAGI_OK;
    }
    // one pipelined block: the caller's stream records `in`, lane (calls & 1) waits for it; returns the lane and the
    // window the block kernel reads.  finish_piped() after the launch.
    int begin_piped(hipStream_t st, hipStream_t *lane, const T **win) {
        const int i = (int)(pipe.calls % (unsigned)StreamPipe::kLanes);
        YG_HIP(hipEventRecord(pipe.in, st));
        YG_HIP(hipStreamWaitEvent(pipe.lane[i], pipe.in, 0));
        *lane = pipe.lane[i];
        *win = pipe.prev_tail ? static_cast<const T *>(pipe.prev_tail) : dev();
        return YAGI_OK;
    }
    int finish_piped(const T *x, size_t n) {          // n >= len
        const int i = (int)(pipe.calls % (unsigned)StreamPipe::kLanes);
        YG_HIP(hipEventRecord(pipe.done[i], pipe.lane[i]));
        pipe.busy[i] = true;
        ++pipe.calls;
        pipe.prev_tail = x + (n - (size_t)len);
        mirror.dev_written();
        return YAGI_OK;
    }
    bool can_pipe(size_t n) const { return pipe.on && mirror.dev_current() && n >= (size_t)len; }

    int init(int n, hipStream_t st) {
        len = n;
        YG_TRY(ring.alloc((size_t)n * sizeof(T)));
        hbuf.assign((size_t)n + kSlack, T{});
        npush = 0;
        return reset(st);
    }
    int reset(hipStream_t st) {       // zeroes the samples in place; the ring position is kept (firfilt.rs:209-213)
        YG_TRY(join(st));
        YG_HIP(hipMemsetAsync(ring.cur(), 0, (size_t)len * sizeof(T), st));
        std::fill(hbuf.begin(), hbuf.begin() + len, T{});
        hend = (size_t)len;
        mirror.in_sync();
        return YAGI_OK;
    }
    const T *dev() const { return ring.template cur<T>(); }
    // for kernels that write the next window themselves: the other buffer, then flip()
    T *next() { return ring.template next<T>(); }
    void flip() { ring.flip(); mirror.dev_written(); }
    // window <- last len of (window ++ x_dev[0..n))
    int advance(const T *x_dev, size_t n, hipStream_t st) {
        if (n == 0) return YAGI_OK;
        YG_TRY(launch_update_window<T>(dev(), x_dev, n, len, next(), st));
        flip();
        return YAGI_OK;
    }
    const T *host() const { return hbuf.data() + (hend - (size_t)len); }        // oldest first; valid after ensure_host
    void push(T v) {                                                              // after ensure_host
        if (hend == hbuf.size()) {
            std::memmove(hbuf.data(), hbuf.data() + (hend - (size_t)len + 1), ((size_t)len - 1) * sizeof(T));
            hend = (size_t)len - 1;
        }
        hbuf[hend++] = v;
        ++npush;
        mirror.host_written();
    }
    // the device window is what the block kernels read: bring it up to date with the host mirror
    int ensure_dev(hipStream_t st) {
        YG_TRY(join(st));
        return mirror.need_dev([&] { return upload(ring.cur(), host(), (size_t)len * sizeof(T), st); });
    }
    // the host mirror is what the per-sample calls read: fetch the window a block kernel left on the device
    int ensure_host(hipStream_t st) {
        YG_TRY(join(st));
        return mirror.need_host([&] {
            hend = (size_t)len;                       // read only once the copy has arrived
            return download(hbuf.data(), ring.cur(), (size_t)len * sizeof(T), st);
        });
    }
    int clone_from(const DevWindow &o, hipStream_t st) {       // o.ensure_dev() has run
        YG_TRY(init(o.len, st));
        YG_HIP(hipMemcpyAsync(ring.cur(), o.ring.cur(), (size_t)len * sizeof(T), hipMemcpyDeviceToDevice, st));
        YG_HIP(hipStreamSynchronize(st));
        npush = o.npush;
        mirror.dev_written();
        return YAGI_OK;
    }
};

// the per-sample arithmetic (host.cpp): the reference's own sequential sums, products unfused
template <class T, class C> T host_fir_ring_dot(const T *w, size_t L, size_t head, const C *h, C scale);
template <class T, class C> T host_fir_window_dot(const T *w, size_t L, const C *h, C scale);

// ---------------------------------------------------------------------------------------------
// FirFilter<T,C>
// ---------------------------------------------------------------------------------------------
template <class K>
struct FirFilt {
    using T = typename K::T;
    using C = typename K::C;
    hipStream_t st = nullptr;
    int L = 0, Lp = 0;
    std::vector<C> h;          // host copy (get_coefficients)
    C scale = one_of<C>();
    DevBuf taps;               // h[0..L) on device
    DevBuf taps_pad;           // crcf only: zero-padded to Lp floats for the sliding kernel
    DevBuf apack;              // crcf only, L <= 256: Toeplitz A-operand table of the MFMA kernel
    int Lm = 0;                // padded length of the MFMA form (0 = not available)
    DevBuf hfreq, twf, twb;    // crcf only, L <= 2049: FFT_4096{[h;0]} and both twiddle tables (fast convolution)
    DevBuf gfft, gfft_s;       // crcf only, L <= 257: conj(DFT_512{reversed taps}) / 512 and its scaled copy in the pair layout (fast correction sum)
    DevBuf hfreq_s;            // scale * hfreq in the pair layout (stream_tables.hpp) for the frequency-domain stream kernel, rebuilt when the scale changes
    bool hfreq_s_valid = false;
    float hfreq_s_scale = 0.f;
    bool conv_ready = false;
    DevWindow<T> w;
    Staging ws;
    int kernel_choice = 0;     // 0 auto, 1 general, 2 sliding (crcf), 3 MFMA Toeplitz (crcf, L <= 256), 4 fast convolution
    int prepare_conv();

    int load_taps(const C *hh, size_t n) {
        if (n == 0) return fail(YAGI_ERR_CONFIG, "filter length must be greater than zero");
        if (n > (size_t)1 << 24) return fail(YAGI_ERR_CONFIG, "filter too long");
        h.assign(hh, hh + n);
        L = (int)n;
        YG_TRY(fill(taps, h.data(), n * sizeof(C), st));
        conv_ready = false;
        hfreq_s_valid = false;
        if (K::id == 1) {
            Lp = (L + 31) / 32 * 32;
            std::vector<float> hp((size_t)Lp, 0.0f);
            std::memcpy(hp.data(), h.data(), n * sizeof(float));
            YG_TRY(fill(taps_pad, hp.data(), (size_t)Lp * sizeof(float), st));
            Lm = mfma_lp_for(L);
            if (Lm) {
                std::vector<float> ap(toeplitz_pack_floats(Lm));
                pack_toeplitz_taps(reinterpret_cast<const float *>(h.data()), L, Lm, ap.data());
                YG_TRY(fill(apack, ap.data(), ap.size() * sizeof(float), st));
            }
        }
        return YAGI_OK;
    }
    int init(const C *hh, size_t n) {
        YG_TRY(require_device());
        YG_TRY(load_taps(hh, n));
        return w.init(L, st);
    }
    int block_dev(const T *x, size_t n, T *y);
    // execute() on the host mirror (firfilt.rs:241-246): the VecDeque's head moves back one slot per push, so after
    // npush pushes it sits at (-npush) mod L and as_slices() splits the newest-first sequence L - head from its start
    T host_execute() const {
        const size_t Ls = (size_t)L, head = (Ls - (size_t)(w.npush % Ls)) % Ls;
        return host_fir_ring_dot<T, C>(w.host(), Ls, head, h.data(), scale);
    }
};

// execute_block on device data.  The auto choice is always a direct form (the dotprod sums of the reference,
// exact on integer-valued data); the overlap-save kernel (kernel_choice 4) is opt-in for every type
// combination: 2.5x (crcf 256 taps) to 10x (rrrf / cccf) faster on long blocks, equal to f32 rounding.
// With the pipeline on (set_pipeline; StreamPipe) a block call of at least L samples runs on one of the object's two
// lanes and reads its window from the tail of the previous call's input.
template <class K>
int FirFilt<K>::block_dev(const T *x, size_t n, T *y) {
    if (n == 0) return w.ensure_dev(st);
    const bool piped = w.can_pipe(n) && (kernel_choice != 4 || conv_ready);
    hipStream_t s = st;
    const T *win = nullptr;
    if (piped) YG_TRY(w.begin_piped(st, &s, &win));
    else { YG_TRY(w.ensure_dev(st)); win = w.dev(); }
    T *wnext = piped ? nullptr : w.next();
    w.npush += n;
    const bool conv = kernel_choice == 4 && L <= 2049;
    if (conv) {
        YG_TRY(prepare_conv());
        if constexpr (K::id == 0)
            YG_TRY(launch_fir_rrrf_fftconv(win, x, 0, n, hfreq.as<cf32>(), scale, L, twf.as<cf32>(), twb.as<cf32>(), y, n, s, wnext));
        else
            YG_TRY(launch_fir_cccf_fftconv(win, x, 0, n, hfreq.as<cf32>(), scale, L, twf.as<cf32>(), twb.as<cf32>(), y, n, s, wnext));
    } else {
        YG_TRY((launch_fir_block<K>(win, x, taps.template as<C>(), L, 1, scale, y, n, s, 0, wnext)));
    }
    if (piped) return w.finish_piped(x, n);
    w.flip();                                       // the kernel's last workgroup wrote the next window
    return YAGI_OK;
}
template <>
int FirFilt<CRCF>::block_dev(const cf32 *x, size_t n, cf32 *y) {
    if (n == 0) return w.ensure_dev(st);
    const bool conv = kernel_choice == 4 && L <= 2049;
    // auto: the matrix-pipe Toeplitz form where it exists (<= 256 taps) and the block fills the chip -- the same sums as
    // the sliding vector form (both exact on integer data), but the vector form runs into the chip's power cap on
    // random data (0.63 of the FP32 peak, 0.80 on all-zero input) and the matrix form does not (0.79 either way:
    // profiles/r03_notes.md); else the register-sliding vector form
    const bool mfma = Lm && (kernel_choice == 3 || (kernel_choice == 0 && n >= ((size_t)1 << 16)));
    const bool slide = (kernel_choice == 2) || (kernel_choice == 0 && Lp <= kSlideMaxTaps && n >= 1024);
    const bool piped = w.can_pipe(n) && (!conv || conv_ready);
    hipStream_t s = st;
    const cf32 *win = nullptr;
    if (piped) YG_TRY(w.begin_piped(st, &s, &win));
    else { YG_TRY(w.ensure_dev(st)); win = w.dev(); }
    cf32 *wnext = piped ? nullptr : w.next();
    w.npush += n;
    if (conv) {
        YG_TRY(prepare_conv());
        YG_TRY(launch_fir_crcf_fftconv(win, x, 0, n, hfreq.as<cf32>(), scale, L, twf.as<cf32>(), twb.as<cf32>(), y, n, s, wnext));
    } else if (mfma) {
        YG_TRY(launch_fir_crcf_mfma(win, x, apack.as<float>(), L, Lm, scale, y, n, s, wnext));
    } else if (slide && Lp <= kSlideMaxTaps) {
        YG_TRY(launch_fir_crcf_slide(win, x, taps_pad.as<float>(), L, Lp, scale, y, n, s, wnext));
    } else {
        YG_TRY((launch_fir_block<CRCF>(win, x, taps.as<float>(), L, 1, scale, y, n, s, 0, wnext)));
    }
    if (piped) return w.finish_piped(x, n);
    w.flip();                                       // the kernel's last workgroup wrote the next window
    return YAGI_OK;
}

// ---------------------------------------------------------------------------------------------
// FirDecimationFilter<T,C>
// ---------------------------------------------------------------------------------------------
template <class K>
struct FirDecim {
    using T = typename K::T;
    using C = typename K::C;
    hipStream_t st = nullptr;
    int L = 0, M = 1;
    std::vector<C> h;
    C scale = one_of<C>();
    DevBuf taps;
    DevWindow<T> w;
    Staging ws;

    int init(size_t m, const C *hh, size_t n) {
        if (n == 0) return fail(YAGI_ERR_CONFIG, "filter length must be greater than zero");
        if (m == 0) return fail(YAGI_ERR_CONFIG, "decimation factor must be greater than zero");
        if (n > (size_t)1 << 24 || m > (size_t)1 << 20) return fail(YAGI_ERR_CONFIG, "filter too large");
        YG_TRY(require_device());
        h.assign(hh, hh + n);
        L = (int)n;
        M = (int)m;
        YG_TRY(fill(taps, h.data(), n * sizeof(C), st));
        return w.init(L, st);
    }
    // n outputs from n*M device samples
    int block_dev(const T *x, size_t n, T *y) {
        YG_TRY(w.ensure_dev(st));
        if (n == 0) return YAGI_OK;
        YG_TRY((launch_fir_block<K>(w.dev(), x, taps.template as<C>(), L, M, scale, y, n, st, 0, w.next())));
        w.flip();                                   // the kernel's last workgroup wrote the next window
        return YAGI_OK;
    }
};

// ---------------------------------------------------------------------------------------------
// FirPfbFilter<T,C>
// ---------------------------------------------------------------------------------------------
template <class K>
struct FirPfb {
    using T = typename K::T;
    using C = typename K::C;
    hipStream_t st = nullptr;
    int nf = 0, Ls = 0;
    std::vector<C> hb;         // [nf][Ls], natural order: hb[i][k] = h[i + k*nf]
    C scale = one_of<C>();
    DevBuf taps;
    DevWindow<T> w;
    Staging ws;

    int init(size_t num_filters, const C *hh, size_t h_len) {
        if (num_filters == 0) return fail(YAGI_ERR_CONFIG, "number of filters must be greater than zero");
        if (h_len == 0) return fail(YAGI_ERR_CONFIG, "filter length must be greater than zero");
        const size_t hs = h_len / num_filters;            // firpfb.rs:42 (floor)
        if (hs == 0) return fail(YAGI_ERR_CONFIG, "window size must be greater than zero");  // window.rs:14
        if (num_filters > (size_t)1 << 20 || hs > (size_t)1 << 20) return fail(YAGI_ERR_CONFIG, "filter bank too large");
        YG_TRY(require_device());
        nf = (int)num_filters;
        Ls = (int)hs;
        hb.resize((size_t)nf * Ls);
        for (int i = 0; i < nf; ++i)
            for (int k = 0; k < Ls; ++k) hb[(size_t)i * Ls + k] = hh[i + (size_t)k * nf];
        YG_TRY(fill(taps, hb.data(), hb.size() * sizeof(C), st));
        return w.init(Ls, st);
    }
    int check_branch(size_t i) const {
        if (i >= (size_t)nf) return fail(YAGI_ERR_CONFIG, "filterbank index (%zu) exceeds maximum (%d)", i, nf);
        return YAGI_OK;
    }
    int block_dev(size_t i, const T *x, size_t n, T *y) {
        YG_TRY(check_branch(i));
        YG_TRY(w.ensure_dev(st));
        YG_TRY((launch_fir_block<K>(w.dev(), x, taps.template as<C>() + i * (size_t)Ls, Ls, 1, scale, y, n, st)));
        return w.advance(x, n, st);
    }
};

// ---------------------------------------------------------------------------------------------
// Fft
// ---------------------------------------------------------------------------------------------
struct FftPlan {
    FftPlanDev d;
    DevBuf tw;
    Staging ws;
    DevBuf bs_w, bs_bf, bs_twf, bs_twb, bs_scratch;      // Bluestein resources (sizes with a large prime factor)
    std::unique_ptr<FftPlan> bs_fwd, bs_bwd;             // Bluestein over m > 8192: the m-point plans
    std::unique_ptr<FftPlan> fs_p1, fs_p2;               // four-step: the n1- and n2-point plans
    DevBuf fs_scratch, fs_wn, fs_wsplit;
};

// radix list of the mixed-radix kernel: the power of two in as few passes as radix <= 16 allows (bits spread
// evenly), then the odd primes in ascending order (3, 5, 7 have register butterflies, larger ones direct sums)
static void factorize(int n, int *fac, int &nfac) {
    nfac = 0;
    int lg = 0;
    while (n % 2 == 0) { ++lg; n /= 2; }
    if (lg) {
        const int np = (lg + 3) / 4;
        for (int i = 0; i < np; ++i) fac[nfac++] = 1 << (lg / np + (i < lg % np ? 1 : 0));
    }
    for (int p = 3; (long long)p * p <= n; p += 2)
        while (n % p == 0) { fac[nfac++] = p; n /= p; }
    if (n > 1) fac[nfac++] = n;
}

// W_n^m, m in [0,n); with half_too the W_{n/2} table follows at offset n (the 8192-point kernel runs two
// 4096-point transforms and needs both)
static int make_twiddles(int n, int dir, DevBuf &buf, bool half_too = false) {
    std::vector<cf32> t((size_t)n + (half_too ? (size_t)n / 2 : 0));
    const double s = (dir == YAGI_FFT_FORWARD) ? -1.0 : 1.0;
    for (int m = 0; m < n; ++m) {
        const double a = s * 2.0 * M_PI * (double)m / (double)n;
        t[m] = cf32{(float)std::cos(a), (float)std::sin(a)};
    }
    if (half_too)
        for (int m = 0; m < n / 2; ++m) {
            const double a = s * 2.0 * M_PI * (double)m / (double)(n / 2);
            t[(size_t)n + m] = cf32{(float)std::cos(a), (float)std::sin(a)};
        }
    return fill(buf, t.data(), t.size() * sizeof(cf32), nullptr);
}

// twiddle table of the 4096-point stream kernels: W_4096^m (m < 4096, forward) followed by six 256-entry rows the
// frequency-domain kernels read with the lane index (coalesced, no gathers): rows 0-3 W^{t 2^k}, row 4 W^{(t&15)(t>>4)},
// row 5 W_256^{(t&15)(t>>4)}.  Behind the rows the headline kernel's two paired tables (stream_tables.hpp): the six
// row entries of lane t and wave 0's six transform twiddles of lane l, two by two for 16-byte loads -- copies of
// entries above, so a kernel that reads them computes what it computed from the rows and the W_4096 gathers, bit for bit
static int make_stream_twiddles(DevBuf &buf) {
    std::vector<cf32> tab(kStreamTabFloat2);
    build_stream_twiddles(tab.data());      // stream_tables.hpp
    return fill(buf, tab.data(), tab.size() * sizeof(cf32), nullptr);
}

// W_n^m for any m < n as a product of two exact entries: tab[m & 4095] = W_n^{m & 4095}, tab[4096 + (m >> 12)] = W_n^{4096 (m >> 12)}
static int make_split_twiddles(size_t n, int dir, DevBuf &buf) {
    const size_t nhi = (n + 4095) / 4096;
    std::vector<cf32> tab(4096 + nhi);
    const double s = dir == YAGI_FFT_FORWARD ? -1.0 : 1.0;
    for (size_t j = 0; j < 4096; ++j) {
        const double a = s * 2.0 * M_PI * (double)j / (double)n;
        tab[j] = cf32{(float)std::cos(a), (float)std::sin(a)};
    }
    for (size_t j = 0; j < nhi; ++j) {
        const double a = s * 2.0 * M_PI * (double)(4096 * j) / (double)n;
        tab[4096 + j] = cf32{(float)std::cos(a), (float)std::sin(a)};
    }
    return fill(buf, tab.data(), tab.size() * sizeof(cf32), nullptr);
}

static int fft_plan_init(FftPlan &p, size_t n, int dir) {
    if (n == 0) return fail(YAGI_ERR_CONFIG, "fft length must be greater than zero");
    if (dir != YAGI_FFT_FORWARD && dir != YAGI_FFT_BACKWARD) return fail(YAGI_ERR_CONFIG, "bad fft direction");
    const bool pow2 = (n & (n - 1)) == 0;
    if (n > kFftMaxPow2 || (!pow2 && 2 * n - 1 > kFftMaxPow2))
        return fail(YAGI_ERR_CONFIG, "fft length %zu not supported (powers of two up to %zu, other sizes up to %zu)", n,
                    kFftMaxPow2, kFftMaxPow2 / 2);
    YG_TRY(require_device());
    p.d.n = (int)n;
    p.d.dir = dir;
    if (n > (size_t)kFftMaxLds) {
        // four-step: n = n1 n2, both <= 8192, as balanced as the divisors of n allow, and neither with a prime factor
        // that would send it to Bluestein (> 89); a size without such a split (a large prime factor) takes Bluestein
        size_t n2 = 0;
        if (pow2 && n >= 65536) {
            // n = 256 n2: 256-point columns in registers, then the n2-point rows (fft_kernels.hip: fft_tile256_kernel)
            n2 = n / 256;
            p.fs_p1 = std::make_unique<FftPlan>();
            p.fs_p2 = std::make_unique<FftPlan>();
            YG_TRY(fft_plan_init(*p.fs_p1, 256, dir));
            YG_TRY(fft_plan_init(*p.fs_p2, n2, dir));
            size_t chunk = ((size_t)1 << 23) / n;              // 64 MiB per scratch buffer (smaller chunks measured slower)
            if (chunk < 1) chunk = 1;
            YG_TRY(p.fs_scratch.alloc((n2 == 256 ? 1 : 2) * chunk * n * sizeof(cf32)));
            YG_TRY(make_split_twiddles(n, dir, p.fs_wsplit));
            p.d.fs_n1 = 256;
            p.d.fs_n2 = (int)n2;
            p.d.fs_p1 = &p.fs_p1->d;
            p.d.fs_p2 = &p.fs_p2->d;
            p.d.fs_scratch = p.fs_scratch.as<cf32>();
            p.d.fs_chunk = (int)chunk;
            p.d.fs_wlo = p.fs_wsplit.as<cf32>();
            p.d.fs_whi = p.fs_wsplit.as<cf32>() + 4096;
            return YAGI_OK;
        }
        auto smooth = [](size_t v) {
            for (size_t q = 2; q <= 89 && v > 1; ++q) while (v % q == 0) v /= q;
            return v == 1;
        };
        for (size_t d = (size_t)std::sqrt((double)n) + 1; d >= 2; --d)
            if (n % d == 0 && n / d <= (size_t)kFftMaxLds && d <= (size_t)kFftMaxLds && smooth(d) && smooth(n / d)) { n2 = d; break; }
        if (n2) {
            const size_t n1 = n / n2;
            p.fs_p1 = std::make_unique<FftPlan>();
            p.fs_p2 = std::make_unique<FftPlan>();
            YG_TRY(fft_plan_init(*p.fs_p1, n1, dir));
            YG_TRY(fft_plan_init(*p.fs_p2, n2, dir));
            size_t chunk = ((size_t)1 << 23) / n;              // 2 x 64 MiB of scratch
            if (chunk < 1) chunk = 1;
            YG_TRY(p.fs_scratch.alloc(2 * chunk * n * sizeof(cf32)));
            p.d.fs_n1 = (int)n1;
            p.d.fs_n2 = (int)n2;
            p.d.fs_p1 = &p.fs_p1->d;
            p.d.fs_p2 = &p.fs_p2->d;
            p.d.fs_scratch = p.fs_scratch.as<cf32>();
            p.d.fs_chunk = (int)chunk;
            YG_TRY(make_split_twiddles(n, dir, p.fs_wsplit));
            p.d.fs_wlo4 = p.fs_wsplit.as<cf32>();
            p.d.fs_whi4 = p.fs_wsplit.as<cf32>() + 4096;
            auto small_pow2 = [](size_t v) { return v >= 64 && v <= 256 && (v & (v - 1)) == 0; };
            if (small_pow2(n1) && small_pow2(n2)) {            // two-launch form (fft_kernels.hip: fft_twopass_kernel)
                YG_TRY(make_twiddles((int)n, dir, p.fs_wn));
                p.d.fs_wn = p.fs_wn.as<cf32>();
            }
            return YAGI_OK;
        }
        if (pow2) return fail(YAGI_ERR_INTERNAL, "no four-step split for %zu", n);
    }
    int maxp = 1;
    if (n <= (size_t)kFftMaxLds) {
        factorize((int)n, p.d.fac, p.d.nfac);
        YG_TRY(make_twiddles((int)n, dir, p.tw, n == 8192));
        p.d.tw = p.tw.as<cf32>();
        for (int i = 0; i < p.d.nfac; ++i) maxp = p.d.fac[i] > maxp ? p.d.fac[i] : maxp;
    }
    // A prime factor p costs O(n p) per transform in the mixed-radix kernel's direct-sum pass; beyond 89 (measured
    // crossover) -- and for every size that does not fit the one-kernel paths -- Bluestein's chirp-z form is used:
    //   X[k] = w[k] sum_j (x[j] w[j]) conj(w[k-j]),  w[k] = e^{-+ j pi k^2 / n}
    static const int bs_minp = getenv("YAGI_HIP_BLUESTEIN_MIN_PRIME") ? atoi(getenv("YAGI_HIP_BLUESTEIN_MIN_PRIME")) : 89;
    if (n > (size_t)kFftMaxLds || maxp > bs_minp) {
        size_t m = 1;
        while (m < 2 * n - 1) m *= 2;
        if (m < 256) m = 256;
        const double sgn = (dir == YAGI_FFT_FORWARD) ? -1.0 : 1.0;
        std::vector<cf32> w(n), b(m, cf32{0.f, 0.f});
        for (size_t k = 0; k < n; ++k) {
            const unsigned long long k2 = ((unsigned long long)k * k) % (2ull * n);      // exact phase index
            const double a = sgn * M_PI * (double)k2 / (double)n;
            w[k] = cf32{(float)std::cos(a), (float)std::sin(a)};
            const cf32 cw{w[k].re, -w[k].im};
            b[k] = cw;
            if (k) b[m - k] = cw;
        }
        YG_TRY(fill(p.bs_w, w.data(), n * sizeof(cf32), nullptr));
        // 2 x 64 MiB of scratch (more for one big transform).  With 2 x 16 MiB the five-stage form was launch-bound on long
        // batches (n = 12 289: 2400 launches of ~9 us for 2^28 points): 0.20 -> 0.30 TB/s, n = 509: 0.42 -> 0.59; 2 x 128 MiB the same
        static const int bs_lg = getenv("YAGI_HIP_BS_CHUNK_LOG2") ? atoi(getenv("YAGI_HIP_BS_CHUNK_LOG2")) : 23;
        size_t chunk = ((size_t)1 << (bs_lg < 16 ? 16 : (bs_lg > 26 ? 26 : bs_lg))) / m;
        if (chunk < 1) chunk = 1;
        if (m == 4096 || m == 8192) chunk = 1;                 // bluestein_fused_kernel: the scratch only serves FFT_m{b} below
        YG_TRY(p.bs_scratch.alloc(2 * chunk * m * sizeof(cf32)));
        YG_TRY(p.bs_bf.alloc(m * sizeof(cf32)));
        FftPlanDev f;                                          // FFT_m of the chirp filter by the device transform itself
        if (m > (size_t)kFftMaxLds) {
            p.bs_fwd = std::make_unique<FftPlan>();
            p.bs_bwd = std::make_unique<FftPlan>();
            YG_TRY(fft_plan_init(*p.bs_fwd, m, YAGI_FFT_FORWARD));
            YG_TRY(fft_plan_init(*p.bs_bwd, m, YAGI_FFT_BACKWARD));
            p.d.bs_fwd = &p.bs_fwd->d;
            p.d.bs_bwd = &p.bs_bwd->d;
            f = p.bs_fwd->d;
        } else {
            YG_TRY(make_twiddles((int)m, YAGI_FFT_FORWARD, p.bs_twf, m == 8192));
            YG_TRY(make_twiddles((int)m, YAGI_FFT_BACKWARD, p.bs_twb, m == 8192));
            f.n = (int)m;
            f.dir = YAGI_FFT_FORWARD;
            f.tw = p.bs_twf.as<cf32>();
        }
        YG_TRY(upload(p.bs_scratch.p, b.data(), m * sizeof(cf32), nullptr));
        YG_TRY(launch_fft_batch(f, p.bs_scratch.as<cf32>(), p.bs_bf.as<cf32>(), 1, nullptr));
        YG_HIP(hipStreamSynchronize(nullptr));
        p.d.bs_m = (int)m;
        p.d.bs_w = p.bs_w.as<cf32>();
        p.d.bs_bf = p.bs_bf.as<cf32>();
        p.d.bs_twf = p.bs_twf.as<cf32>();
        p.d.bs_twb = p.bs_twb.as<cf32>();
        p.d.bs_scratch = p.bs_scratch.as<cf32>();
        p.d.bs_chunk = (int)chunk;
    }
    return YAGI_OK;
}

// fast-convolution resources of a filter: FFT_4096{[h;0]} and both twiddle tables
template <class K>
int FirFilt<K>::prepare_conv() {
    if (conv_ready) return YAGI_OK;
    if (L > 2049) return fail(YAGI_ERR_CONFIG, "fast convolution needs <= 2049 taps");
    YG_TRY(make_stream_twiddles(twf));      // W_4096 forward table + the lane-indexed rows of the table-twiddle transform
    YG_TRY(make_twiddles(4096, YAGI_FFT_BACKWARD, twb));
    // FFT_4096{[h; 0]} evaluated in double on the host (L x 4096 terms, once per tap set), rounded once
    {
        std::vector<double> cs(4096), sn(4096);
        for (int m = 0; m < 4096; ++m) {
            const double a = -2.0 * M_PI * (double)m / 4096.0;
            cs[m] = std::cos(a);
            sn[m] = std::sin(a);
        }
        constexpr bool ctaps = sizeof(C) == sizeof(cf32);
        const float *hf = reinterpret_cast<const float *>(h.data());      // L floats, or L {re, im} pairs
        std::vector<cf32> hp(4096);
        for (int k = 0; k < 4096; ++k) {
            double re = 0.0, im = 0.0;
            for (int i = 0; i < L; ++i) {
                const int m = (int)(((long long)i * k) & 4095);
                const double hr = ctaps ? hf[2 * i] : hf[i], hi = ctaps ? hf[2 * i + 1] : 0.0;
                re += hr * cs[m] - hi * sn[m];
                im += hr * sn[m] + hi * cs[m];
            }
            hp[k] = cf32{(float)re, (float)im};
        }
        YG_TRY(fill(hfreq, hp.data(), 4096 * sizeof(cf32), st));
        // reversed taps g[j] = h[L-1-j] of the frame-boundary correction (freq_kernels.hip)
        if (K::id == 1 && L <= 257) {
            std::vector<float> g(256, 0.0f);
            for (int j = 0; j < L - 1; ++j) g[j] = hf[L - 1 - j];
            // the correction sum as a 512-point circular correlation: conj(DFT_512{g}) / 512 (freq_kernels.hip)
            std::vector<cf32> gf(512);
            for (int k = 0; k < 512; ++k) {
                double re = 0.0, im = 0.0;
                for (int j = 0; j < L - 1; ++j) {
                    const double a = -2.0 * M_PI * (double)((j * k) & 511) / 512.0;
                    re += (double)g[j] * std::cos(a);
                    im += (double)g[j] * std::sin(a);
                }
                gf[k] = cf32{(float)(re / 512.0), (float)(-im / 512.0)};
            }
            YG_TRY(fill(gfft, gf.data(), 512 * sizeof(cf32), st));
        }
        YG_HIP(hipStreamSynchronize(st));      // the host vectors go out of scope
    }
    conv_ready = true;
    return YAGI_OK;
}

// ---------------------------------------------------------------------------------------------
// fused firfilt_crcf -> FFT stream
// ---------------------------------------------------------------------------------------------
struct FirFft {
    FirFilt<CRCF> fir;
    size_t nfft = 0;
    DevBuf tw;
    FftPlan plan;              // nfft != 4096: overlap-save FIR, then this plan over the frames
    int variant = 0;
    Staging ws;
    DevBuf scratch;            // variant 3: the FIR output stream between the two kernels
    int join() { return fir.w.join(fir.st); }
};

// ---------------------------------------------------------------------------------------------
// channelizers
// ---------------------------------------------------------------------------------------------
struct PfbCh {
    hipStream_t st = nullptr;
    int M = 0, p = 0;
    DevBuf h, tw;
    DevWindow<cf32> hist;      // (p-1)*M samples (at least 1 kept so the buffers exist)
    DevWindow<cf32> syn_hist;  // synthesizer: the last (p-1)*M channel samples (its own state, like liquid's separate objects)
    Staging ws;
};
struct PfbCh2 {
    hipStream_t st = nullptr;
    int M = 0, m = 0;
    DevBuf h, tw;
    DevWindow<cf32> hist;      // (2m-1)*M + M/2 samples
    uint64_t step = 0;
    DevWindow<cf32> syn_hist;  // synthesizer: the last (4m-1)*M channel samples; its own step parity
    uint64_t syn_step = 0;
    Staging ws;
    DevBuf shard, gathered;    // sharded analyzer: this rank's sub-bands, and every rank's ([rank][step][M/R] per chunk)
};
struct PfbChr {
    hipStream_t st = nullptr;
    int M = 0, P = 0, m = 0;
    DevBuf h, tw;
    DevWindow<cf32> hist;      // 2Mm - P samples
    uint64_t step = 0;         // analyzer steps since the start of the stream: the commutator's rotation
    DevWindow<cf32> syn_hist;  // synthesizer: the last ceil(2Mm/P) - 1 steps, inverse-transformed ([step][M]); allocated by
    bool syn_ready = false;    // the first synthesizer call, so an analyzer-only object pays nothing for it
    int syn_rows = 0;
    // the synthesizer's state is limited here and not at create: its size says nothing about what the analyzer can hold
    int prepare_synthesizer() {
        if (syn_ready) return YAGI_OK;
        if ((size_t)syn_rows * (size_t)M > ((size_t)1 << 23))
            return fail(YAGI_ERR_CONFIG, "firpfbchr: synthesizer history of %d steps of %d channels is too large", syn_rows, M);
        YG_TRY(syn_hist.init((int)((size_t)syn_rows * (size_t)M), st));
        syn_ready = true;
        return YAGI_OK;
    }
    uint64_t syn_step = 0;
    DevBuf syn_v;              // the call's inverse transforms (chanr_kernels.hip: two launches)
    int choice = 0, last = 0;  // set_kernel / get_last_kernel
    Staging ws;
};

}  // namespace yagi

using namespace yagi;

#define CHECK_Q(q)                                                                              \
    do {                                                                                        \
        if (!(q)) return fail(YAGI_ERR_CONFIG, "null handle");                                  \
    } while (0)
// The block kernels read x (tile halos, the window after the block) while other workgroups already store y: an
// in-place or overlapping call would corrupt outputs AND the carried state.  Rust's borrow rules make it unwritable in
// the reference (&[T] and &mut [T] cannot alias); the C ABI says so explicitly.
static int check_noalias(const void *x, size_t xbytes, const void *y, size_t ybytes) {
    const char *a = static_cast<const char *>(x), *b = static_cast<const char *>(y);
    if (a < b + ybytes && b < a + xbytes)
        return fail(YAGI_ERR_CONFIG, "input and output buffers overlap (in-place execution is not supported)");
    return YAGI_OK;
}
#define CHECK_NOALIAS(x, nx, y, ny) YG_TRY(check_noalias((x), (size_t)(nx) * sizeof(*(x)), (y), (size_t)(ny) * sizeof(*(y))))
#define CHECK_PTR(p)                                                                            \
    do {                                                                                        \
        if (!(p)) return fail(YAGI_ERR_CONFIG, "null pointer argument");                        \
    } while (0)

extern "C" {

// ---- device plumbing ------------------------------------------------------------------------
int yagi_hip_device_count(int *count) try {
    CHECK_PTR(count);
    *count = 0;
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) { *count = 0; return fail(YAGI_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_set_device(int device) try { YG_HIP(hipSetDevice(device)); return YAGI_OK; } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_malloc(void **p, size_t bytes) try {
    CHECK_PTR(p);
    YG_TRY(require_device());
    YG_HIP(hipMalloc(p, bytes ? bytes : 16));
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_free(void *p) try { if (p) YG_HIP(hipFree(p)); return YAGI_OK; } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_memcpy_h2d(void *d, const void *s, size_t n) try { YG_HIP(hipMemcpy(d, s, n, hipMemcpyHostToDevice)); return YAGI_OK; } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_memcpy_d2h(void *d, const void *s, size_t n) try { YG_HIP(hipMemcpy(d, s, n, hipMemcpyDeviceToHost)); return YAGI_OK; } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_memset_dev(void *d, int v, size_t n) try { YG_HIP(hipMemset(d, v, n)); return YAGI_OK; } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_device_synchronize(void) try { YG_HIP(hipDeviceSynchronize()); return YAGI_OK; } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_stream_synchronize(yagi_stream_t s) try { YG_HIP(hipStreamSynchronize(to_stream(s))); return YAGI_OK; } catch (...) { return ::yagi::api_exception(); }

int yagi_hip_gen_real_dev(uint64_t seed, uint64_t first, size_t n, float *x, yagi_stream_t s) try {
    YG_TRY(require_device());
    return launch_gen_real(seed, first, n, x, to_stream(s));
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_gen_complex_dev(uint64_t seed, uint64_t first, size_t n, yagi_cf32 *x, yagi_stream_t s) try {
    YG_TRY(require_device());
    return launch_gen_complex(seed, first, n, x, to_stream(s));
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- dotprod ------------------------------------------------------------------------------------
template <class A, class B, class O>
static int dotprod_dev(const A *a, const B *b, size_t n, O *y, hipStream_t st) {
    YG_TRY(require_device());
    const size_t np = dotprod_num_partials(n);
    if (np == 1) return launch_dotprod<A, B, O, float>(a, b, n, false, 1.0f, y, y, st);
    // multi-workgroup case needs scratch for the partials: one grow-only buffer per host thread and device stream
    // user, kept for the life of the process (a per-call hipMalloc / hipFree pair costs more than the reduction of
    // 2^24 elements and forces a device synchronisation); calls on one stream are ordered, so reuse is safe there,
    // and concurrent streams of one thread are serialised by the event below
    // One scratch per host thread AND device (hipGetDevice): the buffer and its event belong to the device that was
    // current when they were made; after yagi_hip_set_device(other) the thread gets that device's own pair.  Released
    // at thread exit.
    struct Scratch { void *p = nullptr; size_t bytes = 0; hipEvent_t done = nullptr; };
    struct PerThread {
        std::vector<std::pair<int, Scratch>> dev;
        ~PerThread() {
            for (auto &e : dev) {
                int cur = -1;
                if (hipGetDevice(&cur) != hipSuccess) return;          // runtime already gone at process exit
                if (hipSetDevice(e.first) != hipSuccess) continue;
                if (e.second.done) (void)hipEventDestroy(e.second.done);
                if (e.second.p) (void)hipFree(e.second.p);
                (void)hipSetDevice(cur);
            }
        }
    };
    static thread_local PerThread pt;
    int devid = 0;
    YG_HIP(hipGetDevice(&devid));
    Scratch *scp = nullptr;
    for (auto &e : pt.dev) if (e.first == devid) scp = &e.second;
    if (!scp) { pt.dev.emplace_back(devid, Scratch{}); scp = &pt.dev.back().second; }
    Scratch &sc = *scp;
    const size_t need = np * sizeof(O);
    if (sc.done) YG_HIP(hipStreamWaitEvent(st, sc.done, 0));           // previous user of the scratch (any stream)
    else YG_HIP(hipEventCreateWithFlags(&sc.done, hipEventDisableTiming));
    if (need > sc.bytes) {
        if (sc.p) { YG_HIP(hipDeviceSynchronize()); YG_HIP(hipFree(sc.p)); sc.p = nullptr; sc.bytes = 0; }
        YG_HIP(hipMalloc(&sc.p, need + need / 2));
        sc.bytes = need + need / 2;
    }
    YG_TRY((launch_dotprod<A, B, O, float>(a, b, n, false, 1.0f, static_cast<O *>(sc.p), y, st)));
    YG_HIP(hipEventRecord(sc.done, st));
    return YAGI_OK;
}
template <class A, class B, class O>
static int dotprod_host(const A *a, const B *b, size_t n, O *y) {
    CHECK_PTR(y);
    if (n && (!a || !b)) return fail(YAGI_ERR_CONFIG, "null pointer argument");
    YG_TRY(require_device());
    DevBuf da, db, dy;
    YG_TRY(da.alloc(n * sizeof(A)));
    YG_TRY(db.alloc(n * sizeof(B)));
    YG_TRY(dy.alloc(sizeof(O)));
    YG_TRY(upload(da.p, a, n * sizeof(A), nullptr));
    YG_TRY(upload(db.p, b, n * sizeof(B), nullptr));
    YG_TRY((dotprod_dev<A, B, O>(da.as<A>(), db.as<B>(), n, dy.as<O>(), nullptr)));
    return download(y, dy.p, sizeof(O), nullptr);
}

extern "C" {
int yagi_hip_dotprod_rrrf(const float *a, const float *b, size_t n, float *y) try { return dotprod_host<float, float, float>(a, b, n, y); } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_dotprod_rccf(const float *a, const yagi_cf32 *b, size_t n, yagi_cf32 *y) try { return dotprod_host<float, cf32, cf32>(a, b, n, y); } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_dotprod_crcf(const yagi_cf32 *a, const float *b, size_t n, yagi_cf32 *y) try { return dotprod_host<cf32, float, cf32>(a, b, n, y); } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_dotprod_cccf(const yagi_cf32 *a, const yagi_cf32 *b, size_t n, yagi_cf32 *y) try { return dotprod_host<cf32, cf32, cf32>(a, b, n, y); } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_dotprod_rrrf_dev(const float *a, const float *b, size_t n, float *y, yagi_stream_t s) try { return dotprod_dev<float, float, float>(a, b, n, y, to_stream(s)); } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_dotprod_rccf_dev(const float *a, const yagi_cf32 *b, size_t n, yagi_cf32 *y, yagi_stream_t s) try { return dotprod_dev<float, cf32, cf32>(a, b, n, y, to_stream(s)); } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_dotprod_crcf_dev(const yagi_cf32 *a, const float *b, size_t n, yagi_cf32 *y, yagi_stream_t s) try { return dotprod_dev<cf32, float, cf32>(a, b, n, y, to_stream(s)); } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_dotprod_cccf_dev(const yagi_cf32 *a, const yagi_cf32 *b, size_t n, yagi_cf32 *y, yagi_stream_t s) try { return dotprod_dev<cf32, cf32, cf32>(a, b, n, y, to_stream(s)); } catch (...) { return ::yagi::api_exception(); }
}

// ---- FIR family: generic bodies, instantiated per type combination by YAGI_FIR_IMPL ----------------
namespace yagi {

template <class K>
static int firfilt_block_host(FirFilt<K> *q, const typename K::T *x, size_t nx, typename K::T *y, size_t ny) {
    using T = typename K::T;
    if (nx != ny) return fail(YAGI_ERR_CONFIG, "input and output block lengths must be equal");
    if (nx == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    YG_TRY(q->w.join(q->st));                            // the staging buffers are reused: host-pointer calls never pipeline
    return q->ws.run(q->st, x, nx, y, nx, [&](const T *xd, T *yd) {
        const bool was = q->w.pipe.on;
        q->w.pipe.on = false;
        const int rc = q->block_dev(xd, nx, yd);
        q->w.pipe.on = was;
        return rc;
    });
}

template <class K>
static int firdecim_block_host(FirDecim<K> *q, const typename K::T *x, size_t nx, size_t n, typename K::T *y) {
    using T = typename K::T;
    if (n == 0) return YAGI_OK;
    if (nx / (size_t)q->M < n) return fail(YAGI_ERR_CONFIG, "input block too short: need %zu samples, got %zu", n * (size_t)q->M, nx);
    CHECK_PTR(x);
    CHECK_PTR(y);
    const size_t nin = n * (size_t)q->M;
    return q->ws.run(q->st, x, nin, y, n, [&](const T *xd, T *yd) { return q->block_dev(xd, n, yd); });
}

template <class K>
static int firpfb_block_host(FirPfb<K> *q, size_t i, const typename K::T *x, size_t nx, typename K::T *y, size_t ny) {
    using T = typename K::T;
    YG_TRY(q->check_branch(i));
    const size_t n = nx < ny ? nx : ny;       // zip() stops at the shorter slice (firpfb.rs:296)
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    return q->ws.run(q->st, x, n, y, n, [&](const T *xd, T *yd) { return q->block_dev(i, xd, n, yd); });
}

}  // namespace yagi

// ComplexNotch (firfilt.rs:17-44): real coefficients design the notch at f0 directly (a notch pair at +-f0);
// complex coefficients design the DC blocker and mix it up to f0 (a single notch)
static int notch_taps(size_t m, float as_, float f0, std::vector<float> &h) { return design_notch(m, f0, as_, h); }
static int notch_taps(size_t m, float as_, float f0, std::vector<cf32> &h) {
    std::vector<float> hf;
    YG_TRY(design_notch(m, 0.0f, as_, hf));
    h.resize(hf.size());
    for (size_t i = 0; i < hf.size(); ++i) {
        const float phi = 2.0f * 3.14159265358979323846f * f0 * ((float)i - (float)m);
        h[i] = cf32{hf[i] * std::cos(phi), hf[i] * std::sin(phi)};
    }
    return YAGI_OK;
}

// freqresponse (design/mod.rs:666-675): H(fc) = sum_i h[i] e^{-j 2 pi fc i}, the phasor in f64 rounded to f32, the sum in
// Complex32; fir_group_delay (:687-704): Re(sum_i i h[i] e^{+j 2 pi fc i} / sum_i h[i] e^{+j 2 pi fc i}) on the real parts
static cf32 cx_val(float v) { return cf32{v, 0.0f}; }
static cf32 cx_val(cf32 v) { return v; }
template <class C>
static cf32 taps_freqresponse(const std::vector<C> &h, float fc) {
    cf32 acc{0.0f, 0.0f};
    for (size_t i = 0; i < h.size(); ++i) {
        const double a = -2.0 * M_PI * (double)fc * (double)i;
        const cf32 e{(float)std::cos(a), (float)std::sin(a)}, v = cx_val(h[i]);
        acc.re += v.re * e.re - v.im * e.im;
        acc.im += v.re * e.im + v.im * e.re;
    }
    return acc;
}
static cf32 cx_mul(cf32 a, cf32 b) { return cf32{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
template <class C>
static int taps_groupdelay(const std::vector<C> &h, float fc, float *out) {
    if (h.empty()) return fail(YAGI_ERR_CONFIG, "fir_group_delay(), length must be greater than zero");
    if (fc < -0.5f || fc > 0.5f) return fail(YAGI_ERR_CONFIG, "fir_group_delay(), _fc must be in [-0.5,0.5]");
    cf32 t0{0.f, 0.f}, t1{0.f, 0.f};
    for (size_t i = 0; i < h.size(); ++i) {
        const float a = 2.0f * 3.14159265358979323846f * fc * (float)i, hr = cx_val(h[i]).re;
        const cf32 e{std::cos(a), std::sin(a)};
        t0.re += hr * e.re * (float)i;
        t0.im += hr * e.im * (float)i;
        t1.re += hr * e.re;
        t1.im += hr * e.im;
    }
    const float den = t1.re * t1.re + t1.im * t1.im;
    *out = (t0.re * t1.re + t0.im * t1.im) / den;
    return YAGI_OK;
}

#define YAGI_FIR_IMPL(K, KT, T, C)                                                                  \
    struct yagi_hip_firfilt_##K##_s : FirFilt<KT> {};                                               \
    struct yagi_hip_firdecim_##K##_s : FirDecim<KT> {};                                             \
    struct yagi_hip_firpfb_##K##_s : FirPfb<KT> {};                                                 \
    extern "C" {                                                                                    \
    int yagi_hip_firfilt_##K##_create(const C *h, size_t h_len, yagi_hip_firfilt_##K *q) try {      \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (h_len && !h) return fail(YAGI_ERR_CONFIG, "null pointer argument");                     \
        auto o = std::make_unique<yagi_hip_firfilt_##K##_s>();                                      \
        YG_TRY(o->init(h, h_len));                                                                  \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_create_kaiser(size_t n, float fc, float as_, float mu,               \
                                             yagi_hip_firfilt_##K *q) try {                         \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        std::vector<float> hf;                                                                      \
        YG_TRY(design_kaiser(n, fc, as_, mu, hf));                                                  \
        std::vector<C> hc(hf.size());                                                               \
        for (size_t i = 0; i < hf.size(); ++i) hc[i] = to_c(hf[i], (C *)nullptr);                   \
        return yagi_hip_firfilt_##K##_create(hc.data(), hc.size(), q);                              \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_create_rnyquist(int ftype, size_t k, size_t m, float beta, float mu, \
                                               yagi_hip_firfilt_##K *q) try {                       \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        std::vector<float> hf;                                                                      \
        YG_TRY(design_prototype(ftype, k, m, beta, mu, hf));                                        \
        std::vector<C> hc(hf.size());                                                               \
        for (size_t i = 0; i < hf.size(); ++i) hc[i] = to_c(hf[i], (C *)nullptr);                   \
        return yagi_hip_firfilt_##K##_create(hc.data(), hc.size(), q);                              \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_create_rect(size_t n, yagi_hip_firfilt_##K *q) try {                 \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (n == 0 || n > 1024) return fail(YAGI_ERR_CONFIG, "filter length must be in [1,1024]");  \
        std::vector<C> hc(n, one_of<C>());                                                          \
        return yagi_hip_firfilt_##K##_create(hc.data(), hc.size(), q);                              \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_create_notch(size_t m, float as_, float f0, yagi_hip_firfilt_##K *q) try { \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        std::vector<C> hc;                                                                          \
        YG_TRY(notch_taps(m, as_, f0, hc));                                                         \
        return yagi_hip_firfilt_##K##_create(hc.data(), hc.size(), q);                              \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_create_dc_blocker(size_t m, float as_, yagi_hip_firfilt_##K *q) try { \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        std::vector<float> hf;                                                                      \
        YG_TRY(design_notch(m, 0.0f, as_, hf));                                                     \
        std::vector<C> hc(hf.size());                                                               \
        for (size_t i = 0; i < hf.size(); ++i) hc[i] = to_c(hf[i], (C *)nullptr);                   \
        return yagi_hip_firfilt_##K##_create(hc.data(), hc.size(), q);                              \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_destroy(yagi_hip_firfilt_##K q) try {                                \
        delete q;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_clone(yagi_hip_firfilt_##K q, yagi_hip_firfilt_##K *out) try {       \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        YG_TRY(q->w.ensure_dev(q->st));                                                                  \
        auto o = std::make_unique<yagi_hip_firfilt_##K##_s>();                                      \
        o->st = q->st;                                                                              \
        YG_TRY(o->init(q->h.data(), q->h.size()));                                                  \
        o->scale = q->scale;                                                                        \
        o->kernel_choice = q->kernel_choice;                                                        \
        YG_TRY(o->w.clone_from(q->w, q->st));                                                       \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_set_stream(yagi_hip_firfilt_##K q, yagi_stream_t s) try {            \
        CHECK_Q(q);                                                                                 \
        if (q->st == to_stream(s)) return YAGI_OK;                                                  \
        YG_TRY(q->w.join(q->st));                                                                   \
        YG_HIP(hipStreamSynchronize(q->st));                                                        \
        q->st = to_stream(s);                                                                       \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_set_pipeline(yagi_hip_firfilt_##K q, int on) try {                   \
        CHECK_Q(q);                                                                                 \
        YG_TRY(q->w.join(q->st));                                                                   \
        if (on) YG_TRY(q->w.pipe.init());                                                           \
        q->w.pipe.on = on != 0;                                                                     \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_join(yagi_hip_firfilt_##K q) try {                                   \
        CHECK_Q(q);                                                                                 \
        return q->w.join(q->st);                                                                    \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_set_coefficients(yagi_hip_firfilt_##K q, const C *h, size_t n) try { \
        CHECK_Q(q);                                                                                 \
        if (n && !h) return fail(YAGI_ERR_CONFIG, "null pointer argument");                         \
        YG_TRY(q->w.join(q->st));                                                                   \
        YG_HIP(hipStreamSynchronize(q->st));                                                        \
        const bool resize = (n != (size_t)q->L);                                                    \
        YG_TRY(q->load_taps(h, n));                                                                 \
        if (resize) return q->w.init(q->L, q->st);                                                  \
        return q->w.reset(q->st);                                                                   \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_reset(yagi_hip_firfilt_##K q) try {                                  \
        CHECK_Q(q);                                                                                 \
        return q->w.reset(q->st);                                                                   \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_push(yagi_hip_firfilt_##K q, T x) try {                              \
        CHECK_Q(q);                                                                                 \
        YG_TRY(q->w.ensure_host(q->st));                                                            \
        q->w.push(x);                                                                               \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_write(yagi_hip_firfilt_##K q, const T *x, size_t n) try {            \
        CHECK_Q(q);                                                                                 \
        if (n && !x) return fail(YAGI_ERR_CONFIG, "null pointer argument");                         \
        YG_TRY(q->w.ensure_host(q->st));                                                            \
        for (size_t i = 0; i < n; ++i) q->w.push(x[i]);                                             \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_execute(yagi_hip_firfilt_##K q, T *y) try {                          \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(y);                                                                               \
        YG_TRY(q->w.ensure_host(q->st));                                                            \
        *y = q->host_execute();                                                                     \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_execute_one(yagi_hip_firfilt_##K q, T x, T *y) try {                 \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(y);                                                                               \
        YG_TRY(q->w.ensure_host(q->st));                                                            \
        q->w.push(x);                                                                               \
        *y = q->host_execute();                                                                     \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_execute_block(yagi_hip_firfilt_##K q, const T *x, size_t nx, T *y,   \
                                             size_t ny) try {                                       \
        CHECK_Q(q);                                                                                 \
        return firfilt_block_host<KT>(q, x, nx, y, ny);                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_execute_block_dev(yagi_hip_firfilt_##K q, const T *x, size_t n,      \
                                                 T *y) try {                                        \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        CHECK_NOALIAS(x, n, y, n);                                                                  \
        return q->block_dev(x, n, y);                                                               \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_set_scale(yagi_hip_firfilt_##K q, C s) try {                         \
        CHECK_Q(q);                                                                                 \
        q->scale = s;                                                                               \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_get_scale(yagi_hip_firfilt_##K q, C *s) try {                        \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(s);                                                                               \
        *s = q->scale;                                                                              \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_get_length(yagi_hip_firfilt_##K q, size_t *n) try {                  \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(n);                                                                               \
        *n = (size_t)q->L;                                                                          \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_get_coefficients(yagi_hip_firfilt_##K q, C *h, size_t n) try {       \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(h);                                                                               \
        if (n < (size_t)q->L) return fail(YAGI_ERR_CONFIG, "coefficient buffer too short");         \
        std::memcpy(h, q->h.data(), (size_t)q->L * sizeof(C));                                      \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_freqresponse(yagi_hip_firfilt_##K q, float fc, yagi_cf32 *H) try {   \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(H);                                                                               \
        *H = cx_mul(taps_freqresponse(q->h, fc), cx_val(q->scale));                                 \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firfilt_##K##_groupdelay(yagi_hip_firfilt_##K q, float fc, float *delay) try {     \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(delay);                                                                           \
        return taps_groupdelay(q->h, fc, delay);                                                    \
    } catch (...) { return ::yagi::api_exception(); }                                               \
                                                                                                    \
    int yagi_hip_firdecim_##K##_create(size_t M, const C *h, size_t h_len,                          \
                                       yagi_hip_firdecim_##K *q) try {                              \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (h_len && !h) return fail(YAGI_ERR_CONFIG, "null pointer argument");                     \
        auto o = std::make_unique<yagi_hip_firdecim_##K##_s>();                                     \
        YG_TRY(o->init(M, h, h_len));                                                               \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firdecim_##K##_create_kaiser(size_t M, size_t m, float as_,                        \
                                              yagi_hip_firdecim_##K *q) try {                       \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (M < 2) return fail(YAGI_ERR_CONFIG, "decim factor must be greater than 1");             \
        if (m == 0) return fail(YAGI_ERR_CONFIG, "filter delay must be greater than 0");            \
        if (as_ < 0.0f) return fail(YAGI_ERR_CONFIG, "stop-band attenuation must be positive");     \
        std::vector<float> hf;                                                                      \
        YG_TRY(design_kaiser(2 * M * m + 1, 0.5f / (float)M, as_, 0.0f, hf));                       \
        std::vector<C> hc(hf.size());                                                               \
        for (size_t i = 0; i < hf.size(); ++i) hc[i] = to_c(hf[i], (C *)nullptr);                   \
        return yagi_hip_firdecim_##K##_create(M, hc.data(), hc.size(), q);                          \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firdecim_##K##_create_prototype(int ftype, size_t M, size_t m, float beta,         \
                                                 float dt, yagi_hip_firdecim_##K *q) try {          \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (M < 2) return fail(YAGI_ERR_CONFIG, "decimation factor must be greater than 1");        \
        if (m == 0) return fail(YAGI_ERR_CONFIG, "filter delay must be greater than 0");            \
        if (beta < 0.0f || beta > 1.0f)                                                             \
            return fail(YAGI_ERR_CONFIG, "filter excess bandwidth factor must be in [0,1]");        \
        if (dt < -1.0f || dt > 1.0f)                                                                \
            return fail(YAGI_ERR_CONFIG, "filter fractional sample delay must be in [-1,1]");       \
        std::vector<float> hf;                                                                      \
        YG_TRY(design_prototype(ftype, M, m, beta, dt, hf));                                        \
        std::vector<C> hc(hf.size());                                                               \
        for (size_t i = 0; i < hf.size(); ++i) hc[i] = to_c(hf[i], (C *)nullptr);                   \
        return yagi_hip_firdecim_##K##_create(M, hc.data(), hc.size(), q);                          \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firdecim_##K##_destroy(yagi_hip_firdecim_##K q) try {                              \
        delete q;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firdecim_##K##_clone(yagi_hip_firdecim_##K q, yagi_hip_firdecim_##K *out) try {    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        YG_TRY(q->w.ensure_dev(q->st));                                                                  \
        auto o = std::make_unique<yagi_hip_firdecim_##K##_s>();                                     \
        o->st = q->st;                                                                              \
        YG_TRY(o->init((size_t)q->M, q->h.data(), q->h.size()));                                    \
        o->scale = q->scale;                                                                        \
        YG_TRY(o->w.clone_from(q->w, q->st));                                                       \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firdecim_##K##_set_stream(yagi_hip_firdecim_##K q, yagi_stream_t s) try {          \
        CHECK_Q(q);                                                                                 \
        if (q->st == to_stream(s)) return YAGI_OK;                                                  \
        YG_HIP(hipStreamSynchronize(q->st));                                                        \
        q->st = to_stream(s);                                                                       \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firdecim_##K##_reset(yagi_hip_firdecim_##K q) try {                                \
        CHECK_Q(q);                                                                                 \
        return q->w.reset(q->st);                                                                   \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firdecim_##K##_get_decim_rate(yagi_hip_firdecim_##K q, size_t *M) try {            \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(M);                                                                               \
        *M = (size_t)q->M;                                                                          \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firdecim_##K##_set_scale(yagi_hip_firdecim_##K q, C s) try {                       \
        CHECK_Q(q);                                                                                 \
        q->scale = s;                                                                               \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firdecim_##K##_get_scale(yagi_hip_firdecim_##K q, C *s) try {                      \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(s);                                                                               \
        *s = q->scale;                                                                              \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firdecim_##K##_freqresp(yagi_hip_firdecim_##K q, float fc, yagi_cf32 *H) try {     \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(H);                                                                               \
        *H = cx_mul(taps_freqresponse(q->h, fc), cx_val(q->scale));                                 \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firdecim_##K##_execute(yagi_hip_firdecim_##K q, const T *x, size_t nx, T *y) try { \
        CHECK_Q(q);                                                                                 \
        if (nx < (size_t)q->M) return fail(YAGI_ERR_CONFIG, "input block too short: need %zu samples, got %zu", (size_t)q->M, nx); \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        YG_TRY(q->w.ensure_host(q->st));                       /* firdecim.rs:179-191: output after the FIRST of the M pushes */ \
        q->w.push(x[0]);                                                                            \
        *y = host_fir_window_dot<T, C>(q->w.host(), (size_t)q->L, q->h.data(), q->scale);           \
        for (int i = 1; i < q->M; ++i) q->w.push(x[i]);                                             \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firdecim_##K##_execute_block(yagi_hip_firdecim_##K q, const T *x, size_t nx,       \
                                              size_t n, T *y) try {                                 \
        CHECK_Q(q);                                                                                 \
        return firdecim_block_host<KT>(q, x, nx, n, y);                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firdecim_##K##_execute_block_dev(yagi_hip_firdecim_##K q, const T *x, size_t n,    \
                                                  T *y) try {                                       \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        CHECK_NOALIAS(x, n * (size_t)q->M, y, n);                                                   \
        return q->block_dev(x, n, y);                                                               \
    } catch (...) { return ::yagi::api_exception(); }                                               \
                                                                                                    \
    int yagi_hip_firpfb_##K##_create(size_t nf, const C *h, size_t h_len, yagi_hip_firpfb_##K *q) try { \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (h_len && !h) return fail(YAGI_ERR_CONFIG, "null pointer argument");                     \
        auto o = std::make_unique<yagi_hip_firpfb_##K##_s>();                                       \
        YG_TRY(o->init(nf, h, h_len));                                                              \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_create_kaiser(size_t nf, size_t m, float fc, float as_,               \
                                            yagi_hip_firpfb_##K *q) try {                           \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (nf == 0) return fail(YAGI_ERR_CONFIG, "number of filters must be greater than zero");   \
        if (m == 0) return fail(YAGI_ERR_CONFIG, "filter delay must be greater than 0");            \
        if (fc <= 0.0f || fc > 0.5f)                                                                \
            return fail(YAGI_ERR_CONFIG, "filter cut-off frequency must be in (0,0.5)");            \
        if (as_ < 0.0f) return fail(YAGI_ERR_CONFIG, "filter stop-band suppression must be positive"); \
        std::vector<float> hf;                                                                      \
        YG_TRY(design_kaiser(2 * nf * m + 1, fc / (float)nf, as_, 0.0f, hf));                       \
        std::vector<C> hc(hf.size());                                                               \
        for (size_t i = 0; i < hf.size(); ++i) hc[i] = to_c(hf[i], (C *)nullptr);                   \
        return yagi_hip_firpfb_##K##_create(nf, hc.data(), hc.size(), q);                           \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_create_default(size_t nf, size_t m, yagi_hip_firpfb_##K *q) try {     \
        return yagi_hip_firpfb_##K##_create_kaiser(nf, m, 0.5f, 60.0f, q);                          \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_destroy(yagi_hip_firpfb_##K q) try {                                  \
        delete q;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_clone(yagi_hip_firpfb_##K q, yagi_hip_firpfb_##K *out) try {          \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        YG_TRY(q->w.ensure_dev(q->st));                                                                  \
        auto o = std::make_unique<yagi_hip_firpfb_##K##_s>();                                       \
        o->st = q->st;                                                                              \
        o->nf = q->nf;                                                                              \
        o->Ls = q->Ls;                                                                              \
        o->hb = q->hb;                                                                              \
        o->scale = q->scale;                                                                        \
        YG_TRY(fill(o->taps, o->hb.data(), o->hb.size() * sizeof(C), o->st));                       \
        YG_TRY(o->w.clone_from(q->w, q->st));                                                       \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_set_stream(yagi_hip_firpfb_##K q, yagi_stream_t s) try {              \
        CHECK_Q(q);                                                                                 \
        if (q->st == to_stream(s)) return YAGI_OK;                                                  \
        YG_HIP(hipStreamSynchronize(q->st));                                                        \
        q->st = to_stream(s);                                                                       \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_reset(yagi_hip_firpfb_##K q) try {                                    \
        CHECK_Q(q);                                                                                 \
        return q->w.reset(q->st);                                                                   \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_set_scale(yagi_hip_firpfb_##K q, C s) try {                           \
        CHECK_Q(q);                                                                                 \
        q->scale = s;                                                                               \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_get_scale(yagi_hip_firpfb_##K q, C *s) try {                          \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(s);                                                                               \
        *s = q->scale;                                                                              \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_push(yagi_hip_firpfb_##K q, T x) try {                                \
        CHECK_Q(q);                                                                                 \
        YG_TRY(q->w.ensure_host(q->st));                                                            \
        q->w.push(x);                                                                               \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_write(yagi_hip_firpfb_##K q, const T *x, size_t n) try {              \
        CHECK_Q(q);                                                                                 \
        if (n && !x) return fail(YAGI_ERR_CONFIG, "null pointer argument");                         \
        YG_TRY(q->w.ensure_host(q->st));                                                            \
        for (size_t i = 0; i < n; ++i) q->w.push(x[i]);                                             \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_execute(yagi_hip_firpfb_##K q, size_t i, T *y) try {                  \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(y);                                                                               \
        YG_TRY(q->check_branch(i));                                                                 \
        YG_TRY(q->w.ensure_host(q->st));                                                            \
        *y = host_fir_window_dot<T, C>(q->w.host(), (size_t)q->Ls, q->hb.data() + i * (size_t)q->Ls, q->scale); \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_execute_block(yagi_hip_firpfb_##K q, size_t i, const T *x, size_t nx, \
                                            T *y, size_t ny) try {                                  \
        CHECK_Q(q);                                                                                 \
        return firpfb_block_host<KT>(q, i, x, nx, y, ny);                                           \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_execute_block_dev(yagi_hip_firpfb_##K q, size_t i, const T *x,        \
                                                size_t n, T *y) try {                               \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return q->check_branch(i);                                                      \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        CHECK_NOALIAS(x, n, y, n);                                                                  \
        return q->block_dev(i, x, n, y);                                                            \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_execute_all_dev(yagi_hip_firpfb_##K q, const T *x, size_t n, T *y) try { \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        CHECK_NOALIAS(x, n, y, n * (size_t)q->nf);                                                  \
        YG_TRY(q->w.ensure_dev(q->st));                                                                  \
        YG_TRY((launch_firpfb_all<KT>(q->w.dev(), x, q->taps.as<C>(), q->nf, q->Ls, q->scale, y, n, \
                                      q->st)));                                                     \
        return q->w.advance(x, n, q->st);                                                           \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firpfb_##K##_execute_select_dev(yagi_hip_firpfb_##K q, const uint32_t *idx,        \
                                                 const T *x, size_t n, T *y) try {                  \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(idx);                                                                             \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        CHECK_NOALIAS(x, n, y, n);                                                                  \
        YG_TRY(q->w.ensure_dev(q->st));                                                                  \
        YG_TRY((launch_firpfb_select<KT>(q->w.dev(), x, q->taps.as<C>(), idx, q->nf, q->Ls,         \
                                         q->scale, y, n, q->st)));                                  \
        return q->w.advance(x, n, q->st);                                                           \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_FIR_IMPL(rrrf, RRRF, float, float)
YAGI_FIR_IMPL(crcf, CRCF, yagi_cf32, float)
YAGI_FIR_IMPL(cccf, CCCF, yagi_cf32, yagi_cf32)

// which block kernel execute_block uses: 0 auto, 1 general direct form, 4 overlap-save fast convolution (<= 2049
// taps); crcf also 2 register-sliding direct form (<= 1024 taps) and 3 MFMA Toeplitz direct form (<= 256 taps)
template <class Q>
static int firfilt_set_kernel(Q *q, int choice, bool crcf) {
    CHECK_Q(q);
    if (choice < 0 || choice > 4 || (!crcf && (choice == 2 || choice == 3)))
        return fail(YAGI_ERR_CONFIG, "unknown kernel choice %d", choice);
    if (choice == 4 && q->L > 2049) return fail(YAGI_ERR_CONFIG, "fast convolution needs <= 2049 taps");
    q->kernel_choice = choice;
    return YAGI_OK;
}
extern "C" int yagi_hip_firfilt_rrrf_set_kernel(yagi_hip_firfilt_rrrf q, int choice) { return firfilt_set_kernel(q, choice, false); }
extern "C" int yagi_hip_firfilt_crcf_set_kernel(yagi_hip_firfilt_crcf q, int choice) { return firfilt_set_kernel(q, choice, true); }
extern "C" int yagi_hip_firfilt_cccf_set_kernel(yagi_hip_firfilt_cccf q, int choice) { return firfilt_set_kernel(q, choice, false); }

// ---- Fft --------------------------------------------------------------------------------------------
struct yagi_hip_fft_s : FftPlan {};

extern "C" {

int yagi_hip_fft_create(size_t n, int direction, yagi_hip_fft *plan) try {
    CHECK_PTR(plan);
    *plan = nullptr;
    auto p = std::make_unique<yagi_hip_fft_s>();
    YG_TRY(fft_plan_init(*p, n, direction));
    *plan = p.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_fft_destroy(yagi_hip_fft plan) try { delete plan; return YAGI_OK; } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_fft_clone(yagi_hip_fft plan, yagi_hip_fft *out) try {
    CHECK_Q(plan);
    return yagi_hip_fft_create((size_t)plan->d.n, plan->d.dir, out);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_fft_len(yagi_hip_fft plan, size_t *n) try {
    CHECK_Q(plan);
    CHECK_PTR(n);
    *n = (size_t)plan->d.n;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_fft_describe(yagi_hip_fft plan, yagi_hip_fft_info *info) try {
    CHECK_Q(plan);
    CHECK_PTR(info);
    fft_describe(plan->d, *info);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_fft_run_batch_dev(yagi_hip_fft plan, const yagi_cf32 *in, yagi_cf32 *out, size_t batch,
                               yagi_stream_t s) try {
    CHECK_Q(plan);
    if (batch == 0) return YAGI_OK;
    CHECK_PTR(in);
    CHECK_PTR(out);
    return launch_fft_batch(plan->d, in, out, batch, to_stream(s));
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_fft_run(yagi_hip_fft plan, const yagi_cf32 *input, size_t n_in, yagi_cf32 *output, size_t n_out) try {
    CHECK_Q(plan);
    const size_t n = (size_t)plan->d.n;
    // the reference panics on a length mismatch (copy_from_slice, fft/mod.rs:46)
    if (n_in != n || n_out != n) return fail(YAGI_ERR_CONFIG, "fft buffers must hold exactly %zu samples", n);
    CHECK_PTR(input);
    CHECK_PTR(output);
    return plan->ws.run(nullptr, input, n, output, n,
                        [&](const cf32 *xd, cf32 *yd) { return launch_fft_batch(plan->d, xd, yd, 1, nullptr); });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_fft_shift_dev(yagi_cf32 *buf, size_t n, size_t batch, yagi_stream_t s) try {
    if (n == 0 || batch == 0) return YAGI_OK;
    CHECK_PTR(buf);
    YG_TRY(require_device());
    return launch_fft_shift(buf, n, batch, to_stream(s));
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_fft_shift(yagi_cf32 *buf, size_t n) try {
    if (n < 2) return YAGI_OK;
    CHECK_PTR(buf);
    YG_TRY(require_device());
    DevBuf d;
    YG_TRY(fill(d, buf, n * sizeof(cf32), nullptr));
    YG_TRY(launch_fft_shift(d.as<cf32>(), n, 1, nullptr));
    return download(buf, d.p, n * sizeof(cf32), nullptr);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_fft_run_oneshot(const yagi_cf32 *input, yagi_cf32 *output, size_t n, int direction) try {
    yagi_hip_fft p = nullptr;
    YG_TRY(yagi_hip_fft_create(n, direction, &p));
    int rc = yagi_hip_fft_run(p, input, n, output, n);
    yagi_hip_fft_destroy(p);
    return rc;
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- FirInterpolationFilter (src/filter/fir/firinterp.rs): a FirPfb bank run over every branch -------
namespace yagi {

template <class K>
struct FirInterp {
    using T = typename K::T;
    using C = typename K::C;
    FirPfb<K> bank;
    int interp = 0, hs = 0;

    int init(size_t m, const C *h, size_t h_len) {
        if (m < 2) return fail(YAGI_ERR_CONFIG, "interp factor must be greater than 1");
        if (h_len < m) return fail(YAGI_ERR_CONFIG, "filter length cannot be less than interp factor");
        size_t sub = 0;
        while (m * sub < h_len) ++sub;                       // firinterp.rs:44-47
        std::vector<C> hp(m * sub, C{});
        for (size_t i = 0; i < h_len; ++i) hp[i] = h[i];
        YG_TRY(bank.init(m, hp.data(), hp.size()));
        interp = (int)m;
        hs = (int)sub;
        return YAGI_OK;
    }
    // n inputs -> n*interp outputs (device pointers)
    int block_dev(const T *x, size_t n, T *y) {
        YG_TRY(bank.w.ensure_dev(bank.st));
        if (n == 0) return YAGI_OK;
        YG_TRY((launch_firpfb_all<K>(bank.w.dev(), x, bank.taps.template as<C>(), bank.nf, bank.Ls,
                                     bank.scale, y, n, bank.st, bank.w.next())));
        bank.w.flip();                              // the kernel's last workgroup wrote the next window
        return YAGI_OK;
    }
    int block_host(const T *x, size_t n, T *y) {
        if (n == 0) return YAGI_OK;
        return bank.ws.run(bank.st, x, n, y, n * (size_t)interp, [&](const T *xd, T *yd) { return block_dev(xd, n, yd); });
    }
};

// new_prototype (firinterp.rs:105-124): its checks, then all 2 interp m + 1 taps of the design
static int firinterp_prototype_taps(int ftype, size_t interp, size_t m, float beta, float dt, std::vector<float> &hf) {
    if (interp < 2) return fail(YAGI_ERR_CONFIG, "interp factor must be greater than 1");
    if (m == 0) return fail(YAGI_ERR_CONFIG, "filter delay must be greater than 0");
    if (beta < 0.0f || beta > 1.0f) return fail(YAGI_ERR_CONFIG, "filter excess bandwidth factor must be in [0,1]");
    if (dt < -1.0f || dt > 1.0f) return fail(YAGI_ERR_CONFIG, "filter fractional sample delay must be in [-1,1]");
    return design_prototype(ftype, interp, m, beta, dt, hf);
}

}  // namespace yagi

#define YAGI_FIRINTERP_IMPL(K, KT, T, C)                                                            \
    struct yagi_hip_firinterp_##K##_s : FirInterp<KT> {};                                           \
    extern "C" {                                                                                    \
    int yagi_hip_firinterp_##K##_create(size_t interp, const C *h, size_t h_len,                    \
                                        yagi_hip_firinterp_##K *q) try {                            \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (h_len && !h) return fail(YAGI_ERR_CONFIG, "null pointer argument");                     \
        auto o = std::make_unique<yagi_hip_firinterp_##K##_s>();                                    \
        YG_TRY(o->init(interp, h, h_len));                                                          \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_create_kaiser(size_t interp, size_t m, float as_,                  \
                                               yagi_hip_firinterp_##K *q) try {                     \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (interp < 2) return fail(YAGI_ERR_CONFIG, "interp factor must be greater than 1");       \
        if (m == 0) return fail(YAGI_ERR_CONFIG, "filter delay must be greater than 0");            \
        if (as_ < 0.0f) return fail(YAGI_ERR_CONFIG, "stop-band attenuation must be positive");     \
        std::vector<float> hf;                                                                      \
        YG_TRY(design_kaiser(2 * interp * m + 1, 0.5f / (float)interp, as_, 0.0f, hf));             \
        std::vector<C> hc(hf.size());                                                               \
        for (size_t i = 0; i < hf.size(); ++i) hc[i] = to_c(hf[i], (C *)nullptr);                   \
        return yagi_hip_firinterp_##K##_create(interp, hc.data(), hc.size() - 1, q);                \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_create_prototype(int ftype, size_t interp, size_t m, float beta,   \
                                                  float dt, yagi_hip_firinterp_##K *q) try {        \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        std::vector<float> hf;                                                                      \
        YG_TRY(firinterp_prototype_taps(ftype, interp, m, beta, dt, hf));                           \
        std::vector<C> hc(hf.size());                                                               \
        for (size_t i = 0; i < hf.size(); ++i) hc[i] = to_c(hf[i], (C *)nullptr);                   \
        return yagi_hip_firinterp_##K##_create(interp, hc.data(), hc.size(), q);                    \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_create_linear(size_t interp, yagi_hip_firinterp_##K *q) try {      \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (interp < 1) return fail(YAGI_ERR_CONFIG, "interp factor must be greater than 1");       \
        std::vector<C> hc(2 * interp);                                                              \
        for (size_t i = 0; i < interp; ++i) {                                                       \
            hc[i] = to_c((float)i / (float)interp, (C *)nullptr);                                   \
            hc[interp + i] = to_c(1.0f - (float)i / (float)interp, (C *)nullptr);                   \
        }                                                                                           \
        return yagi_hip_firinterp_##K##_create(interp, hc.data(), hc.size(), q);                    \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_create_window(size_t interp, size_t m, yagi_hip_firinterp_##K *q) try { \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (interp < 1) return fail(YAGI_ERR_CONFIG, "interp factor must be greater than 1");       \
        if (m < 1) return fail(YAGI_ERR_CONFIG, "filter semi-length must be greater than 0");       \
        const size_t hl = 2 * m * interp;                                                           \
        std::vector<C> hc(hl);                                                                      \
        for (size_t i = 0; i < hl; ++i) {                                                           \
            const float sv = std::sin(3.14159265358979323846f * (float)i / (float)(2 * m * interp));\
            hc[i] = to_c(sv * sv, (C *)nullptr);                                                    \
        }                                                                                           \
        return yagi_hip_firinterp_##K##_create(interp, hc.data(), hl, q);                           \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_destroy(yagi_hip_firinterp_##K q) try {                            \
        delete q;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_clone(yagi_hip_firinterp_##K q, yagi_hip_firinterp_##K *out) try { \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        YG_TRY(q->bank.w.ensure_dev(q->bank.st));                                                        \
        auto o = std::make_unique<yagi_hip_firinterp_##K##_s>();                                    \
        o->interp = q->interp;                                                                      \
        o->hs = q->hs;                                                                              \
        o->bank.st = q->bank.st;                                                                    \
        o->bank.nf = q->bank.nf;                                                                    \
        o->bank.Ls = q->bank.Ls;                                                                    \
        o->bank.hb = q->bank.hb;                                                                    \
        o->bank.scale = q->bank.scale;                                                              \
        YG_TRY(fill(o->bank.taps, o->bank.hb.data(), o->bank.hb.size() * sizeof(C), o->bank.st));   \
        YG_TRY(o->bank.w.clone_from(q->bank.w, q->bank.st));                                        \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_set_stream(yagi_hip_firinterp_##K q, yagi_stream_t s) try {        \
        CHECK_Q(q);                                                                                 \
        if (q->bank.st == to_stream(s)) return YAGI_OK;                                             \
        YG_HIP(hipStreamSynchronize(q->bank.st));                                                   \
        q->bank.st = to_stream(s);                                                                  \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_reset(yagi_hip_firinterp_##K q) try {                              \
        CHECK_Q(q);                                                                                 \
        return q->bank.w.reset(q->bank.st);                                                         \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_get_interp_rate(yagi_hip_firinterp_##K q, size_t *interp) try {    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(interp);                                                                          \
        *interp = (size_t)q->interp;                                                                \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_get_sub_len(yagi_hip_firinterp_##K q, size_t *hs) try {            \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(hs);                                                                              \
        *hs = (size_t)q->hs;                                                                        \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_set_scale(yagi_hip_firinterp_##K q, C scale) try {                 \
        CHECK_Q(q);                                                                                 \
        q->bank.scale = scale;                                                                      \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_get_scale(yagi_hip_firinterp_##K q, C *scale) try {                \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(scale);                                                                           \
        *scale = q->bank.scale;                                                                     \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_execute(yagi_hip_firinterp_##K q, T x, T *y, size_t ny) try {      \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(y);                                                                               \
        if (ny < (size_t)q->interp) return fail(YAGI_ERR_CONFIG, "output must hold interp samples");\
        return q->block_host(&x, 1, y);                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_execute_block(yagi_hip_firinterp_##K q, const T *x, size_t nx,     \
                                               T *y, size_t ny) try {                               \
        CHECK_Q(q);                                                                                 \
        if (nx == 0) return YAGI_OK;                                                                \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        if (ny < nx * (size_t)q->interp)                                                            \
            return fail(YAGI_ERR_CONFIG, "output must hold n*interp samples");                      \
        return q->block_host(x, nx, y);                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_execute_block_dev(yagi_hip_firinterp_##K q, const T *x, size_t n,  \
                                                   T *y) try {                                      \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        CHECK_NOALIAS(x, n, y, n * (size_t)q->bank.nf);                                             \
        return q->block_dev(x, n, y);                                                               \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_firinterp_##K##_flush(yagi_hip_firinterp_##K q, T *y, size_t ny) try {             \
        T zero{};                                                                                   \
        return yagi_hip_firinterp_##K##_execute(q, zero, y, ny);                                    \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_FIRINTERP_IMPL(rrrf, RRRF, float, float)
YAGI_FIRINTERP_IMPL(crcf, CRCF, yagi_cf32, float)
YAGI_FIRINTERP_IMPL(cccf, CCCF, yagi_cf32, yagi_cf32)

// ---- Rresamp (src/filter/resampler/rresamp.rs) ----------------------------------------------------------
namespace yagi {

static size_t gcd_sz(size_t a, size_t b) {
    while (b) { const size_t t = a % b; a = b; b = t; }
    return a;
}

template <class K>
struct RresampObj {
    using T = typename K::T;
    using C = typename K::C;
    FirPfb<K> bank;                      // P branches of 2m taps (rresamp.rs:40)
    int P = 0, Q = 0, m = 0, block_len = 1;

    int init(size_t interp, size_t decim, size_t m_, const C *h, size_t h_len) {      // :28-57
        if (interp == 0) return fail(YAGI_ERR_CONFIG, "interpolation rate must be greater than zero");
        if (decim == 0) return fail(YAGI_ERR_CONFIG, "decimation rate must be greater than zero");
        if (m_ == 0) return fail(YAGI_ERR_CONFIG, "filter semi-length must be greater than zero");
        if (interp > (size_t)1 << 15 || decim > (size_t)1 << 15 || m_ > (size_t)1 << 15)
            return fail(YAGI_ERR_CONFIG, "rresamp: rate or filter too large");
        if (h_len < 2 * interp * m_) return fail(YAGI_ERR_CONFIG, "rresamp: need 2*interp*m filter coefficients");
        YG_TRY(bank.init(interp, h, 2 * interp * m_));
        P = (int)interp; Q = (int)decim; m = (int)m_;
        block_len = 1;
        return YAGI_OK;
    }
    // nblocks primitive blocks: nblocks*Q inputs -> nblocks*P outputs (device pointers); :162-183
    int blocks_dev(const T *x, size_t nblocks, T *y) {
        YG_TRY(bank.w.ensure_dev(bank.st));
        if (nblocks == 0) return YAGI_OK;
        YG_TRY((launch_rresamp<K>(bank.w.dev(), x, bank.taps.template as<C>(), P, Q, bank.Ls, bank.scale, y,
                                  nblocks, bank.st, bank.w.next())));
        bank.w.flip();                              // the kernel's last workgroup wrote the next window
        return YAGI_OK;
    }
    int blocks_host(const T *x, size_t nblocks, T *y) {
        if (nblocks == 0) return YAGI_OK;
        return bank.ws.run(bank.st, x, nblocks * (size_t)Q, y, nblocks * (size_t)P,
                           [&](const T *xd, T *yd) { return blocks_dev(xd, nblocks, yd); });
    }
};

}  // namespace yagi

#define YAGI_RRESAMP_IMPL(K, KT, T, C)                                                              \
    struct yagi_hip_rresamp_##K##_s : RresampObj<KT> {};                                            \
    extern "C" {                                                                                    \
    int yagi_hip_rresamp_##K##_create(size_t interp, size_t decim, size_t m, const C *h,            \
                                      size_t h_len, yagi_hip_rresamp_##K *q) try {                  \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (h_len && !h) return fail(YAGI_ERR_CONFIG, "null pointer argument");                     \
        auto o = std::make_unique<yagi_hip_rresamp_##K##_s>();                                      \
        YG_TRY(o->init(interp, decim, m, h, h_len));                                                \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_rresamp_##K##_create_kaiser(size_t interp, size_t decim, size_t m, float bw,       \
                                             float as_, yagi_hip_rresamp_##K *q) try {              \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (interp == 0 || decim == 0) return fail(YAGI_ERR_CONFIG, "gcd: arguments must be greater than zero"); \
        const size_t g = gcd_sz(interp, decim);                          /* rresamp.rs:60-62 */     \
        interp /= g;                                                                                \
        decim /= g;                                                                                 \
        if (bw < 0.0f) bw = interp > decim ? 0.5f : 0.5f * (float)interp / (float)decim;            \
        else if (bw > 0.5f) return fail(YAGI_ERR_CONFIG, "invalid bandwidth (%g), must be less than 0.5", (double)bw); \
        if (m == 0) return fail(YAGI_ERR_CONFIG, "filter semi-length must be greater than zero");   \
        std::vector<float> hf;                                                                      \
        YG_TRY(design_kaiser(2 * interp * m + 1, bw / (float)interp, as_, 0.0f, hf));               \
        std::vector<C> hc(hf.size());                                                               \
        for (size_t i = 0; i < hf.size(); ++i) hc[i] = to_c(hf[i], (C *)nullptr);                   \
        YG_TRY(yagi_hip_rresamp_##K##_create(interp, decim, m, hc.data(), hc.size(), q));           \
        (*q)->bank.scale = to_c(2.0f * bw * std::sqrt((float)decim / (float)interp), (C *)nullptr); \
        (*q)->block_len = (int)g;                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_rresamp_##K##_create_default(size_t interp, size_t decim, yagi_hip_rresamp_##K *q) try { \
        return yagi_hip_rresamp_##K##_create_kaiser(interp, decim, 12, 0.5f, 60.0f, q);  /* :99-104 */ \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_rresamp_##K##_destroy(yagi_hip_rresamp_##K q) try {                                \
        delete q;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_rresamp_##K##_clone(yagi_hip_rresamp_##K q, yagi_hip_rresamp_##K *out) try {  /* derive(Clone) rresamp.rs:8 */ \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        YG_TRY(q->bank.w.ensure_dev(q->bank.st));                                                        \
        auto o = std::make_unique<yagi_hip_rresamp_##K##_s>();                                      \
        o->bank.st = q->bank.st;                                                                    \
        o->bank.nf = q->bank.nf;                                                                    \
        o->bank.Ls = q->bank.Ls;                                                                    \
        o->bank.hb = q->bank.hb;                                                                    \
        o->bank.scale = q->bank.scale;                                                              \
        YG_TRY(fill(o->bank.taps, o->bank.hb.data(), o->bank.hb.size() * sizeof(C), o->bank.st));   \
        YG_TRY(o->bank.w.clone_from(q->bank.w, q->bank.st));                                        \
        o->P = q->P; o->Q = q->Q; o->m = q->m; o->block_len = q->block_len;                         \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_rresamp_##K##_set_stream(yagi_hip_rresamp_##K q, yagi_stream_t s) try {            \
        CHECK_Q(q);                                                                                 \
        if (q->bank.st == to_stream(s)) return YAGI_OK;                                             \
        YG_HIP(hipStreamSynchronize(q->bank.st));                                                   \
        q->bank.st = to_stream(s);                                                                  \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_rresamp_##K##_reset(yagi_hip_rresamp_##K q) try {                                  \
        CHECK_Q(q);                                                                                 \
        return q->bank.w.reset(q->bank.st);                                                         \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_rresamp_##K##_set_scale(yagi_hip_rresamp_##K q, C scale) try {                     \
        CHECK_Q(q);                                                                                 \
        q->bank.scale = scale;                                                                      \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_rresamp_##K##_get_scale(yagi_hip_rresamp_##K q, C *scale) try {                    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(scale);                                                                           \
        *scale = q->bank.scale;                                                                     \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_rresamp_##K##_get_params(yagi_hip_rresamp_##K q, size_t *interp, size_t *decim,    \
                                          size_t *m, size_t *block_len) try {                       \
        CHECK_Q(q);                                                                                 \
        if (interp) *interp = (size_t)q->P;                                                         \
        if (decim) *decim = (size_t)q->Q;                                                           \
        if (m) *m = (size_t)q->m;                                                                   \
        if (block_len) *block_len = (size_t)q->block_len;                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_rresamp_##K##_write(yagi_hip_rresamp_##K q, const T *x, size_t n) try {            \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        YG_TRY(q->bank.w.ensure_host(q->bank.st));                                                  \
        for (size_t i = 0; i < n; ++i) q->bank.w.push(x[i]);                                        \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_rresamp_##K##_execute(yagi_hip_rresamp_##K q, const T *x, size_t nx, T *y,         \
                                       size_t ny) try {                                             \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        const size_t bl = (size_t)q->block_len;                                                     \
        if (nx < bl * (size_t)q->Q) return fail(YAGI_ERR_RANGE, "input must hold Q*block_len samples"); \
        if (ny < bl * (size_t)q->P) return fail(YAGI_ERR_RANGE, "output must hold P*block_len samples"); \
        return q->blocks_host(x, bl, y);                                                            \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_rresamp_##K##_execute_block(yagi_hip_rresamp_##K q, const T *x, size_t nx,         \
                                             size_t n, T *y, size_t ny) try {                       \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        const size_t nb = n * (size_t)q->block_len;                                                 \
        if (nx < nb * (size_t)q->Q) return fail(YAGI_ERR_RANGE, "input must hold n*Q*block_len samples"); \
        if (ny < nb * (size_t)q->P) return fail(YAGI_ERR_RANGE, "output must hold n*P*block_len samples"); \
        return q->blocks_host(x, nb, y);                                                            \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_rresamp_##K##_execute_block_dev(yagi_hip_rresamp_##K q, const T *x, size_t n,      \
                                                 T *y) try {                                        \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        CHECK_NOALIAS(x, n * (size_t)q->block_len * (size_t)q->Q, y, n * (size_t)q->block_len * (size_t)q->P); \
        return q->blocks_dev(x, n * (size_t)q->block_len, y);                                       \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_RRESAMP_IMPL(rrrf, RRRF, float, float)
YAGI_RRESAMP_IMPL(crcf, CRCF, yagi_cf32, float)
YAGI_RRESAMP_IMPL(cccf, CCCF, yagi_cf32, yagi_cf32)

// ---- Spgram (src/fft/spgram.rs) -----------------------------------------------------------------------
namespace yagi {

template <class T>
struct SpgramObj {
    hipStream_t st = nullptr;
    int nfft = 0, wtype = 0, wlen = 0, delay = 0;
    float alpha = 1.0f, gamma = 1.0f;
    bool accumulate = true;
    DevWindow<T> buf;
    DevBuf w, psd, out, tbuf, fbuf, part;
    FftPlan plan;
    Staging ws;
    std::vector<T> queue;                // samples push()ed since the last flush
    size_t sample_timer = 0;
    uint64_t num_samples = 0, num_samples_total = 0, num_transforms = 0, num_transforms_total = 0;
    float frequency = 0.0f, sample_rate = -1.0f;

    int init(size_t nfft_, int wtype_, size_t wlen_, size_t delay_) {
        if (nfft_ < 2) return fail(YAGI_ERR_CONFIG, "fft size must be at least 2");
        if (wlen_ > nfft_) return fail(YAGI_ERR_CONFIG, "window size cannot exceed fft size");
        if (wlen_ == 0) return fail(YAGI_ERR_CONFIG, "window size must be greater than zero");
        if (wtype_ == YAGI_WINDOW_KAISER && wlen_ % 2 != 0)              // spgram.rs:60-62 (sic)
            return fail(YAGI_ERR_CONFIG, "KBD window length must be even");
        if (delay_ == 0) return fail(YAGI_ERR_CONFIG, "delay must be greater than 0");
        if (wtype_ < 1 || wtype_ > 9) return fail(YAGI_ERR_CONFIG, "unknown window type");
        if (nfft_ > ((size_t)1 << 20)) return fail(YAGI_ERR_CONFIG, "fft size %zu not supported (max %d)", nfft_, 1 << 20);
        YG_TRY(require_device());
        nfft = (int)nfft_; wtype = wtype_; wlen = (int)wlen_; delay = (int)delay_;
        // taper (spgram.rs:93-119): window, then normalise to unit energy
        std::vector<float> wv(wlen_);
        float g = 0.0f;
        for (size_t i = 0; i < wlen_; ++i) {
            float arg = 0.0f;
            switch (wtype) {
                case YAGI_WINDOW_KAISER: arg = 10.0f; break;
                case YAGI_WINDOW_KBD: arg = 3.0f; break;
                case YAGI_WINDOW_TRIANGULAR: arg = (float)wlen_; break;
                case YAGI_WINDOW_RCOSTAPER: arg = (float)(wlen_ / 3); break;
                default: break;
            }
            YG_TRY(window_value(wtype, i, wlen_, arg, &wv[i]));
            g += wv[i] * wv[i];
        }
        g = 1.0f / std::sqrt(g);
        for (auto &v : wv) v = g * v;
        YG_TRY(fill(w, wv.data(), wlen_ * sizeof(float), st));
        YG_TRY(psd.alloc(nfft_ * sizeof(float)));
        YG_TRY(out.alloc(nfft_ * sizeof(float)));
        YG_TRY(fft_plan_init(plan, nfft_, YAGI_FFT_FORWARD));
        YG_TRY(buf.init(wlen, st));
        set_alpha_unchecked(-1.0f);
        return reset();
    }
    void set_alpha_unchecked(float a) {
        accumulate = (a == -1.0f);
        if (accumulate) { alpha = 1.0f; gamma = 1.0f; } else { alpha = a; gamma = 1.0f - a; }
    }
    int clear() {                                                    // :135-147
        queue.clear();
        sample_timer = (size_t)delay;
        num_transforms = 0;
        num_samples = 0;
        YG_HIP(hipMemsetAsync(psd.p, 0, (size_t)nfft * sizeof(float), st));
        return YAGI_OK;
    }
    int reset() {                                                    // :150-155
        YG_TRY(clear());
        YG_TRY(buf.reset(st));
        num_samples_total = 0;
        num_transforms_total = 0;
        return YAGI_OK;
    }
    // transforms whose newest sample is X[first + f*delay], f < nframes (X = window ++ x)
    // x_len = samples readable at x (the write() block)
    int run_frames(const T *x, long long first, size_t nframes, size_t x_len = 0) {
        if (spgram_fused_supported(nfft)) {       // fused taper -> FFT -> |X|^2 -> accumulate (spgram_kernels.hip)
            const size_t big = spgram_launch_frames(nfft);      // transforms per launch
            for (size_t f0 = 0; f0 < nframes; f0 += big) {
                const size_t nf = (nframes - f0) < big ? (nframes - f0) : big;
                YG_TRY(part.ensure(spgram_fused_scratch_floats(nfft, nf) * sizeof(float)));
                YG_TRY(launch_spgram_fused<T>(nfft, buf.dev(), x, x_len, w.as<float>(), wlen, first + (long long)f0 * delay, delay, nf,
                                                  alpha, gamma, num_transforms == 0, plan.d.tw, psd.as<float>(),
                                                  part.as<float>(), st));
                num_transforms += nf;
                num_transforms_total += nf;
            }
            return YAGI_OK;
        }
        const size_t chunk = spgram_launch_frames(nfft);        // transforms per batch: 2 x 256 MiB of frames at most
        for (size_t f0 = 0; f0 < nframes; f0 += chunk) {
            const size_t nf = (nframes - f0) < chunk ? (nframes - f0) : chunk;
            YG_TRY(tbuf.ensure(nf * (size_t)nfft * sizeof(cf32)));
            YG_TRY(fbuf.ensure(nf * (size_t)nfft * sizeof(cf32)));
            YG_TRY(launch_spgram_frames<T>(buf.dev(), x, w.as<float>(), wlen, nfft, first + (long long)f0 * delay, delay,
                                           nf, tbuf.as<cf32>(), st));
            YG_TRY(launch_fft_batch(plan.d, tbuf.as<cf32>(), fbuf.as<cf32>(), nf, st));
            YG_TRY(part.ensure(spgram_accum_scratch_floats(nfft, nf) * sizeof(float)));
            YG_TRY(launch_spgram_accum(fbuf.as<cf32>(), nfft, nf, alpha, gamma, num_transforms == 0, psd.as<float>(),
                                       part.as<float>(), st));
            num_transforms += nf;
            num_transforms_total += nf;
        }
        return YAGI_OK;
    }
    int write_dev(const T *x, size_t n) {                            // push() x n, :237-259
        if (n == 0) return YAGI_OK;
        const size_t t = sample_timer;                               // 1..delay pushes until the next transform
        size_t nframes = 0;
        if (n >= t) nframes = (n - t) / (size_t)delay + 1;
        if (nframes) YG_TRY(run_frames(x, (long long)t - 1, nframes, n));
        sample_timer = (n < t) ? t - n : (size_t)delay - (n - t) % (size_t)delay;
        num_samples += n;
        num_samples_total += n;
        return buf.advance(x, n, st);
    }
    int write_host(const T *x, size_t n) {
        if (n == 0) return YAGI_OK;
        YG_TRY(ws.put(st, x, n));
        return write_dev(ws.x.as<T>(), n);
    }
    int flush() {
        if (queue.empty()) return YAGI_OK;
        std::vector<T> q2;
        q2.swap(queue);
        return write_host(q2.data(), q2.size());
    }
    int get(float *o, size_t n, bool db) {                           // :292-316
        if (n < (size_t)nfft) return fail(YAGI_ERR_CONFIG, "psd buffer must hold nfft values");
        YG_TRY(flush());
        const uint64_t nt = num_transforms ? num_transforms : 1;
        const float scale = accumulate ? 1.0f / (float)nt : 0.0f;    // the reference's 0.0 when not accumulating
        YG_TRY(launch_spgram_psd(psd.as<float>(), nfft, scale, db, out.as<float>(), st));
        return download(o, out.p, (size_t)nfft * sizeof(float), st);
    }
};

}  // namespace yagi

#define YAGI_SPGRAM_IMPL(K, T)                                                                      \
    struct yagi_hip_spgram##K##_s : SpgramObj<T> {};                                                \
    extern "C" {                                                                                    \
    int yagi_hip_spgram##K##_create(size_t nfft, int wtype, size_t window_len, size_t delay,        \
                                    yagi_hip_spgram##K *q) try {                                    \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        auto o = std::make_unique<yagi_hip_spgram##K##_s>();                                        \
        YG_TRY(o->init(nfft, wtype, window_len, delay));                                            \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_create_default(size_t nfft, yagi_hip_spgram##K *q) try {               \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (nfft < 2) return fail(YAGI_ERR_CONFIG, "fft size must be at least 2");                  \
        return yagi_hip_spgram##K##_create(nfft, YAGI_WINDOW_KAISER, nfft / 2, nfft / 4, q);        \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_destroy(yagi_hip_spgram##K q) try {                                    \
        delete q;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_set_stream(yagi_hip_spgram##K q, yagi_stream_t s) try {                \
        CHECK_Q(q);                                                                                 \
        if (q->st == to_stream(s)) return YAGI_OK;                                                  \
        YG_HIP(hipStreamSynchronize(q->st));                                                        \
        q->st = to_stream(s);                                                                       \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_clear(yagi_hip_spgram##K q) try {                                      \
        CHECK_Q(q);                                                                                 \
        YG_TRY(q->flush());                                                                         \
        return q->clear();                                                                          \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_reset(yagi_hip_spgram##K q) try {                                      \
        CHECK_Q(q);                                                                                 \
        return q->reset();                                                                          \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_set_alpha(yagi_hip_spgram##K q, float alpha) try {                     \
        CHECK_Q(q);                                                                                 \
        if (alpha != -1.0f && (alpha < 0.0f || alpha > 1.0f))                                       \
            return fail(YAGI_ERR_CONFIG, "alpha must be in {-1,[0,1]}");                            \
        YG_TRY(q->flush());                                                                         \
        q->set_alpha_unchecked(alpha);                                                              \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_get_alpha(yagi_hip_spgram##K q, float *alpha) try {                    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(alpha);                                                                           \
        *alpha = q->alpha;                                                                          \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_set_freq(yagi_hip_spgram##K q, float freq) try {                       \
        CHECK_Q(q);                                                                                 \
        q->frequency = freq;                                                                        \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_set_rate(yagi_hip_spgram##K q, float rate) try {                       \
        CHECK_Q(q);                                                                                 \
        if (rate <= 0.0f) return fail(YAGI_ERR_CONFIG, "sample rate must be greater than zero");    \
        q->sample_rate = rate;                                                                      \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_get_params(yagi_hip_spgram##K q, size_t *nfft, size_t *window_len,     \
                                        size_t *delay, int *wtype) try {                            \
        CHECK_Q(q);                                                                                 \
        if (nfft) *nfft = (size_t)q->nfft;                                                          \
        if (window_len) *window_len = (size_t)q->wlen;                                              \
        if (delay) *delay = (size_t)q->delay;                                                       \
        if (wtype) *wtype = q->wtype;                                                               \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_get_counters(yagi_hip_spgram##K q, uint64_t *ns, uint64_t *nst,        \
                                          uint64_t *nt, uint64_t *ntt) try {                        \
        CHECK_Q(q);                                                                                 \
        YG_TRY(q->flush());                                                                         \
        if (ns) *ns = q->num_samples;                                                               \
        if (nst) *nst = q->num_samples_total;                                                       \
        if (nt) *nt = q->num_transforms;                                                            \
        if (ntt) *ntt = q->num_transforms_total;                                                    \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_push(yagi_hip_spgram##K q, T x) try {                                  \
        CHECK_Q(q);                                                                                 \
        q->queue.push_back(x);                                                                      \
        if (q->queue.size() >= (size_t)1 << 20) return q->flush();                                  \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_write(yagi_hip_spgram##K q, const T *x, size_t n) try {                \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        YG_TRY(q->flush());                                                                         \
        return q->write_host(x, n);                                                                 \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_write_dev(yagi_hip_spgram##K q, const T *x, size_t n) try {            \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        YG_TRY(q->flush());                                                                         \
        return q->write_dev(x, n);                                                                  \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_get_psd_mag(yagi_hip_spgram##K q, float *psd, size_t n) try {          \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(psd);                                                                             \
        return q->get(psd, n, false);                                                               \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_get_psd(yagi_hip_spgram##K q, float *psd, size_t n) try {              \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(psd);                                                                             \
        return q->get(psd, n, true);                                                                \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_spgram##K##_estimate_psd(size_t nfft, const T *x, size_t n, float *psd) try {      \
        CHECK_PTR(psd);                                                                             \
        if (n && !x) return fail(YAGI_ERR_CONFIG, "null pointer argument");                         \
        yagi_hip_spgram##K q = nullptr;                                                             \
        YG_TRY(yagi_hip_spgram##K##_create_default(nfft, &q));                                      \
        std::unique_ptr<yagi_hip_spgram##K##_s> guard(q);                                           \
        YG_TRY(q->write_host(x, n));                                                                \
        if (q->num_transforms == 0) YG_TRY(q->run_frames(nullptr, -1, 1));   /* q.step() :325-327 */ \
        return q->get(psd, nfft, true);                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_SPGRAM_IMPL(cf, yagi_cf32)
YAGI_SPGRAM_IMPL(f, float)

// ---- FftFilt ---------------------------------------------------------------------------------------
namespace yagi {

static cf32 cx_of(float v) { return cf32{v, 0.0f}; }
static cf32 cx_of(cf32 v) { return v; }
static float div_scalar(float s, float d) { return s / d; }
static cf32 div_scalar(cf32 s, float d) { return cf32{s.re / d, s.im / d}; }
static float mul_scalar(float s, float d) { return s * d; }
static cf32 mul_scalar(cf32 s, float d) { return cf32{s.re * d, s.im * d}; }

template <class K>
struct FftFiltObj {
    using T = typename K::T;
    using C = typename K::C;
    hipStream_t st = nullptr;
    std::vector<C> h;
    int n = 0;
    C scale = one_of<C>();          // stored divided by 2n like the reference (fftfilt.rs:95-97)
    FftPlan fwd, bwd;
    DevBuf hfreq;                   // FFT{[h;0]}, 2n points
    PingPong<> w;                   // overlap tail, n points
    DevBuf tbuf, fbuf;              // [nblocks][2n] time / frequency buffers
    Staging ws;
    // h_len <= 2049: the blocks of one call are contiguous in the stream and what FftFilt computes is the
    // stream's linear convolution with h, whatever the block length -- so the call goes to the one-launch
    // overlap-save kernel (4096-point transforms chained in registers) and the carried state is the last h_len
    // input samples instead of the overlap-add tail.  Longer filters keep the reference's five stages.
    bool use_conv = false;
    FirFilt<K> fir;

    int init(const C *hh, size_t h_len, size_t nn) {
        if (h_len == 0) return fail(YAGI_ERR_CONFIG, "filter length must be greater than zero");
        if (nn < h_len - 1) return fail(YAGI_ERR_CONFIG, "block length must be greater than h_len-1 (%zu)", h_len - 1);
        if (nn == 0) return fail(YAGI_ERR_CONFIG, "block length must be greater than zero");
        if (2 * nn > ((size_t)1 << 22)) return fail(YAGI_ERR_CONFIG, "block length %zu not supported (2n <= %d)", nn, 1 << 22);
        YG_TRY(require_device());
        h.assign(hh, hh + h_len);
        n = (int)nn;
        scale = div_scalar(one_of<C>(), 2.0f * (float)n);
        use_conv = h_len <= 2049;
        if (use_conv) {
            fir.st = st;
            YG_TRY(fir.init(hh, h_len));
            fir.kernel_choice = 4;
            return YAGI_OK;
        }
        YG_TRY(fft_plan_init(fwd, 2 * nn, YAGI_FFT_FORWARD));
        YG_TRY(fft_plan_init(bwd, 2 * nn, YAGI_FFT_BACKWARD));
        std::vector<cf32> tb(2 * nn, cf32{0.f, 0.f});
        for (size_t i = 0; i < h_len && i < 2 * nn; ++i) tb[i] = cx_of(h[i]);
        YG_TRY(tbuf.alloc(2 * nn * sizeof(cf32)));
        YG_TRY(hfreq.alloc(2 * nn * sizeof(cf32)));
        YG_TRY(upload(tbuf.p, tb.data(), 2 * nn * sizeof(cf32), st));
        YG_TRY(launch_fft_batch(fwd.d, tbuf.as<cf32>(), hfreq.as<cf32>(), 1, st));
        YG_TRY(w.alloc(nn * sizeof(cf32)));
        scale = div_scalar(one_of<C>(), 2.0f * (float)n);
        return reset();
    }
    int reset() {
        if (use_conv) return fir.w.reset(st);
        YG_HIP(hipMemsetAsync(w.cur(), 0, (size_t)n * sizeof(cf32), st));
        return YAGI_OK;
    }
    int blocks_dev(const T *x, size_t nblocks, T *y) {
        if (nblocks == 0) return YAGI_OK;
        if (use_conv) {
            fir.st = st;
            fir.scale = mul_scalar(scale, 2.0f * (float)n);         // the caller's scale (ours is stored / 2n)
            return fir.block_dev(x, nblocks * (size_t)n, y);
        }
        const size_t n2 = 2 * (size_t)n;
        YG_TRY(tbuf.ensure(nblocks * n2 * sizeof(cf32)));
        YG_TRY(fbuf.ensure(nblocks * n2 * sizeof(cf32)));
        YG_TRY(launch_fftfilt_pad<T>(x, n, nblocks, tbuf.as<cf32>(), st));
        YG_TRY(launch_fft_batch(fwd.d, tbuf.as<cf32>(), fbuf.as<cf32>(), nblocks, st));
        YG_TRY(launch_fftfilt_mul(fbuf.as<cf32>(), hfreq.as<cf32>(), (int)n2, nblocks, st));
        YG_TRY(launch_fft_batch(bwd.d, fbuf.as<cf32>(), tbuf.as<cf32>(), nblocks, st));
        YG_TRY((launch_fftfilt_ola<T, C>(tbuf.as<cf32>(), w.cur<cf32>(), n, nblocks, scale, y,
                                         w.next<cf32>(), st)));
        w.flip();
        return YAGI_OK;
    }
    int blocks_host(const T *x, size_t nblocks, T *y) {
        if (nblocks == 0) return YAGI_OK;
        const size_t len = nblocks * (size_t)n;
        return ws.run(st, x, len, y, len, [&](const T *xd, T *yd) { return blocks_dev(xd, nblocks, yd); });
    }
};

}  // namespace yagi

#define YAGI_FFTFILT_IMPL(K, KT, T, C)                                                              \
    struct yagi_hip_fftfilt_##K##_s : FftFiltObj<KT> {};                                            \
    extern "C" {                                                                                    \
    int yagi_hip_fftfilt_##K##_create(const C *h, size_t h_len, size_t n, yagi_hip_fftfilt_##K *q) try { \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (h_len && !h) return fail(YAGI_ERR_CONFIG, "null pointer argument");                     \
        auto o = std::make_unique<yagi_hip_fftfilt_##K##_s>();                                      \
        YG_TRY(o->init(h, h_len, n));                                                               \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fftfilt_##K##_destroy(yagi_hip_fftfilt_##K q) try {                                \
        delete q;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fftfilt_##K##_clone(yagi_hip_fftfilt_##K q, yagi_hip_fftfilt_##K *out) try {       \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        auto o = std::make_unique<yagi_hip_fftfilt_##K##_s>();                                      \
        o->st = q->st;                                                                              \
        YG_TRY(o->init(q->h.data(), q->h.size(), (size_t)q->n));                                    \
        o->scale = q->scale;                                                                        \
        if (q->use_conv) {                                                                          \
            YG_TRY(q->fir.w.ensure_dev(q->st));                                                          \
            YG_TRY(o->fir.w.clone_from(q->fir.w, q->st));                                           \
        } else {                                                                                    \
            YG_HIP(hipMemcpyAsync(o->w.cur(), q->w.cur(), (size_t)q->n * sizeof(cf32),              \
                                  hipMemcpyDeviceToDevice, q->st));                                 \
        YG_HIP(hipStreamSynchronize(q->st));                                                    \
        }                                                                                           \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fftfilt_##K##_set_stream(yagi_hip_fftfilt_##K q, yagi_stream_t s) try {            \
        CHECK_Q(q);                                                                                 \
        if (q->st == to_stream(s)) return YAGI_OK;                                                  \
        YG_HIP(hipStreamSynchronize(q->st));                                                        \
        q->st = to_stream(s);                                                                       \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fftfilt_##K##_reset(yagi_hip_fftfilt_##K q) try {                                  \
        CHECK_Q(q);                                                                                 \
        return q->reset();                                                                          \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fftfilt_##K##_set_scale(yagi_hip_fftfilt_##K q, C scale) try {                     \
        CHECK_Q(q);                                                                                 \
        q->scale = div_scalar(scale, 2.0f * (float)q->n);                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fftfilt_##K##_get_scale(yagi_hip_fftfilt_##K q, C *scale) try {                    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(scale);                                                                           \
        *scale = mul_scalar(q->scale, 2.0f * (float)q->n);                                          \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fftfilt_##K##_get_length(yagi_hip_fftfilt_##K q, size_t *h_len) try {              \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(h_len);                                                                           \
        *h_len = q->h.size();                                                                       \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fftfilt_##K##_execute(yagi_hip_fftfilt_##K q, const T *x, size_t nx, T *y,         \
                                       size_t ny) try {                                             \
        CHECK_Q(q);                                                                                 \
        if (nx != (size_t)q->n || ny != (size_t)q->n)                                               \
            return fail(YAGI_ERR_CONFIG, "input and output lengths must match filter block size");  \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        return q->blocks_host(x, 1, y);                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fftfilt_##K##_execute_blocks(yagi_hip_fftfilt_##K q, const T *x, size_t nblocks,   \
                                              T *y) try {                                           \
        CHECK_Q(q);                                                                                 \
        if (nblocks == 0) return YAGI_OK;                                                           \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        return q->blocks_host(x, nblocks, y);                                                       \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fftfilt_##K##_execute_blocks_dev(yagi_hip_fftfilt_##K q, const T *x,               \
                                                  size_t nblocks, T *y) try {                       \
        CHECK_Q(q);                                                                                 \
        if (nblocks == 0) return YAGI_OK;                                                           \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        CHECK_NOALIAS(x, nblocks * (size_t)q->n, y, nblocks * (size_t)q->n);                        \
        return q->blocks_dev(x, nblocks, y);                                                        \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_FFTFILT_IMPL(rrrf, RRRF, float, float)
YAGI_FFTFILT_IMPL(crcf, CRCF, yagi_cf32, float)
YAGI_FFTFILT_IMPL(cccf, CCCF, yagi_cf32, yagi_cf32)

// ---- fused firfilt_crcf -> FFT stream ------------------------------------------------------------------
struct yagi_hip_firfft_crcf_s : FirFft {};

extern "C" {

int yagi_hip_firfft_crcf_create(const float *h, size_t h_len, size_t nfft, yagi_hip_firfft_crcf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    if (h_len && !h) return fail(YAGI_ERR_CONFIG, "null pointer argument");
    if (nfft == 0) return fail(YAGI_ERR_CONFIG, "fft length must be greater than zero");
    auto o = std::make_unique<yagi_hip_firfft_crcf_s>();
    YG_TRY(o->fir.init(h, h_len));
    if (o->fir.L > 2049) return fail(YAGI_ERR_CONFIG, "fused stream: filter too long (%zu taps, at most 2049)", h_len);
    o->nfft = nfft;
    if (nfft == 4096) YG_TRY(make_stream_twiddles(o->tw));
    else YG_TRY(fft_plan_init(o->plan, nfft, YAGI_FFT_FORWARD));      // any size the Fft object supports
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firfft_crcf_destroy(yagi_hip_firfft_crcf q) try { delete q; return YAGI_OK; } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firfft_crcf_set_pipeline(yagi_hip_firfft_crcf q, int on) try {
    CHECK_Q(q);
    YG_TRY(q->join());
    if (on) YG_TRY(q->fir.w.pipe.init());
    q->fir.w.pipe.on = on != 0;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firfft_crcf_join(yagi_hip_firfft_crcf q) try {
    CHECK_Q(q);
    return q->join();
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firfft_crcf_set_stream(yagi_hip_firfft_crcf q, yagi_stream_t s) try {
    CHECK_Q(q);
    if (q->fir.st == to_stream(s)) return YAGI_OK;
    YG_TRY(q->join());
    YG_HIP(hipStreamSynchronize(q->fir.st));
    q->fir.st = to_stream(s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firfft_crcf_set_scale(yagi_hip_firfft_crcf q, float scale) try { CHECK_Q(q); q->fir.scale = scale; return YAGI_OK; } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firfft_crcf_reset(yagi_hip_firfft_crcf q) try {
    CHECK_Q(q);
    YG_TRY(q->join());
    return q->fir.w.reset(q->fir.st);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firfft_crcf_set_variant(yagi_hip_firfft_crcf q, int variant) try {
    CHECK_Q(q);
    if (variant < 0 || variant > 4) return fail(YAGI_ERR_CONFIG, "unknown variant %d", variant);
    if (q->nfft != 4096 && variant != 0 && variant != 3)
        return fail(YAGI_ERR_CONFIG, "nfft = %zu runs as overlap-save FIR + batched FFT (variant 3) only", q->nfft);
    if (variant == 3 && q->fir.L > 2049) return fail(YAGI_ERR_CONFIG, "fast convolution needs <= 2049 taps");
    if (variant == 4 && q->fir.L > 257) return fail(YAGI_ERR_CONFIG, "frequency-domain variant needs <= 257 taps");
    if (variant == 2 && !q->fir.Lm) return fail(YAGI_ERR_CONFIG, "MFMA variant needs <= 256 taps");
    if (variant == 1 && q->fir.Lp > kSlideMaxTaps) return fail(YAGI_ERR_CONFIG, "sliding variant needs <= %d taps", kSlideMaxTaps);
    YG_TRY(q->join());
    q->variant = variant;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firfft_crcf_execute_dev(yagi_hip_firfft_crcf q, const yagi_cf32 *x, size_t nframes, yagi_cf32 *spectra) try {
    CHECK_Q(q);
    if (nframes == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(spectra);
    CHECK_NOALIAS(x, nframes * q->nfft, spectra, nframes * q->nfft);
    auto &f = q->fir;
    const bool use_freq = q->nfft == 4096 && (q->variant == 4 || (q->variant == 0 && f.L <= 257));
    const bool piped = use_freq && f.w.can_pipe(nframes * q->nfft) && f.conv_ready && f.hfreq_s_valid &&
                       f.hfreq_s_scale == f.scale;
    if (!piped) YG_TRY(f.w.ensure_dev(f.st));   // joins the lanes: everything below runs on the caller's stream
    // auto (0): fast convolution once the filter is long enough for it to win (measured crossover ~100 taps:
    // the direct kernels cost ~0.65 us per tap and 2^24 samples, the convolution kernel a flat 88 us)
    if (q->nfft != 4096) {     // other frame lengths: overlap-save FIR into a scratch stream, then the batched transform
        YG_TRY(f.prepare_conv());
        const size_t n = nframes * q->nfft;
        YG_TRY(q->scratch.ensure(n * sizeof(cf32)));
        cf32 *ys = q->scratch.as<cf32>();
        YG_TRY(launch_fir_crcf_fftconv(f.w.dev(), x, 0, n, f.hfreq.as<cf32>(), f.scale, f.L, f.twf.as<cf32>(),
                                       f.twb.as<cf32>(), ys, n, f.st));
        YG_TRY(launch_fft_batch(q->plan.d, ys, spectra, nframes, f.st));
        return f.w.advance(x, n, f.st);
    }
    if (piped) {
        // the frequency-domain kernel on the next lane (see StreamPipe); tables and scaled FFT{h} are in place
        const size_t n = nframes * q->nfft;
        hipStream_t lane;
        const cf32 *win;
        YG_TRY(f.w.begin_piped(f.st, &lane, &win));
        YG_TRY(launch_firfft_crcf_4096_freq(win, x, f.hfreq_s.as<cf32>(), f.gfft_s.as<cf32>(), f.L, q->tw.as<cf32>(), spectra,
                                            nullptr, nframes, lane));
        return f.w.finish_piped(x, n);
    }
    if (use_freq) {
        // frequency-domain form (one kernel, 16 B/sample): FFT{h}.FFT{x_f} + FFT{frame-boundary correction}
        YG_TRY(f.prepare_conv());
        if (!f.hfreq_s_valid || f.hfreq_s_scale != f.scale) {
            YG_TRY(f.hfreq_s.ensure(4096 * sizeof(cf32)));
            YG_TRY(launch_scale_cf32_pairs(f.hfreq.as<cf32>(), f.scale, f.hfreq_s.as<cf32>(), 256, 4096, f.st));
            YG_TRY(f.gfft_s.ensure(512 * sizeof(cf32)));
            YG_TRY(launch_scale_cf32_pairs(f.gfft.as<cf32>(), f.scale, f.gfft_s.as<cf32>(), 64, 512, f.st));
            f.hfreq_s_valid = true;
            f.hfreq_s_scale = f.scale;
        }
        YG_TRY(launch_firfft_crcf_4096_freq(f.w.dev(), x, f.hfreq_s.as<cf32>(), f.gfft_s.as<cf32>(), f.L,
                                            q->tw.as<cf32>(), spectra, f.w.next(), nframes, f.st));
        f.w.flip();
        return YAGI_OK;
    }
    const bool use_conv = q->variant == 3 || (q->variant == 0 && f.L <= 2049);
    if (use_conv) {
        // fast-convolution form (two kernels): overlap-save FIR into a scratch stream, then the batched
        // 4096-point FFT over its frames.  32 B/sample of HBM traffic instead of 16.  (Running the two
        // kernels as a chunked two-stream pipeline was measured slower: profiles/r01_notes.md.)
        YG_TRY(f.prepare_conv());
        const size_t n = nframes * q->nfft;
        YG_TRY(q->scratch.ensure(n * sizeof(cf32)));
        FftPlanDev d;
        d.n = 4096;
        d.dir = YAGI_FFT_FORWARD;
        d.tw = q->tw.as<cf32>();
        cf32 *ys = q->scratch.as<cf32>();
        YG_TRY(launch_fir_crcf_fftconv(f.w.dev(), x, 0, n, f.hfreq.as<cf32>(), f.scale, f.L, f.twf.as<cf32>(),
                                       f.twb.as<cf32>(), ys, n, f.st));
        YG_TRY(launch_fft_batch(d, ys, spectra, nframes, f.st));
        return f.w.advance(x, n, f.st);
    }
    YG_TRY(launch_firfft_crcf_4096(f.w.dev(), x, f.taps_pad.as<float>(), f.apack.as<float>(), f.L, f.Lp, f.Lm, f.scale,
                                   q->tw.as<cf32>(), spectra, nframes, q->variant, f.st));
    return f.w.advance(x, nframes * q->nfft, f.st);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firfft_crcf_execute(yagi_hip_firfft_crcf q, const yagi_cf32 *x, size_t nframes, yagi_cf32 *spectra) try {
    CHECK_Q(q);
    if (nframes == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(spectra);
    const size_t n = nframes * q->nfft;
    YG_TRY(q->join());
    return q->ws.run(q->fir.st, x, n, spectra, n, [&](const cf32 *xd, cf32 *yd) {
        YG_TRY(yagi_hip_firfft_crcf_execute_dev(q, xd, nframes, yd));
        return q->join();
    });
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- channelizers ------------------------------------------------------------------------------------
struct yagi_hip_firpfbch_crcf_s : PfbCh {};
struct yagi_hip_firpfbch2_crcf_s : PfbCh2 {};

extern "C" {

int yagi_hip_firpfbch_crcf_create(size_t M, size_t p, const float *h, yagi_hip_firpfbch_crcf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    if (M == 0) return fail(YAGI_ERR_CONFIG, "number of channels must be greater than zero");
    if (p == 0) return fail(YAGI_ERR_CONFIG, "invalid filter size (must be greater than 0)");
    CHECK_PTR(h);
    if (M > 8192 || p > 4096) return fail(YAGI_ERR_CONFIG, "channelizer too large");
    YG_TRY(require_device());
    auto o = std::make_unique<yagi_hip_firpfbch_crcf_s>();
    o->M = (int)M;
    o->p = (int)p;
    YG_TRY(fill(o->h, h, M * p * sizeof(float), nullptr));
    YG_TRY(make_twiddles((int)M, YAGI_FFT_FORWARD, o->tw));
    const size_t hl = (p - 1) * M;
    YG_TRY(o->hist.init((int)(hl ? hl : 1), nullptr));
    YG_TRY(o->syn_hist.init((int)(hl ? hl : 1), nullptr));
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch_crcf_create_kaiser(size_t M, size_t m, float as_, yagi_hip_firpfbch_crcf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    if (M == 0) return fail(YAGI_ERR_CONFIG, "number of channels must be greater than zero");
    if (m == 0) return fail(YAGI_ERR_CONFIG, "invalid filter size (must be greater than 0)");
    std::vector<float> hf;
    YG_TRY(design_kaiser(2 * M * m + 1, 0.5f / (float)M, std::fabs(as_), 0.0f, hf));
    return yagi_hip_firpfbch_crcf_create(M, 2 * m, hf.data(), q);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch_crcf_destroy(yagi_hip_firpfbch_crcf q) try { delete q; return YAGI_OK; } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch_crcf_set_stream(yagi_hip_firpfbch_crcf q, yagi_stream_t s) try {
    CHECK_Q(q);
    if (q->st == to_stream(s)) return YAGI_OK;      // unchanged: no host synchronisation
    YG_HIP(hipStreamSynchronize(q->st));
    q->st = to_stream(s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch_crcf_reset(yagi_hip_firpfbch_crcf q) try {
    CHECK_Q(q);
    YG_TRY(q->hist.reset(q->st));
    return q->syn_hist.reset(q->st);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch_crcf_analyzer_execute_dev(yagi_hip_firpfbch_crcf q, const yagi_cf32 *x, size_t nframes, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (nframes == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    CHECK_NOALIAS(x, nframes * (size_t)q->M, y, nframes * (size_t)q->M);
    // a p == 1 channelizer has no history; the 1-sample placeholder window is never read
    bool written = false;
    cf32 *next = (q->p > 1 && q->hist.len == (int)((q->p - 1) * q->M)) ? q->hist.next() : nullptr;
    YG_TRY(launch_firpfbch(q->hist.dev(), x, q->h.as<float>(), q->M, q->p, q->tw.as<cf32>(), y, nframes, q->st, next, &written));
    if (written) { q->hist.flip(); return YAGI_OK; }         // the kernel's last workgroup wrote the next history
    if (q->p > 1) return q->hist.advance(x, nframes * (size_t)q->M, q->st);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch_crcf_analyzer_execute(yagi_hip_firpfbch_crcf q, const yagi_cf32 *x, size_t nframes, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (nframes == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    const size_t n = nframes * (size_t)q->M;
    return q->ws.run(q->st, x, n, y, n,
                     [&](const cf32 *xd, cf32 *yd) { return yagi_hip_firpfbch_crcf_analyzer_execute_dev(q, xd, nframes, yd); });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_firpfbch_crcf_synthesizer_execute_dev(yagi_hip_firpfbch_crcf q, const yagi_cf32 *x, size_t nframes, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (nframes == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    CHECK_NOALIAS(x, nframes * (size_t)q->M, y, nframes * (size_t)q->M);
    YG_TRY(launch_firpfbch_syn(q->syn_hist.dev(), x, q->h.as<float>(), q->M, q->p, q->tw.as<cf32>(), y, nframes, q->st));
    if (q->p > 1) return q->syn_hist.advance(x, nframes * (size_t)q->M, q->st);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch_crcf_synthesizer_execute(yagi_hip_firpfbch_crcf q, const yagi_cf32 *x, size_t nframes, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (nframes == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    const size_t n = nframes * (size_t)q->M;
    return q->ws.run(q->st, x, n, y, n,
                     [&](const cf32 *xd, cf32 *yd) { return yagi_hip_firpfbch_crcf_synthesizer_execute_dev(q, xd, nframes, yd); });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_firpfbch2_crcf_create(size_t M, size_t m, const float *h, yagi_hip_firpfbch2_crcf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    if (M < 2 || (M & 1)) return fail(YAGI_ERR_CONFIG, "number of channels must be greater than 2 and even");
    if (m < 1) return fail(YAGI_ERR_CONFIG, "filter semi-length must be at least 1");
    CHECK_PTR(h);
    if (M > 8192 || m > 2048) return fail(YAGI_ERR_CONFIG, "channelizer too large");
    YG_TRY(require_device());
    auto o = std::make_unique<yagi_hip_firpfbch2_crcf_s>();
    o->M = (int)M;
    o->m = (int)m;
    const size_t hl = 2 * M * m;
    YG_TRY(fill(o->h, h, hl * sizeof(float), nullptr));
    YG_TRY(make_twiddles((int)M, YAGI_FFT_FORWARD, o->tw));
    YG_TRY(o->hist.init((int)((2 * m - 1) * M + M / 2), nullptr));
    YG_TRY(o->syn_hist.init((int)((4 * m - 1) * M), nullptr));
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch2_crcf_create_kaiser(size_t M, size_t m, float as_, yagi_hip_firpfbch2_crcf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    if (M < 2 || (M & 1)) return fail(YAGI_ERR_CONFIG, "number of channels must be greater than 2 and even");
    if (m < 1) return fail(YAGI_ERR_CONFIG, "filter semi-length must be at least 1");
    std::vector<float> hf;
    YG_TRY(design_kaiser(2 * M * m + 1, 1.0f / (float)M, std::fabs(as_), 0.0f, hf));
    float hsum = 0.0f;                          // normalise to unit channel gain: sum(h) = M
    for (float v : hf) hsum += v;
    for (float &v : hf) v = v * (float)M / hsum;
    return yagi_hip_firpfbch2_crcf_create(M, m, hf.data(), q);
} catch (...) { return ::yagi::api_exception(); }
// prototype of the matching synthesizer: kaiser(2Mm+1, 0.5/M, as), scaled to sum M (analyzer: cutoff 1/M)
int yagi_hip_firpfbch2_crcf_create_kaiser_synthesizer(size_t M, size_t m, float as_, yagi_hip_firpfbch2_crcf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    if (M < 2 || (M & 1)) return fail(YAGI_ERR_CONFIG, "number of channels must be greater than 2 and even");
    if (m < 1) return fail(YAGI_ERR_CONFIG, "filter semi-length must be at least 1");
    std::vector<float> hf;
    YG_TRY(design_kaiser(2 * M * m + 1, 0.5f / (float)M, std::fabs(as_), 0.0f, hf));
    float hsum = 0.0f;
    for (float v : hf) hsum += v;
    for (float &v : hf) v = v * (float)M / hsum;
    return yagi_hip_firpfbch2_crcf_create(M, m, hf.data(), q);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch2_crcf_destroy(yagi_hip_firpfbch2_crcf q) try { delete q; return YAGI_OK; } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch2_crcf_set_stream(yagi_hip_firpfbch2_crcf q, yagi_stream_t s) try {
    CHECK_Q(q);
    if (q->st == to_stream(s)) return YAGI_OK;      // unchanged: no host synchronisation
    YG_HIP(hipStreamSynchronize(q->st));
    q->st = to_stream(s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch2_crcf_reset(yagi_hip_firpfbch2_crcf q) try {
    CHECK_Q(q);
    q->step = 0;
    q->syn_step = 0;
    YG_TRY(q->hist.reset(q->st));
    return q->syn_hist.reset(q->st);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch2_crcf_synthesizer_execute_dev(yagi_hip_firpfbch2_crcf q, const yagi_cf32 *x, size_t nsteps, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (nsteps == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    CHECK_NOALIAS(x, nsteps * (size_t)q->M, y, nsteps * (size_t)(q->M / 2));
    YG_TRY(launch_firpfbch2_syn(q->syn_hist.dev(), q->syn_hist.len, x, q->h.as<float>(), q->M, q->m, q->tw.as<cf32>(),
                                q->syn_step, y, nsteps, q->st));
    q->syn_step += nsteps;
    return q->syn_hist.advance(x, nsteps * (size_t)q->M, q->st);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch2_crcf_synthesizer_execute(yagi_hip_firpfbch2_crcf q, const yagi_cf32 *x, size_t nsteps, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (nsteps == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    const size_t nin = nsteps * (size_t)q->M;
    return q->ws.run(q->st, x, nin, y, nin / 2, [&](const cf32 *xd, cf32 *yd) {
        return yagi_hip_firpfbch2_crcf_synthesizer_execute_dev(q, xd, nsteps, yd);
    });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch2_crcf_analyzer_execute_shard_dev(yagi_hip_firpfbch2_crcf q, const yagi_cf32 *x, size_t nsteps,
                                                       int rank, int nranks, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (nsteps == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    if (nranks > 0) CHECK_NOALIAS(x, nsteps * (size_t)(q->M / 2), y, nsteps * (size_t)(q->M / nranks));
    bool written = false;
    YG_TRY(launch_firpfbch2(q->hist.dev(), q->hist.len, x, q->h.as<float>(), q->M, q->m, q->tw.as<cf32>(),
                            q->step, rank, nranks, y, nsteps, q->st, q->hist.next(), &written));
    q->step += nsteps;
    if (written) { q->hist.flip(); return YAGI_OK; }         // the kernel's last workgroup wrote the next history
    return q->hist.advance(x, nsteps * (size_t)(q->M / 2), q->st);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch2_crcf_analyzer_execute_dev(yagi_hip_firpfbch2_crcf q, const yagi_cf32 *x, size_t nsteps, yagi_cf32 *y) try {
    return yagi_hip_firpfbch2_crcf_analyzer_execute_shard_dev(q, x, nsteps, 0, 1, y);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch2_crcf_analyzer_execute(yagi_hip_firpfbch2_crcf q, const yagi_cf32 *x, size_t nsteps, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (nsteps == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    return q->ws.run(q->st, x, nsteps * (size_t)(q->M / 2), y, nsteps * (size_t)q->M, [&](const cf32 *xd, cf32 *yd) {
        return yagi_hip_firpfbch2_crcf_analyzer_execute_dev(q, xd, nsteps, yd);
    });
} catch (...) { return ::yagi::api_exception(); }
// sub-bands sharded over the ranks of `comm`: shard kernel (this stream) -> RCCL all-gather -> assemble (the
// communicator's stream), chunk by chunk so chunk k's exchange runs beside chunk k+1's kernel
int yagi_hip_firpfbch2_crcf_analyzer_execute_sharded_dev(yagi_hip_firpfbch2_crcf q, const yagi_cf32 *x, size_t nsteps,
                                                         yagi_hip_comm comm, int nchunks, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (!comm) return fail(YAGI_ERR_CONFIG, "null communicator");
    if (nsteps == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    CHECK_NOALIAS(x, nsteps * (size_t)(q->M / 2), y, nsteps * (size_t)q->M);
    const int R = comm->nranks, rank = comm->rank;
    if (R == 1 && nchunks >= 0) return yagi_hip_firpfbch2_crcf_analyzer_execute_dev(q, x, nsteps, y);
    if (q->M % R) return fail(YAGI_ERR_CONFIG, "firpfbch2: %d channels do not shard over %d ranks", q->M, R);
    const size_t M = (size_t)q->M, Mr = M / (size_t)R, M2 = M / 2;
    // chunks: even step counts (the column kernels start on an even step), at least 2048 steps each
    size_t nc = nchunks ? (size_t)(nchunks < 0 ? -nchunks : nchunks) : 8;
    while (nc > 1 && nsteps / nc < 2048) --nc;
    size_t per = (nsteps + nc - 1) / nc;
    per += per & 1;
    YG_TRY(q->shard.ensure(nsteps * Mr * sizeof(cf32)));
    YG_TRY(q->gathered.ensure(nsteps * M * sizeof(cf32)));
    while (comm->ev.size() < nc) {
        hipEvent_t e;
        YG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        comm->ev.push_back(e);
    }
    // the exchange stream must not run ahead of work already queued on the object's stream that still reads y
    auto chunks = [&]() -> int {
        size_t done = 0, k = 0;
        while (done < nsteps) {
            const size_t ns = std::min(per, nsteps - done);
            cf32 *sh = q->shard.as<cf32>() + done * Mr;
            cf32 *ga = q->gathered.as<cf32>() + done * M;
            YG_TRY(yagi_hip_firpfbch2_crcf_analyzer_execute_shard_dev(q, x + done * M2, ns, rank, R, sh));
            YG_HIP(hipEventRecord(comm->ev[k], q->st));
            YG_HIP(hipStreamWaitEvent(comm->st, comm->ev[k], 0));
            YG_TRY(comm_all_gather(comm, sh, ga, ns * Mr * sizeof(cf32), comm->st));
            YG_TRY(launch_firpfbch2_assemble(ga, ns, (int)M, R, y + done * M, comm->st));
            done += ns;
            ++k;
        }
        return YAGI_OK;
    };
    const int rc = chunks();
    // success or not: the object's stream waits for whatever the exchange stream was handed, so a later call cannot
    // rewrite (or ensure() free) q->shard / q->gathered while a gather or an assemble still reads them
    if (hipEventRecord(comm->done, comm->st) != hipSuccess || hipStreamWaitEvent(q->st, comm->done, 0) != hipSuccess) {
        (void)hipStreamSynchronize(comm->st);
        if (rc == YAGI_OK) return fail(YAGI_ERR_DEVICE, "joining the exchange stream failed");
    }
    return rc;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbch2_crcf_assemble_dev(const yagi_cf32 *gathered, size_t nsteps, size_t M, int nranks,
                                         yagi_cf32 *y, yagi_stream_t s) try {
    if (nsteps == 0) return YAGI_OK;
    CHECK_PTR(gathered);
    CHECK_PTR(y);
    return launch_firpfbch2_assemble(gathered, nsteps, (int)M, nranks, y, to_stream(s));
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- firpfbchr: M channels, P inputs per analyzer step (chanr_kernels.hip) -----------------------------
struct yagi_hip_firpfbchr_crcf_s : PfbChr {};

// argument errors first, before the device is required
static int firpfbchr_check_args(size_t M, size_t P, size_t m) {
    if (M < 2) return fail(YAGI_ERR_CONFIG, "number of channels must be at least 2");
    if (P < 1 || P > M) return fail(YAGI_ERR_CONFIG, "decimation rate must be in [1, M]");
    if (m < 1) return fail(YAGI_ERR_CONFIG, "filter semi-length must be at least 1");
    if (M > 8192 || m > 2048) return fail(YAGI_ERR_CONFIG, "channelizer too large");
    return firpfbchr_check_shape((int)M, (int)P, (int)m);
}

extern "C" {

int yagi_hip_firpfbchr_crcf_create(size_t M, size_t P, size_t m, const float *h, yagi_hip_firpfbchr_crcf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    YG_TRY(firpfbchr_check_args(M, P, m));
    CHECK_PTR(h);
    YG_TRY(require_device());
    auto o = std::make_unique<yagi_hip_firpfbchr_crcf_s>();
    o->M = (int)M;
    o->P = (int)P;
    o->m = (int)m;
    const size_t hl = 2 * M * m;
    YG_TRY(fill(o->h, h, hl * sizeof(float), nullptr));
    YG_TRY(make_twiddles((int)M, YAGI_FFT_FORWARD, o->tw));
    YG_TRY(o->hist.init((int)(hl - P), nullptr));
    o->syn_rows = (int)((hl + P - 1) / P - 1);                 // the history itself: prepare_synthesizer()
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
static int firpfbchr_create_designed(size_t M, size_t P, size_t m, float fc, float as_, yagi_hip_firpfbchr_crcf *q) {
    CHECK_PTR(q);
    *q = nullptr;
    YG_TRY(firpfbchr_check_args(M, P, m));
    std::vector<float> hf;
    YG_TRY(design_kaiser(2 * M * m + 1, fc, std::fabs(as_), 0.0f, hf));
    float hsum = 0.0f;                          // unit channel gain: sum(h) = M
    for (float v : hf) hsum += v;
    for (float &v : hf) v = v * (float)M / hsum;
    return yagi_hip_firpfbchr_crcf_create(M, P, m, hf.data(), q);
}
// analyzer prototype kaiser(2Mm+1, 0.5/P, as): the channel keeps the whole band its output rate can carry
int yagi_hip_firpfbchr_crcf_create_kaiser(size_t M, size_t P, size_t m, float as_, yagi_hip_firpfbchr_crcf *q) try {
    return firpfbchr_create_designed(M, P, m, 0.5f / (float)(P ? P : 1), as_, q);
} catch (...) { return ::yagi::api_exception(); }
// prototype of the matching synthesizer: kaiser(2Mm+1, 0.5/M, as)
int yagi_hip_firpfbchr_crcf_create_kaiser_synthesizer(size_t M, size_t P, size_t m, float as_, yagi_hip_firpfbchr_crcf *q) try {
    return firpfbchr_create_designed(M, P, m, 0.5f / (float)(M ? M : 1), as_, q);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbchr_crcf_destroy(yagi_hip_firpfbchr_crcf q) try { delete q; return YAGI_OK; } catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbchr_crcf_set_stream(yagi_hip_firpfbchr_crcf q, yagi_stream_t s) try {
    CHECK_Q(q);
    if (q->st == to_stream(s)) return YAGI_OK;      // unchanged: no host synchronisation
    YG_HIP(hipStreamSynchronize(q->st));
    q->st = to_stream(s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbchr_crcf_reset(yagi_hip_firpfbchr_crcf q) try {
    CHECK_Q(q);
    q->step = 0;
    q->syn_step = 0;
    YG_TRY(q->hist.reset(q->st));
    return q->syn_ready ? q->syn_hist.reset(q->st) : YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbchr_crcf_set_kernel(yagi_hip_firpfbchr_crcf q, int choice) try {
    CHECK_Q(q);
    if (choice < 0 || choice > 2) return fail(YAGI_ERR_CONFIG, "kernel choice must be 0 (auto), 1 (general) or 2 (column)");
    if (choice == 2 && !firpfbchr_col_served(q->M, q->P, q->m))
        return fail(YAGI_ERR_CONFIG, "firpfbchr: the column kernel serves M in {64,128,256}, P a multiple of M/8, 2m <= 16");
    q->choice = choice;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbchr_crcf_get_last_kernel(yagi_hip_firpfbchr_crcf q, int *k) try {
    CHECK_Q(q);
    CHECK_PTR(k);
    *k = q->last;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbchr_crcf_analyzer_execute_dev(yagi_hip_firpfbchr_crcf q, const yagi_cf32 *x, size_t nsteps, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (nsteps == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    CHECK_NOALIAS(x, nsteps * (size_t)q->P, y, nsteps * (size_t)q->M);
    int ran = 0;
    YG_TRY(launch_firpfbchr(q->hist.dev(), q->hist.len, x, q->h.as<float>(), q->M, q->P, q->m, q->tw.as<cf32>(), q->step, y,
                            nsteps, q->st, q->choice, &ran));
    q->last = ran;
    q->step += nsteps;
    return q->hist.advance(x, nsteps * (size_t)q->P, q->st);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbchr_crcf_analyzer_execute(yagi_hip_firpfbchr_crcf q, const yagi_cf32 *x, size_t nsteps, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (nsteps == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    return q->ws.run(q->st, x, nsteps * (size_t)q->P, y, nsteps * (size_t)q->M, [&](const cf32 *xd, cf32 *yd) {
        return yagi_hip_firpfbchr_crcf_analyzer_execute_dev(q, xd, nsteps, yd);
    });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbchr_crcf_synthesizer_execute_dev(yagi_hip_firpfbchr_crcf q, const yagi_cf32 *x, size_t nsteps, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (nsteps == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    CHECK_NOALIAS(x, nsteps * (size_t)q->M, y, nsteps * (size_t)q->P);
    YG_TRY(q->prepare_synthesizer());
    const size_t nv = nsteps * (size_t)q->M;
    YG_TRY(q->syn_v.ensure(nv * sizeof(cf32)));
    cf32 *v = q->syn_v.as<cf32>();
    YG_TRY(launch_firpfbchr_syn_transform(x, q->M, q->tw.as<cf32>(), v, nsteps, q->st));
    YG_TRY(launch_firpfbchr_syn_combine(q->syn_hist.dev(), q->syn_rows, v, q->h.as<float>(), q->M, q->P, q->m, q->syn_step, y,
                                        nsteps, q->st));
    q->syn_step += nsteps;
    return q->syn_hist.advance(v, nv, q->st);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firpfbchr_crcf_synthesizer_execute(yagi_hip_firpfbchr_crcf q, const yagi_cf32 *x, size_t nsteps, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (nsteps == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    return q->ws.run(q->st, x, nsteps * (size_t)q->M, y, nsteps * (size_t)q->P, [&](const cf32 *xd, cf32 *yd) {
        return yagi_hip_firpfbchr_crcf_synthesizer_execute_dev(q, xd, nsteps, yd);
    });
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"


// ---- Resamp2 / MsResamp2 (src/filter/resampler/resamp2.rs, msresamp2.rs) ---------------
namespace yagi {

// Resamp2Coeff::for_halfband (resamp2.rs:9-23), f32 arithmetic as the reference spells it
static float for_halfband(float hf, float t, float f0, float *) {
    const float pi = 3.14159265358979323846f;
    return 2.0f * hf * std::cos(2.0f * pi * t * f0);
}
static cf32 for_halfband(float hf, float t, float f0, cf32 *) {
    const float pi = 3.14159265358979323846f;
    const float g = 2.0f * hf, a = 2.0f * pi * t * f0;
    return cf32{g * std::cos(a), g * std::sin(a)};
}

template <class K>
struct Resamp2Obj {
    using T = typename K::T;
    using C = typename K::C;
    hipStream_t st = nullptr;
    int m = 0;
    std::vector<C> h1;             // h1[i] = h[h_len - 2i - 2] (resamp2.rs:66-70)
    DevBuf h1d;
    PingPong<> state;              // [w0 (2m, oldest first)][w1 (2m)]
    int toggle = 0;
    C scale;
    Staging ws;

    // new() from the designed half-band prototype hf[4m+1] (:44-88)
    int init(const float *hf, size_t m_, float f0) {
        if (m_ < 2) return fail(YAGI_ERR_CONFIG, "filter semi-length must be at least 2");
        if (m_ > (size_t)kR2MaxSemiLen) return fail(YAGI_ERR_CONFIG, "filter semi-length must not exceed %d", kR2MaxSemiLen);
        if (f0 < -0.5f || f0 > 0.5f) return fail(YAGI_ERR_CONFIG, "f0 (%g) must be in [-0.5,0.5]", (double)f0);
        m = (int)m_;
        const size_t h_len = 4 * m_ + 1;
        std::vector<C> h(h_len);
        for (size_t i = 0; i < h_len; ++i) {
            const float t = (float)i - (float)(h_len - 1) / 2.0f;
            h[i] = for_halfband(hf[i], t, f0, (C *)nullptr);
        }
        h1.resize(2 * m_);
        for (size_t i = 0; i < 2 * m_; ++i) h1[i] = h[h_len - 2 * i - 2];
        scale = to_c(1.0f, (C *)nullptr);
        YG_TRY(fill(h1d, h1.data(), h1.size() * sizeof(C), st));
        YG_TRY(state.alloc(4 * m_ * sizeof(T)));
        return reset();
    }
    int reset() {                                                   // :90-94
        toggle = 0;
        YG_HIP(hipMemsetAsync(state.cur(), 0, 4 * (size_t)m * sizeof(T), st));
        return YAGI_OK;
    }
    static size_t out_count(int mode, size_t nx) {
        return mode == kR2Filter || mode == kR2Interp ? 2 * nx : mode == kR2Decim ? nx / 2 : nx;
    }
    // the reference's slices carry their lengths (copy_from_slice / indexing panics on a mismatch); the C ABI checks
    static int check_form(int mode, size_t nx) {
        if (mode < kR2Filter || mode > kR2Interp) return fail(YAGI_ERR_CONFIG, "resamp2: unknown form %d", mode);
        if (mode != kR2Filter && mode != kR2Interp && (nx & 1))
            return fail(YAGI_ERR_CONFIG, "resamp2: this form consumes pairs of samples (got %zu)", nx);
        return YAGI_OK;
    }
    static int check_lengths(int mode, size_t nx, size_t ny) {
        YG_TRY(check_form(mode, nx));
        if (ny != out_count(mode, nx))
            return fail(YAGI_ERR_CONFIG, "resamp2: form %d turns %zu samples into %zu, the output holds %zu", mode, nx,
                        out_count(mode, nx), ny);
        return YAGI_OK;
    }
    int block_dev(int mode, const T *x, size_t nx, T *y) {
        YG_TRY(check_form(mode, nx));
        if (nx == 0) return YAGI_OK;
        if (resamp2_takes_chain(mode, m, nx)) {
            // a long decimator block: the one-stage case of the MsResamp2 chain kernels (the same sums in the same order;
            // the middle of the block four outputs per lane through msresamp2_decim_fast_kernel)
            const int mk = m;
            const C sc = scale;
            const C *hp = h1d.template as<C>();
            const T *sp = state.cur<T>();
            T *sn = state.next<T>();
            YG_TRY((launch_msresamp2_decim<T, C>(1, &mk, &sc, &hp, &sp, &sn, x, y, nx / 2, st)));
        } else {
            YG_TRY((launch_resamp2<T, C>(mode, state.cur<T>(), x, nx, h1d.template as<C>(), m, scale, toggle, y,
                                         state.next<T>(), st)));
        }
        state.flip();
        if (mode == kR2Filter) toggle = (toggle + (int)(nx & 1)) & 1;
        return YAGI_OK;
    }
    int block_host(int mode, const T *x, size_t nx, T *y) {
        if (nx == 0) return YAGI_OK;
        // room for one output even where ny == 0 (a one-sample decimator block): the kernel is handed a buffer
        return ws.run(st, x, nx, y, out_count(mode, nx), [&](const T *xd, T *yd) { return block_dev(mode, xd, nx, yd); }, 1);
    }
    int clone_into(Resamp2Obj &o) const {
        o.st = st;
        o.m = m;
        o.h1 = h1;
        o.toggle = toggle;
        o.scale = scale;
        YG_TRY(fill(o.h1d, h1.data(), h1.size() * sizeof(C), st));
        YG_TRY(o.state.alloc(4 * (size_t)m * sizeof(T)));
        YG_HIP(hipMemcpyAsync(o.state.cur(), state.cur(), 4 * (size_t)m * sizeof(T), hipMemcpyDeviceToDevice, st));
        YG_HIP(hipStreamSynchronize(st));
        return YAGI_OK;
    }
};

// estimate_req_filter_len (design/mod.rs:138-152 with Kaiser's formula :228-238) and MsResamp2::new's stage plan
// (msresamp2.rs:66-88): semi-length of every half-band stage
static int msresamp2_stage_lengths(size_t num_stages, float fc, float as_, std::vector<size_t> &m_stage) {
    if (num_stages > 16) return fail(YAGI_ERR_CONFIG, "number of stages should not exceed 16");
    if (fc <= 0.0f || fc >= 0.5f) return fail(YAGI_ERR_CONFIG, "cut-off frequency must be in (0,0.5)");
    m_stage.assign(num_stages, 0);
    const float a = as_ + 5.0f;
    for (size_t i = 0; i < num_stages; ++i) {
        fc = (i == 1) ? (0.5f - fc) / 2.0f : 0.5f * fc;
        const float ft = 2.0f * (0.25f - fc);
        if (ft <= 0.0f || ft > 0.5f) return fail(YAGI_ERR_CONFIG, "cutoff frequency (%g) out of range (0, 0.5)", (double)ft);
        if (a <= 0.0f) return fail(YAGI_ERR_CONFIG, "stopband attenuation must be greater than zero");
        const float hl = (a - 7.95f) / (14.26f * ft);
        const size_t h_len = hl <= 0.0f ? 0 : (size_t)hl;
        const size_t mm = (size_t)std::ceil(((float)h_len - 1.0f) / 4.0f);
        m_stage[i] = mm < 3 ? 3 : mm;
    }
    return YAGI_OK;
}

template <class K>
struct MsResamp2Obj {
    using T = typename K::T;
    using C = typename K::C;
    hipStream_t st = nullptr;
    bool interp = false;
    size_t num_stages = 0, rate = 1;
    std::vector<size_t> m_stage;
    std::vector<std::unique_ptr<Resamp2Obj<K>>> stage;
    DevBuf buf[2];
    Staging ws;

    // n execute() calls: interpolator n -> n * rate, decimator n * rate -> n (msresamp2.rs:137-152, :181 copy_from_slice)
    int check_lengths(size_t nx, size_t ny, size_t *n) const {
        const size_t big = interp ? ny : nx, small = interp ? nx : ny;
        if (big != small * rate)
            return fail(YAGI_ERR_CONFIG, "msresamp2: %s by %zu needs %zu %s samples for %zu %s samples (got %zu)",
                        interp ? "interpolation" : "decimation", rate, small * rate, interp ? "output" : "input", small,
                        interp ? "input" : "output", big);
        *n = small;
        return YAGI_OK;
    }

    int init(bool interp_, size_t ns, const size_t *ms, const float *hf_all) {
        if (ns > 16) return fail(YAGI_ERR_CONFIG, "number of stages should not exceed 16");
        interp = interp_;
        num_stages = ns;
        rate = (size_t)1 << ns;
        m_stage.assign(ms, ms + ns);
        for (size_t i = 0; i < ns; ++i) {
            auto s = std::make_unique<Resamp2Obj<K>>();
            s->st = st;
            YG_TRY(s->init(hf_all, ms[i], 0.0f));                    // f0_stage = 0 (msresamp2.rs:44-46)
            hf_all += 4 * ms[i] + 1;
            stage.push_back(std::move(s));
        }
        // the decimator's zeta = 1/rate multiplies the last stage's output (:197); folded into that stage's scale
        // (its scale is 1, so (y0 + y1) * 1 * zeta == (y0 + y1) * zeta bit for bit)
        if (!interp && ns) stage[0]->scale = to_c(1.0f / (float)rate, (C *)nullptr);
        return YAGI_OK;
    }
    // n execute() calls: interp n -> n*rate, decim n*rate -> n (device pointers)
    int block_dev(const T *x, size_t n, T *y) {
        if (n == 0) return YAGI_OK;
        if (num_stages == 0) {
            YG_HIP(hipMemcpyAsync(y, x, n * sizeof(T), hipMemcpyDeviceToDevice, st));
            return YAGI_OK;
        }
        const size_t big = n * rate;
        if (num_stages > 1) {                                        // ping-pong intermediates: at most big/2 samples
            YG_TRY(buf[0].ensure(big / 2 * sizeof(T)));
            YG_TRY(buf[1].ensure(big / 2 * sizeof(T)));
        }
        const T *src = x;
        int pp = 0;
        if (interp && fused_interp_fits()) {                         // the whole chain in one launch (LDS-resident levels)
            const int ns = (int)num_stages;
            int mk[4];
            C sc[4];
            const C *h1[4];
            const T *sta[4];
            T *stn[4];
            for (int k = 0; k < ns; ++k) {                           // processing order: stage k
                Resamp2Obj<K> &o = *stage[(size_t)k];
                mk[k] = o.m;
                sc[k] = o.scale;
                h1[k] = o.h1d.template as<C>();
                sta[k] = o.state.template cur<T>();
                stn[k] = o.state.template next<T>();
            }
            YG_TRY((launch_msresamp2_interp<T, C>(ns, mk, sc, h1, sta, stn, x, y, n, st)));
            for (size_t g = 0; g < num_stages; ++g) stage[g]->state.flip();
        } else if (interp) {                                         // stage s doubles n 2^s samples (:154-175)
            size_t cnt = n;
            for (size_t s = 0; s < num_stages; ++s) {
                const bool last = s + 1 == num_stages;
                T *dst = last ? y : buf[pp].template as<T>();
                YG_TRY(stage[s]->block_dev(kR2Interp, src, cnt, dst));
                src = dst;
                cnt *= 2;
                pp ^= 1;
            }
        } else if (!interp && fused_decim_fits()) {                  // the whole chain in one launch (LDS-resident intermediates)
            const int ns = (int)num_stages;
            int mk[4];
            C sc[4];
            const C *h1[4];
            const T *sta[4];
            T *stn[4];
            for (int k = 0; k < ns; ++k) {                           // processing order: stage g = S-1-k
                Resamp2Obj<K> &o = *stage[num_stages - 1 - (size_t)k];
                mk[k] = o.m;
                sc[k] = o.scale;
                h1[k] = o.h1d.template as<C>();
                sta[k] = o.state.template cur<T>();
                stn[k] = o.state.template next<T>();
            }
            YG_TRY((launch_msresamp2_decim<T, C>(ns, mk, sc, h1, sta, stn, x, y, n, st)));
            for (size_t g = 0; g < num_stages; ++g) stage[g]->state.flip();
        } else {                                                     // stages g = S-1 .. 0, each halves (:177-197)
            size_t cnt = big;
            for (size_t s = 0; s < num_stages; ++s) {
                const size_t g = num_stages - 1 - s;
                const bool last = g == 0;
                T *dst = last ? y : buf[pp].template as<T>();
                YG_TRY(stage[g]->block_dev(kR2Decim, src, cnt, dst));
                src = dst;
                cnt /= 2;
                pp ^= 1;
            }
        }
        return YAGI_OK;
    }
    // the planners' answer (kernels.hpp): at most four stages whose streams fit 64 KiB of LDS
    bool fused_interp_fits() const {
        if (num_stages > 4) return false;
        int mk[4];
        for (size_t k = 0; k < num_stages && k < 4; ++k) mk[k] = stage[k]->m;
        return msresamp2_interp_plan((int)num_stages, mk, sizeof(T), 1).fused;
    }
    bool fused_decim_fits() const {
        if (num_stages > 4) return false;
        int mk[4];
        for (size_t k = 0; k < num_stages && k < 4; ++k) mk[k] = stage[num_stages - 1 - k]->m;
        return msresamp2_decim_plan((int)num_stages, mk, sizeof(T), 1).fused;
    }
    int block_host(const T *x, size_t n, T *y) {
        if (n == 0) return YAGI_OK;
        const size_t nin = interp ? n : n * rate, nout = interp ? n * rate : n;
        return ws.run(st, x, nin, y, nout, [&](const T *xd, T *yd) { return block_dev(xd, n, yd); });
    }
    float delay() const {                                            // :118-135
        float d = 0.0f;
        if (interp) {
            for (size_t i = 0; i < num_stages; ++i) { d *= 0.5f; d += (float)m_stage[num_stages - i - 1]; }
        } else {
            for (size_t i = 0; i < num_stages; ++i) { d *= 2.0f; d += 2.0f * (float)m_stage[i] - 1.0f; }
        }
        return d;
    }
};

}  // namespace yagi

#define YAGI_RESAMP2_IMPL(K, KT, T, C)                                                              \
    struct yagi_hip_resamp2_##K##_s : Resamp2Obj<KT> {};                                            \
    struct yagi_hip_msresamp2_##K##_s : MsResamp2Obj<KT> {};                                        \
    extern "C" {                                                                                    \
    int yagi_hip_resamp2_##K##_create(const float *hf, size_t m, float f0, yagi_hip_resamp2_##K *q) try { \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        CHECK_PTR(hf);                                                                              \
        auto o = std::make_unique<yagi_hip_resamp2_##K##_s>();                                      \
        YG_TRY(o->init(hf, m, f0));                                                                 \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp2_##K##_create_kaiser(size_t m, float f0, float as_, yagi_hip_resamp2_##K *q) try { \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (m < 2) return fail(YAGI_ERR_CONFIG, "filter semi-length must be at least 2");           \
        if (f0 < -0.5f || f0 > 0.5f) return fail(YAGI_ERR_CONFIG, "f0 (%g) must be in [-0.5,0.5]", (double)f0); \
        if (as_ < 0.0f) return fail(YAGI_ERR_CONFIG, "as (%g) must be greater than zero", (double)as_); \
        if (m > (size_t)kR2MaxSemiLen) return fail(YAGI_ERR_CONFIG, "filter semi-length must not exceed %d", kR2MaxSemiLen); \
        std::vector<float> hf;                                                                      \
        YG_TRY(design_kaiser(4 * m + 1, 0.25f, as_ > 0.0f ? as_ : 1e-3f, 0.0f, hf));                \
        for (float &v : hf) v *= 0.5f;                 /* sinc(t/2) w(t) has centre 1: half-band = centre 1/2 */ \
        return yagi_hip_resamp2_##K##_create(hf.data(), m, f0, q);                                  \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp2_##K##_destroy(yagi_hip_resamp2_##K q) try { delete q; return YAGI_OK; } catch (...) { return ::yagi::api_exception(); } \
    int yagi_hip_resamp2_##K##_clone(yagi_hip_resamp2_##K q, yagi_hip_resamp2_##K *out) try {       \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        auto o = std::make_unique<yagi_hip_resamp2_##K##_s>();                                      \
        YG_TRY(q->clone_into(*o));                                                                  \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp2_##K##_reset(yagi_hip_resamp2_##K q) try { CHECK_Q(q); return q->reset(); } catch (...) { return ::yagi::api_exception(); } \
    int yagi_hip_resamp2_##K##_set_stream(yagi_hip_resamp2_##K q, yagi_stream_t s) try {            \
        CHECK_Q(q);                                                                                 \
        if (q->st == to_stream(s)) return YAGI_OK;                                                  \
        YG_HIP(hipStreamSynchronize(q->st));                                                        \
        q->st = to_stream(s);                                                                       \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp2_##K##_set_scale(yagi_hip_resamp2_##K q, C scale) try { CHECK_Q(q); q->scale = scale; return YAGI_OK; } catch (...) { return ::yagi::api_exception(); } \
    int yagi_hip_resamp2_##K##_get_scale(yagi_hip_resamp2_##K q, C *scale) try {                    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(scale);                                                                           \
        *scale = q->scale;                                                                          \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp2_##K##_get_delay(yagi_hip_resamp2_##K q, size_t *delay) try {               \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(delay);                                                                           \
        *delay = 2 * (size_t)q->m - 1;                                                              \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp2_##K##_execute_block(yagi_hip_resamp2_##K q, int mode, const T *x, size_t nx, T *y, size_t ny) try { \
        CHECK_Q(q);                                                                                 \
        YG_TRY(q->check_lengths(mode, nx, ny));                                                     \
        if (nx == 0) return YAGI_OK;                                                                \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        return q->block_host(mode, x, nx, y);                                                       \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp2_##K##_execute_block_dev(yagi_hip_resamp2_##K q, int mode, const T *x, size_t nx, T *y, size_t ny) try { \
        CHECK_Q(q);                                                                                 \
        YG_TRY(q->check_lengths(mode, nx, ny));                                                     \
        if (nx == 0) return YAGI_OK;                                                                \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        CHECK_NOALIAS(x, nx, y, ny);                                                                \
        return q->block_dev(mode, x, nx, y);                                                        \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp2_##K##_create_taps(int interp, size_t num_stages, const size_t *m_stage,  \
                                             const float *hf_all, yagi_hip_msresamp2_##K *q) try {  \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (num_stages) { CHECK_PTR(m_stage); CHECK_PTR(hf_all); }                                  \
        auto o = std::make_unique<yagi_hip_msresamp2_##K##_s>();                                    \
        YG_TRY(o->init(interp != 0, num_stages, m_stage, hf_all));                                  \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp2_##K##_create(int interp, size_t num_stages, float fc, float f0, float as_, \
                                        yagi_hip_msresamp2_##K *q) try {                            \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        std::vector<size_t> ms;                                                                     \
        YG_TRY(msresamp2_stage_lengths(num_stages, fc, as_, ms));                                   \
        if (f0 != 0.0f) return fail(YAGI_ERR_CONFIG, "non-zero center frequency not yet supported"); \
        std::vector<float> all, hf;                                                                 \
        for (size_t i = 0; i < num_stages; ++i) {                                                   \
            YG_TRY(design_kaiser(4 * ms[i] + 1, 0.25f, as_ + 5.0f, 0.0f, hf));                      \
            for (float &v : hf) v *= 0.5f;                                                          \
            all.insert(all.end(), hf.begin(), hf.end());                                            \
        }                                                                                           \
        return yagi_hip_msresamp2_##K##_create_taps(interp, num_stages, ms.data(), all.data(), q);  \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp2_##K##_destroy(yagi_hip_msresamp2_##K q) try { delete q; return YAGI_OK; } catch (...) { return ::yagi::api_exception(); } \
    int yagi_hip_msresamp2_##K##_clone(yagi_hip_msresamp2_##K q, yagi_hip_msresamp2_##K *out) try { \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        auto o = std::make_unique<yagi_hip_msresamp2_##K##_s>();                                    \
        o->st = q->st;                                                                              \
        o->interp = q->interp;                                                                      \
        o->num_stages = q->num_stages;                                                              \
        o->rate = q->rate;                                                                          \
        o->m_stage = q->m_stage;                                                                    \
        for (auto &s : q->stage) {                                                                  \
            auto c = std::make_unique<Resamp2Obj<KT>>();                                            \
            YG_TRY(s->clone_into(*c));                                                              \
            o->stage.push_back(std::move(c));                                                       \
        }                                                                                           \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp2_##K##_reset(yagi_hip_msresamp2_##K q) try {                              \
        CHECK_Q(q);                                                                                 \
        for (auto &s : q->stage) YG_TRY(s->reset());                                                \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp2_##K##_set_stream(yagi_hip_msresamp2_##K q, yagi_stream_t s) try {        \
        CHECK_Q(q);                                                                                 \
        if (q->st == to_stream(s)) return YAGI_OK;                                                  \
        YG_HIP(hipStreamSynchronize(q->st));                                                        \
        q->st = to_stream(s);                                                                       \
        for (auto &g : q->stage) g->st = q->st;                                                     \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp2_##K##_get_params(yagi_hip_msresamp2_##K q, int *interp, size_t *num_stages, \
                                            float *delay, size_t *m_stage) try {                    \
        CHECK_Q(q);                                                                                 \
        if (interp) *interp = q->interp ? 1 : 0;                                                    \
        if (num_stages) *num_stages = q->num_stages;                                                \
        if (delay) *delay = q->delay();                                                             \
        if (m_stage) for (size_t i = 0; i < q->num_stages; ++i) m_stage[i] = q->m_stage[i];         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp2_##K##_execute_block(yagi_hip_msresamp2_##K q, const T *x, size_t nx, T *y, size_t ny) try { \
        CHECK_Q(q);                                                                                 \
        size_t n = 0;                                                                               \
        YG_TRY(q->check_lengths(nx, ny, &n));                                                       \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        return q->block_host(x, n, y);                                                              \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp2_##K##_execute_block_dev(yagi_hip_msresamp2_##K q, const T *x, size_t nx, T *y, size_t ny) try { \
        CHECK_Q(q);                                                                                 \
        size_t n = 0;                                                                               \
        YG_TRY(q->check_lengths(nx, ny, &n));                                                       \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        CHECK_NOALIAS(x, nx, y, ny);                                                                \
        return q->block_dev(x, n, y);                                                               \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_RESAMP2_IMPL(rrrf, RRRF, float, float)
YAGI_RESAMP2_IMPL(crcf, CRCF, yagi_cf32, float)
YAGI_RESAMP2_IMPL(cccf, CCCF, yagi_cf32, yagi_cf32)

// ---- Resamp (src/filter/resampler/resamp.rs) ------------------------------------------------------------
namespace yagi {

constexpr size_t kResampHostMax = 32;    // execute_block on host data: up to this many inputs on the host mirror

// the kernel stages at least one output's 2m + 1 input samples in its 48 KiB of LDS (fir_kernels.hip: launch_resamp)
template <class T>
static int resamp_check_len(size_t m) {
    if (m > ((size_t)1 << 20) || (2 * m + 1) * sizeof(T) > ((size_t)48 << 10))
        return fail(YAGI_ERR_CONFIG, "resamp: filter semi-length %zu too large for this engine", m);
    return YAGI_OK;
}

template <class K>
struct ResampObj {
    using T = typename K::T;
    using C = typename K::C;
    FirPfb<K> bank;                      // 2^bits branches of 2m taps (resamp.rs:56)
    size_t m = 0;
    int bits = 0;
    float r = 0.0f;
    uint32_t step = 0, phase = 0;        // :12-13, 24 fractional bits

    int set_rate(float rate) {                                                       // :95-106
        if (rate <= 0.0f) return fail(YAGI_ERR_CONFIG, "resampling rate must be greater than zero");
        if (rate < 0.004f || rate > 250.0f) return fail(YAGI_ERR_CONFIG, "resampling rate must be in [0.004,250]");
        r = rate;
        step = (uint32_t)std::round(16777216.0f / r);       // f32 division, half away from zero, as Rust's round()
        return YAGI_OK;
    }
    int init(float rate, size_t m_, size_t npfb, const C *h, size_t h_len) {
        if (m_ == 0) return fail(YAGI_ERR_CONFIG, "filter semi-length must be greater than zero");
        if (npfb < 2 || npfb > ((size_t)1 << 16) || (npfb & (npfb - 1)))
            return fail(YAGI_ERR_CONFIG, "number of filter banks must be a power of two in [2,2^16]");
        YG_TRY(resamp_check_len<T>(m_));
        if (h_len < 2 * m_ * npfb) return fail(YAGI_ERR_CONFIG, "resamp: need 2*m*npfb filter coefficients");
        YG_TRY(bank.init(npfb, h, 2 * m_ * npfb));
        m = m_;
        bits = 0;
        while (((size_t)1 << bits) < npfb) ++bits;
        YG_TRY(set_rate(rate));
        phase = 0;
        return YAGI_OK;
    }
    // closed form of get_num_output (:128-139): A_j = phase + j step < 2^24 nx; *next = the phase after the call
    size_t num_output(size_t nx, uint32_t *next = nullptr) const {
        const unsigned __int128 end = (unsigned __int128)nx << 24;
        size_t n = 0;
        if (end > phase) n = (size_t)((end - phase + step - 1) / step);
        if (next) *next = (uint32_t)((unsigned __int128)phase + (unsigned __int128)n * step - end);
        return n;
    }
    // execute(x) on the host mirror (:141-154): push, then the branch outputs while phase <= 0xFFFFFF
    size_t one_host(T x, T *y) {
        bank.w.push(x);
        size_t n = 0;
        while (phase <= 0x00ffffffu) {
            const uint32_t idx = phase >> (24 - bits);
            y[n++] = host_fir_window_dot<T, C>(bank.w.host(), (size_t)bank.Ls, bank.hb.data() + (size_t)idx * bank.Ls,
                                               bank.scale);
            phase += step;
        }
        phase -= 1u << 24;
        return n;
    }
    int block_host_mirror(const T *x, size_t nx, T *y) {
        YG_TRY(bank.w.ensure_host(bank.st));
        size_t ny = 0;
        for (size_t i = 0; i < nx; ++i) ny += one_host(x[i], y + ny);
        return YAGI_OK;
    }
    // nx inputs on the device -> ny = num_output(nx) outputs; window and phase advanced
    int block_dev(const T *x, size_t nx, T *y, size_t ny) {
        YG_TRY(bank.w.ensure_dev(bank.st));
        if (nx == 0) return YAGI_OK;
        uint32_t next = 0;
        if (num_output(nx, &next) != ny) return fail(YAGI_ERR_INTERNAL, "resamp: output count mismatch");
        if (ny == 0) {
            YG_TRY(bank.w.advance(x, nx, bank.st));
        } else {
            YG_TRY((launch_resamp<K>(bank.w.dev(), x, bank.taps.template as<C>(), bank.Ls, bits, step, phase, y, ny, nx,
                                     bank.st, bank.w.next())));
            bank.w.flip();                          // the kernel's last workgroup wrote the next window
        }
        phase = next;
        return YAGI_OK;
    }
    int block_host(const T *x, size_t nx, T *y, size_t ny) {
        if (nx == 0) return YAGI_OK;
        if (nx <= kResampHostMax) return block_host_mirror(x, nx, y);
        return bank.ws.run(bank.st, x, nx, y, ny, [&](const T *xd, T *yd) { return block_dev(xd, nx, yd, ny); });
    }
    int clone_into(ResampObj &o) {                 // derive(Clone) :8
        YG_TRY(bank.w.ensure_dev(bank.st));
        o.bank.st = bank.st;
        o.bank.nf = bank.nf;
        o.bank.Ls = bank.Ls;
        o.bank.hb = bank.hb;
        o.bank.scale = bank.scale;
        YG_TRY(fill(o.bank.taps, o.bank.hb.data(), o.bank.hb.size() * sizeof(C), o.bank.st));
        YG_TRY(o.bank.w.clone_from(bank.w, bank.st));
        o.m = m; o.bits = bits; o.r = r; o.step = step; o.phase = phase;
        return YAGI_OK;
    }
};

// new(rate, m, fc, as_, npfb) :24-71 up to the bank: checks in the reference's order, Kaiser design of 2 m npfb + 1 taps
// normalised to DC gain npfb (sequential f32 sum, like iter().sum()); *npfb_out = 2^nextpow2(npfb)
template <class T, class C>
static int resamp_design(float rate, size_t m, float fc, float as_, size_t npfb, std::vector<C> &h, size_t *npfb_out) {
    if (rate <= 0.0f) return fail(YAGI_ERR_CONFIG, "resampling rate must be greater than zero");
    if (m == 0) return fail(YAGI_ERR_CONFIG, "filter semi-length must be greater than zero");
    if (fc <= 0.0f || fc >= 0.5f) return fail(YAGI_ERR_CONFIG, "filter cutoff must be in (0,0.5)");
    if (as_ <= 0.0f) return fail(YAGI_ERR_CONFIG, "filter stop-band suppression must be greater than zero");
    if (npfb == 0) return fail(YAGI_ERR_VALUE, "nextpow2(), input must be greater than zero");   // math/mod.rs:80-92
    int bits = 0;
    while (bits < 64 && ((size_t)1 << bits) < npfb) ++bits;
    if (bits < 1 || bits > 16) return fail(YAGI_ERR_CONFIG, "number of filter banks must be in (2^0,2^16)");
    npfb = (size_t)1 << bits;
    YG_TRY(resamp_check_len<T>(m));
    std::vector<float> hf;
    YG_TRY(design_kaiser(2 * m * npfb + 1, fc / (float)npfb, as_, 0.0f, hf));
    float gain = 0.0f;
    for (float v : hf) gain += v;
    gain = (float)npfb / gain;
    h.resize(hf.size());
    for (size_t i = 0; i < hf.size(); ++i) h[i] = to_c(hf[i] * gain, (C *)nullptr);
    *npfb_out = npfb;
    return YAGI_OK;
}

}  // namespace yagi

#define YAGI_RESAMP_IMPL(K, KT, T, C)                                                               \
    struct yagi_hip_resamp_##K##_s : ResampObj<KT> {};                                              \
    extern "C" {                                                                                    \
    int yagi_hip_resamp_##K##_create_taps(float rate, size_t m, size_t npfb, const C *h,            \
                                          size_t h_len, yagi_hip_resamp_##K *q) try {               \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        CHECK_PTR(h);                                                                               \
        auto o = std::make_unique<yagi_hip_resamp_##K##_s>();                                       \
        YG_TRY(o->init(rate, m, npfb, h, h_len));                                                   \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp_##K##_create(float rate, size_t m, float fc, float as_, size_t npfb,        \
                                     yagi_hip_resamp_##K *q) try {                                  \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        std::vector<C> h;                                                                           \
        YG_TRY((resamp_design<T, C>(rate, m, fc, as_, npfb, h, &npfb)));                                 \
        return yagi_hip_resamp_##K##_create_taps(rate, m, npfb, h.data(), h.size(), q);             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp_##K##_create_default(float rate, yagi_hip_resamp_##K *q) try {  /* :73-84 */ \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (rate <= 0.0f) return fail(YAGI_ERR_CONFIG, "resampling rate must be greater than zero"); \
        return yagi_hip_resamp_##K##_create(rate, 7, 0.25f, 60.0f, 256, q);                         \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp_##K##_destroy(yagi_hip_resamp_##K q) try { delete q; return YAGI_OK; } catch (...) { return ::yagi::api_exception(); } \
    int yagi_hip_resamp_##K##_clone(yagi_hip_resamp_##K q, yagi_hip_resamp_##K *out) try {          \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        auto o = std::make_unique<yagi_hip_resamp_##K##_s>();                                       \
        YG_TRY(q->clone_into(*o));                                                                  \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp_##K##_set_stream(yagi_hip_resamp_##K q, yagi_stream_t s) try {              \
        CHECK_Q(q);                                                                                 \
        if (q->bank.st == to_stream(s)) return YAGI_OK;                                             \
        YG_HIP(hipStreamSynchronize(q->bank.st));                                                   \
        q->bank.st = to_stream(s);                                                                  \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp_##K##_reset(yagi_hip_resamp_##K q) try {                  /* :86-89 */      \
        CHECK_Q(q);                                                                                 \
        q->phase = 0;                                                                               \
        return q->bank.w.reset(q->bank.st);                                                         \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp_##K##_set_rate(yagi_hip_resamp_##K q, float rate) try {                     \
        CHECK_Q(q);                                                                                 \
        return q->set_rate(rate);                                                                   \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp_##K##_adjust_rate(yagi_hip_resamp_##K q, float gamma) try { /* :112-118 */  \
        CHECK_Q(q);                                                                                 \
        if (gamma <= 0.0f)                                                                          \
            return fail(YAGI_ERR_CONFIG, "resampling adjustment (%g) must be greater than zero", (double)gamma); \
        return q->set_rate(q->r * gamma);                                                           \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp_##K##_get_rate(yagi_hip_resamp_##K q, float *rate) try {                    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(rate);                                                                            \
        *rate = q->r;                                                                               \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp_##K##_get_delay(yagi_hip_resamp_##K q, size_t *delay) try {                 \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(delay);                                                                           \
        *delay = q->m;                                                                              \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp_##K##_get_num_output(yagi_hip_resamp_##K q, size_t nx, size_t *ny) try {    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(ny);                                                                              \
        *ny = q->num_output(nx);                                                                    \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp_##K##_execute(yagi_hip_resamp_##K q, T x, T *y, size_t ny_cap, size_t *nw) try { \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(nw);                                                                              \
        *nw = 0;                                                                                    \
        const size_t ny = q->num_output(1);                                                         \
        if (ny > ny_cap) return fail(YAGI_ERR_RANGE, "resamp: output holds %zu samples, %zu needed", ny_cap, ny); \
        if (ny) CHECK_PTR(y);                                                                       \
        YG_TRY(q->block_host_mirror(&x, 1, y));                                                     \
        *nw = ny;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp_##K##_execute_block(yagi_hip_resamp_##K q, const T *x, size_t nx, T *y,     \
                                            size_t ny_cap, size_t *nw) try {                        \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(nw);                                                                              \
        *nw = 0;                                                                                    \
        const size_t ny = q->num_output(nx);                                                        \
        if (ny > ny_cap) return fail(YAGI_ERR_RANGE, "resamp: output holds %zu samples, %zu needed", ny_cap, ny); \
        if (nx == 0) return YAGI_OK;                                                                \
        CHECK_PTR(x);                                                                               \
        if (ny) CHECK_PTR(y);                                                                       \
        YG_TRY(q->block_host(x, nx, y, ny));                                                        \
        *nw = ny;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_resamp_##K##_execute_block_dev(yagi_hip_resamp_##K q, const T *x, size_t nx, T *y, \
                                                size_t ny_cap, size_t *nw) try {                    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(nw);                                                                              \
        *nw = 0;                                                                                    \
        const size_t ny = q->num_output(nx);                                                        \
        if (ny > ny_cap) return fail(YAGI_ERR_RANGE, "resamp: output holds %zu samples, %zu needed", ny_cap, ny); \
        if (nx == 0) return YAGI_OK;                                                                \
        CHECK_PTR(x);                                                                               \
        if (ny) {                                                                                   \
            CHECK_PTR(y);                                                                           \
            CHECK_NOALIAS(x, nx, y, ny);                                                            \
        }                                                                                           \
        YG_TRY(q->block_dev(x, nx, y, ny));                                                         \
        *nw = ny;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_RESAMP_IMPL(rrrf, RRRF, float, float)
YAGI_RESAMP_IMPL(crcf, CRCF, yagi_cf32, float)
YAGI_RESAMP_IMPL(cccf, CCCF, yagi_cf32, yagi_cf32)

// ---- MsResamp (src/filter/resampler/msresamp.rs) -------------------------------------------------------
namespace yagi {

// H2 / HR: the C-ABI object types of MsResamp2 and Resamp of the same type combination (made through their create())
template <class K, class H2, class HR>
struct MsResampObj {
    using T = typename K::T;
    using C = typename K::C;
    hipStream_t st = nullptr;
    bool interp = false;
    float rate = 0.0f, rate_arbitrary = 0.0f;
    size_t num_stages = 0;
    std::unique_ptr<H2> half;            // halfband_resamp :18
    std::unique_ptr<HR> arb;             // arbitrary_resamp :19
    DevBuf carry;                        // decimator: the buffer_index (< 2^S) inputs not yet through the half-band chain
    size_t carry_len = 0;
    DevBuf mid;                          // the stream between the two parts
    Staging ws;

    size_t group() const { return (size_t)1 << num_stages; }
    size_t num_output(size_t nx) const {                                             // :109-120
        if (interp) return arb->num_output(nx) << num_stages;
        return arb->num_output((carry_len + nx) >> num_stages);
    }
    float delay() const {                                                            // :87-103
        const float dh = half->delay(), da = (float)arb->m;
        if (num_stages == 0) return da;
        if (interp) return dh / rate_arbitrary + da;
        return dh + (float)group() * da;
    }
    int copy_dev(T *dst, const T *src, size_t n) {
        if (n) YG_HIP(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToDevice, st));
        return YAGI_OK;
    }
    // nx inputs -> ny = num_output(nx) outputs, device pointers
    int exec_dev(const T *x, size_t nx, T *y, size_t ny) {
        if (nx == 0) return YAGI_OK;
        if (num_stages == 0) return arb->block_dev(x, nx, y, ny);
        if (interp) {                                                                // :129-142
            const size_t n1 = arb->num_output(nx);
            YG_TRY(mid.ensure(n1 * sizeof(T)));
            YG_TRY(arb->block_dev(x, nx, mid.template as<T>(), n1));
            return half->block_dev(mid.template as<T>(), n1, y);
        }
        // decimator (:144-168): groups of 2^S inputs through the half-band chain, the first one completing the carry
        const size_t R = group(), total = carry_len + nx, groups = total >> num_stages, left = total & (R - 1);
        T *cb = carry.template as<T>();
        if (groups == 0) {
            YG_TRY(copy_dev(cb + carry_len, x, nx));
            carry_len += nx;
            return YAGI_OK;
        }
        YG_TRY(mid.ensure(groups * sizeof(T)));
        T *mb = mid.template as<T>();
        size_t g = 0, xo = 0;
        if (carry_len) {
            xo = R - carry_len;
            YG_TRY(copy_dev(cb + carry_len, x, xo));
            YG_TRY(half->block_dev(cb, 1, mb));
            g = 1;
        }
        if (groups > g) YG_TRY(half->block_dev(x + xo, groups - g, mb + g));
        YG_TRY(copy_dev(cb, x + (nx - left), left));
        carry_len = left;
        return arb->block_dev(mb, groups, y, ny);
    }
    int exec_host(const T *x, size_t nx, T *y, size_t ny) {
        if (nx == 0) return YAGI_OK;
        return ws.run(st, x, nx, y, ny, [&](const T *xd, T *yd) { return exec_dev(xd, nx, yd, ny); });
    }
};

}  // namespace yagi

#define YAGI_MSRESAMP_IMPL(K, KT, T, C)                                                             \
    struct yagi_hip_msresamp_##K##_s : MsResampObj<KT, yagi_hip_msresamp2_##K##_s, yagi_hip_resamp_##K##_s> {}; \
    extern "C" {                                                                                    \
    int yagi_hip_msresamp_##K##_create(float rate, float as_, yagi_hip_msresamp_##K *q) try {       \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        if (rate <= 0.0f) return fail(YAGI_ERR_CONFIG, "resampling rate must be greater than zero"); \
        auto o = std::make_unique<yagi_hip_msresamp_##K##_s>();                                     \
        o->rate = rate;                                                                             \
        o->interp = rate > 1.0f;                                           /* msresamp.rs:33 */     \
        o->rate_arbitrary = rate;                                                                   \
        if (o->interp) {                                                   /* :38-51 */             \
            while (o->rate_arbitrary > 2.0f) { ++o->num_stages; o->rate_arbitrary *= 0.5f; }        \
        } else {                                                                                    \
            while (o->rate_arbitrary < 0.5f) { ++o->num_stages; o->rate_arbitrary *= 2.0f; }        \
        }                                                                                           \
        yagi_hip_msresamp2_##K h2 = nullptr;                                                        \
        YG_TRY(yagi_hip_msresamp2_##K##_create(o->interp ? 1 : 0, o->num_stages, 0.4f, 0.0f, as_, &h2)); \
        o->half.reset(h2);                                                                          \
        yagi_hip_resamp_##K hr = nullptr;                                                           \
        const float ra = o->rate_arbitrary;                                                         \
        YG_TRY(yagi_hip_resamp_##K##_create(ra, 7, std::min(0.515f * ra, 0.49f), as_, 256, &hr));   \
        o->arb.reset(hr);                                                                           \
        YG_TRY(o->carry.alloc(o->group() * sizeof(T)));                                             \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp_##K##_destroy(yagi_hip_msresamp_##K q) try { delete q; return YAGI_OK; } catch (...) { return ::yagi::api_exception(); } \
    int yagi_hip_msresamp_##K##_clone(yagi_hip_msresamp_##K q, yagi_hip_msresamp_##K *out) try {    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        auto o = std::make_unique<yagi_hip_msresamp_##K##_s>();                                     \
        o->st = q->st;                                                                              \
        o->interp = q->interp;                                                                      \
        o->rate = q->rate;                                                                          \
        o->rate_arbitrary = q->rate_arbitrary;                                                      \
        o->num_stages = q->num_stages;                                                              \
        yagi_hip_msresamp2_##K h2 = nullptr;                                                        \
        YG_TRY(yagi_hip_msresamp2_##K##_clone(q->half.get(), &h2));                                 \
        o->half.reset(h2);                                                                          \
        yagi_hip_resamp_##K hr = nullptr;                                                           \
        YG_TRY(yagi_hip_resamp_##K##_clone(q->arb.get(), &hr));                                     \
        o->arb.reset(hr);                                                                           \
        YG_TRY(o->carry.alloc(o->group() * sizeof(T)));                                             \
        o->carry_len = q->carry_len;                                                                \
        YG_TRY(o->copy_dev(o->carry.template as<T>(), q->carry.template as<T>(), q->carry_len));    \
        YG_HIP(hipStreamSynchronize(o->st));                                                        \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp_##K##_set_stream(yagi_hip_msresamp_##K q, yagi_stream_t s) try {          \
        CHECK_Q(q);                                                                                 \
        if (q->st == to_stream(s)) return YAGI_OK;                                                  \
        YG_HIP(hipStreamSynchronize(q->st));                                                        \
        YG_TRY(yagi_hip_msresamp2_##K##_set_stream(q->half.get(), s));                              \
        YG_TRY(yagi_hip_resamp_##K##_set_stream(q->arb.get(), s));                                  \
        q->st = to_stream(s);                                                                       \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp_##K##_reset(yagi_hip_msresamp_##K q) try {              /* :81-85 */      \
        CHECK_Q(q);                                                                                 \
        YG_TRY(yagi_hip_msresamp2_##K##_reset(q->half.get()));                                      \
        YG_TRY(yagi_hip_resamp_##K##_reset(q->arb.get()));                                          \
        q->carry_len = 0;                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp_##K##_get_rate(yagi_hip_msresamp_##K q, float *rate) try {                \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(rate);                                                                            \
        *rate = q->rate;                                                                            \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp_##K##_get_delay(yagi_hip_msresamp_##K q, float *delay) try {              \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(delay);                                                                           \
        *delay = q->delay();                                                                        \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp_##K##_get_params(yagi_hip_msresamp_##K q, int *interp,                    \
                                           size_t *num_halfband_stages, float *rate_arbitrary) try { \
        CHECK_Q(q);                                                                                 \
        if (interp) *interp = q->interp ? 1 : 0;                                                    \
        if (num_halfband_stages) *num_halfband_stages = q->num_stages;                              \
        if (rate_arbitrary) *rate_arbitrary = q->rate_arbitrary;                                    \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp_##K##_get_num_output(yagi_hip_msresamp_##K q, size_t nx, size_t *ny) try { \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(ny);                                                                              \
        *ny = q->num_output(nx);                                                                    \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp_##K##_execute(yagi_hip_msresamp_##K q, const T *x, size_t nx, T *y,       \
                                        size_t ny_cap, size_t *nw) try {                            \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(nw);                                                                              \
        *nw = 0;                                                                                    \
        const size_t ny = q->num_output(nx);                                                        \
        if (ny > ny_cap) return fail(YAGI_ERR_RANGE, "msresamp: output holds %zu samples, %zu needed", ny_cap, ny); \
        if (nx == 0) return YAGI_OK;                                                                \
        CHECK_PTR(x);                                                                               \
        if (ny) CHECK_PTR(y);                                                                       \
        YG_TRY(q->exec_host(x, nx, y, ny));                                                         \
        *nw = ny;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_msresamp_##K##_execute_dev(yagi_hip_msresamp_##K q, const T *x, size_t nx, T *y,   \
                                            size_t ny_cap, size_t *nw) try {                        \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(nw);                                                                              \
        *nw = 0;                                                                                    \
        const size_t ny = q->num_output(nx);                                                        \
        if (ny > ny_cap) return fail(YAGI_ERR_RANGE, "msresamp: output holds %zu samples, %zu needed", ny_cap, ny); \
        if (nx == 0) return YAGI_OK;                                                                \
        CHECK_PTR(x);                                                                               \
        if (ny) {                                                                                   \
            CHECK_PTR(y);                                                                           \
            CHECK_NOALIAS(x, nx, y, ny);                                                            \
        }                                                                                           \
        YG_TRY(q->exec_dev(x, nx, y, ny));                                                          \
        *nw = ny;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_MSRESAMP_IMPL(rrrf, RRRF, float, float)
YAGI_MSRESAMP_IMPL(crcf, CRCF, yagi_cf32, float)
YAGI_MSRESAMP_IMPL(cccf, CCCF, yagi_cf32, yagi_cf32)

// ---- IirFilter (src/filter/iir/iirfilt.rs, iirfiltsos.rs) -----------------------------------------------------------
// State: TF = the VecDeque's logical v[0 .. n-1) (newest first) plus its physical head, which decides where the
// reference splits its dot products; SOS = [v0, v1] per section.  A host mirror serves execute() and short host blocks
// (host.cpp, the reference's order bit for bit); every group of the device path keeps its part of the state in a small
// device buffer.  The two copies are synchronised lazily, like DevWindow.
namespace yagi {

template <class T, class C> T host_iir_tf_step(T *s, size_t S, size_t *head, const C *a, const C *b, T x);   // host.cpp
template <class T, class C> T host_iir_sos_step(T *s, size_t nsec, const C *b, const C *a, T x);
template <class T, class C> T host_iir_scale(T y, C scale);
int design_iir_pintelon(bool differentiator, float *b, float *a);
int design_iir_lowpass_sos(int shape, size_t order, float fc, float ap, float as_, float *b, float *a);
int design_pll_active_lag(float w, float zeta, float k, float *b, float *a);
int iir_group_delay(const float *b, size_t nb, const float *a, size_t na, float fc, float *out);

constexpr size_t kIirHostMax = 32;    // execute_block on host data: up to this many samples on the host mirror

static inline float c_re(float v) { return v; }
static inline float c_re(cf32 v) { return v.re; }
static inline cf32 c_div(cf32 a, cf32 b) {     // num-complex Div
    const float d = b.re * b.re + b.im * b.im;
    return cf32{(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}
static inline float c_div(float a, float b) { return a / b; }
static inline std::complex<double> c_64(float v) { return {(double)v, 0.0}; }
static inline std::complex<double> c_64(cf32 v) { return {(double)v.re, (double)v.im}; }
static inline cf32 c_f32(cf32 v) { return v; }
static inline cf32 c_f32(float v) { return cf32{v, 0.0f}; }
static inline cf32 c_mul32(cf32 a, cf32 b) { return cf32{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
static inline cf32 c_add32(cf32 a, cf32 b) { return cf32{a.re + b.re, a.im + b.im}; }
static inline cf32 c_polar(float th) { return cf32{std::cos(th), std::sin(th)}; }

// one kernel pass: the whole TF filter or up to kIirSosGroup sections
template <class K>
struct IirGroup {
    using M = typename IirF64<K>::M;
    using V = typename IirF64<K>::V;
    IirParams<K> p{};
    size_t off = 0;                 // first state entry of this group in the object's state
    DevBuf tab, state, z, agg, init;

    // A = the state transition with zero input, column j = one step from the unit state e_j, in f64 from the
    // normalised f32 coefficients; P_0 = A^T by squaring, P_k = P_{k-1}^2
    int build(hipStream_t st) {
        const int S = p.S;
        using cd = std::complex<double>;
        std::vector<cd> A((size_t)S * S), s(S), t(S);
        for (int j = 0; j < S; ++j) {
            std::fill(s.begin(), s.end(), cd(0.0));
            s[j] = 1.0;
            if (!p.sos) {
                cd w = 0.0;
                for (int i = 1; i <= S; ++i) w -= c_64(p.a[i]) * s[i - 1];
                t[0] = w;
                for (int i = 1; i < S; ++i) t[i] = s[i - 1];
            } else {
                cd u = 0.0;
                for (int k = 0; k < p.n; ++k) {
                    const cd v1 = s[2 * k], v2 = s[2 * k + 1];
                    const cd v0 = u - c_64(p.a[3 * k + 1]) * v1 - c_64(p.a[3 * k + 2]) * v2;
                    u = c_64(p.b[3 * k]) * v0 + c_64(p.b[3 * k + 1]) * v1 + c_64(p.b[3 * k + 2]) * v2;
                    t[2 * k] = v0;
                    t[2 * k + 1] = v1;
                }
            }
            for (int i = 0; i < S; ++i) A[(size_t)i * S + j] = t[i];
        }
        auto sq = [S](const std::vector<cd> &X) {
            std::vector<cd> Y((size_t)S * S, cd(0.0));
            for (int i = 0; i < S; ++i)
                for (int k = 0; k < S; ++k) {
                    const cd x = X[(size_t)i * S + k];
                    if (x == cd(0.0)) continue;
                    for (int j = 0; j < S; ++j) Y[(size_t)i * S + j] += x * X[(size_t)k * S + j];
                }
            return Y;
        };
        for (int t2 = 1; t2 < p.T; t2 <<= 1) A = sq(A);
        std::vector<M> h((size_t)kIirLevels * S * S);
        for (int k = 0; k < kIirLevels; ++k) {
            if (k) A = sq(A);
            for (size_t e = 0; e < (size_t)S * S; ++e) store(h[(size_t)k * S * S + e], A[e]);
        }
        YG_TRY(fill(tab, h.data(), h.size() * sizeof(M), st));
        YG_TRY(state.alloc((size_t)S * sizeof(typename K::T)));
        return YAGI_OK;
    }
    static void store(double &d, std::complex<double> v) { d = v.real(); }
    static void store(dcplx &d, std::complex<double> v) { d = dcplx{v.real(), v.imag()}; }
    int scratch(size_t n) {                     // the scan's own scratch for n filter steps
        using T = typename K::T;
        const size_t nc = (n + (size_t)p.T - 1) / (size_t)p.T;
        const size_t G = (nc + kIirWg - 1) / kIirWg;
        YG_TRY(z.ensure(nc * (size_t)p.S * sizeof(T)));
        YG_TRY(agg.ensure(G * (size_t)p.S * sizeof(V)));
        return init.ensure(G * (size_t)p.S * sizeof(V));
    }
    int run(const typename K::T *x, size_t n, typename K::T *y, hipStream_t st) {
        using T = typename K::T;
        YG_TRY(scratch(n));
        return launch_iir<K>(p, x, n, y, state.template as<T>(), z.template as<T>(), agg.p, init.p, tab.p, kIirLevels, st);
    }
    // the mapped forms over n filter steps (kernels.hpp)
    int run_rate(const IirRateIo<K> &io, size_t n, hipStream_t st) {
        using T = typename K::T;
        YG_TRY(scratch(n));
        return launch_iir_rate<K>(p, io, n, state.template as<T>(), z.template as<T>(), agg.p, init.p, tab.p, kIirLevels, st);
    }
    int run_hilb(const IirHilbIo &io, size_t n, hipStream_t st) {
        YG_TRY(scratch(n));
        return launch_iir_hilb(p, io, n, state.template as<cf32>(), z.template as<cf32>(), agg.p, init.p, tab.p, kIirLevels, st);
    }
};

template <class K>
struct IirObj {
    using T = typename K::T;
    using C = typename K::C;
    hipStream_t st = nullptr;
    bool sos = false;
    size_t n = 0, nb = 0, na = 0, nsos = 0;     // get_length() = n (TF) or 2 nsos (SOS)
    std::vector<C> b, a;                        // TF: normalised, zero-padded to n; SOS: normalised per section
    std::vector<C> braw, araw;                  // SOS: as given (freqresponse reads them, iirfilt.rs:437-447)
    C scale = one_of<C>();
    size_t head = 0;                            // TF: the VecDeque's physical head
    std::vector<T> hs;                          // host mirror of the state
    Mirror mirror;
    std::vector<std::unique_ptr<IirGroup<K>>> groups;
    DevBuf mid, mid2;                           // mid2: the mapped forms' second intermediate (their y is no spare)
    Staging ws;

    size_t S() const { return hs.size(); }
    static int chunk_len(int S) {               // the combine (2 x 6 levels of S^2 f64 MACs per chunk) <= ~1/4
        int T = 64;
        while (T < 256 && T < 8 * S) T <<= 1;
        return T;
    }
    int build() {
        YG_TRY(require_device());
        if (!sos) {
            auto g = std::make_unique<IirGroup<K>>();
            g->p.sos = 0;
            g->p.n = (int)n;
            g->p.S = (int)n - 1;
            for (size_t i = 0; i < n; ++i) { g->p.b[i] = b[i]; g->p.a[i] = a[i]; }
            groups.push_back(std::move(g));
        } else {
            for (size_t s0 = 0; s0 < nsos; s0 += kIirSosGroup) {
                auto g = std::make_unique<IirGroup<K>>();
                const size_t ns = std::min((size_t)kIirSosGroup, nsos - s0);
                g->p.sos = 1;
                g->p.n = (int)ns;
                g->p.S = (int)(2 * ns);
                g->off = 2 * s0;
                for (size_t i = 0; i < 3 * ns; ++i) { g->p.b[i] = b[3 * s0 + i]; g->p.a[i] = a[3 * s0 + i]; }
                groups.push_back(std::move(g));
            }
        }
        for (auto &g : groups) {
            g->p.T = chunk_len(g->p.S);
            g->p.scale = one_of<C>();
            YG_TRY(g->build(st));
        }
        hs.assign(sos ? 2 * nsos : n - 1, T{});
        mirror.host_written();
        return YAGI_OK;
    }
    int init_tf(const C *b_, size_t nb_, const C *a_, size_t na_) {        // new() :65-100
        if (nb_ == 0) return fail(YAGI_ERR_CONFIG, "numerator length cannot be zero");
        if (na_ == 0) return fail(YAGI_ERR_CONFIG, "denominator length cannot be zero");
        nb = nb_; na = na_;
        n = std::max(na, nb);
        if (n > (size_t)kIirTfMaxN)
            return fail(YAGI_ERR_CONFIG, "iirfilt: transfer-function filters are limited to %d coefficients (got %zu): "
                        "in f32 they are unusable beyond about 8 (iirfilt.rs:53-56); use second-order sections",
                        kIirTfMaxN, n);
        const C a0 = a_[0];
        b.assign(n, C{});
        a.assign(n, C{});
        for (size_t i = 0; i < nb; ++i) b[i] = c_div(b_[i], a0);
        for (size_t i = 0; i < na; ++i) a[i] = c_div(a_[i], a0);
        sos = false;
        return build();
    }
    int init_sos(const C *b_, const C *a_, size_t nsos_) {                  // new_sos() :111-137
        if (nsos_ == 0) return fail(YAGI_ERR_CONFIG, "filter must have at least one 2nd-order section");
        nsos = nsos_;
        n = 2 * nsos;
        braw.assign(b_, b_ + 3 * nsos);
        araw.assign(a_, a_ + 3 * nsos);
        b.resize(3 * nsos);
        a.resize(3 * nsos);
        for (size_t k = 0; k < nsos; ++k) {                                  // IirFilterSos::set_coefficients
            const C a0 = a_[3 * k];
            for (int i = 0; i < 3; ++i) {
                b[3 * k + i] = c_div(b_[3 * k + i], a0);
                a[3 * k + i] = c_div(a_[3 * k + i], a0);
            }
        }
        sos = true;
        return build();
    }
    int ensure_host() {
        return mirror.need_host([&]() -> int {
            for (auto &g : groups) YG_TRY(download(hs.data() + g->off, g->state.p, (size_t)g->p.S * sizeof(T), st));
            return YAGI_OK;
        });
    }
    int ensure_dev() {
        return mirror.need_dev([&]() -> int {
            for (auto &g : groups) YG_TRY(upload(g->state.p, hs.data() + g->off, (size_t)g->p.S * sizeof(T), st));
            return YAGI_OK;
        });
    }
    int reset() {                         // :333-343 (the deque keeps its head); the device copy follows at its next use
        std::fill(hs.begin(), hs.end(), T{});
        mirror.in_sync();                 // every entry of the host copy is new, whatever it missed before ...
        mirror.host_written();            // ... and the device copy has not seen it
        return YAGI_OK;
    }
    T one_host(T x) {                                                        // execute() :385-390
        T y = sos ? host_iir_sos_step<T, C>(hs.data(), nsos, b.data(), a.data(), x)
                  : host_iir_tf_step<T, C>(hs.data(), hs.size(), &head, a.data(), b.data(), x);
        return host_iir_scale<T, C>(y, scale);
    }
    int block_host_mirror(const T *x, size_t nx, T *y) {
        YG_TRY(ensure_host());
        mirror.host_written();
        for (size_t i = 0; i < nx; ++i) y[i] = one_host(x[i]);
        return YAGI_OK;
    }
    int block_dev(const T *x, size_t nx, T *y) {
        if (nx == 0) return YAGI_OK;
        YG_TRY(ensure_dev());
        mirror.dev_written();
        const size_t ng = groups.size();
        if (ng > 1) YG_TRY(mid.ensure(nx * sizeof(T)));
        const T *in = x;
        for (size_t g = 0; g < ng; ++g) {
            IirGroup<K> &G = *groups[g];
            T *out = ((ng - 1 - g) % 2 == 0) ? y : mid.template as<T>();
            G.p.scale = (g + 1 == ng) ? scale : one_of<C>();
            if (!sos) G.p.head0 = (uint32_t)head;
            YG_TRY(G.run(in, nx, out, st));
            in = out;
        }
        if (!sos) head = (head + n - nx % n) % n;
        return YAGI_OK;
    }
    // The mapped forms (IirDecim, IirInterp, IirHilbertFilter): one pass per group over nsteps filter steps.
    // pass(group, in, out) launches it; in / out are the intermediate streams at the filter's rate, nullptr where the
    // pass reads the caller's x through the input map (first group) or writes its y through the output map (last).
    template <class F>
    int run_groups(size_t nsteps, F &&pass) {
        YG_TRY(ensure_dev());
        mirror.dev_written();
        const size_t ng = groups.size();
        if (ng > 1) YG_TRY(mid.ensure(nsteps * sizeof(T)));
        if (ng > 2) YG_TRY(mid2.ensure(nsteps * sizeof(T)));
        const T *in = nullptr;
        for (size_t g = 0; g < ng; ++g) {
            IirGroup<K> &G = *groups[g];
            T *out = (g + 1 == ng) ? nullptr : (g % 2 == 0 ? mid : mid2).template as<T>();
            G.p.scale = (g + 1 == ng) ? scale : one_of<C>();
            if (!sos) G.p.head0 = (uint32_t)head;
            YG_TRY(pass(G, in, out));
            in = out;
        }
        if (!sos) head = (head + n - nsteps % n) % n;
        return YAGI_OK;
    }
    int block_host(const T *x, size_t nx, T *y) {
        if (nx == 0) return YAGI_OK;
        if (nx <= kIirHostMax) return block_host_mirror(x, nx, y);
        return ws.run(st, x, nx, y, nx, [&](const T *xd, T *yd) { return block_dev(xd, nx, yd); });
    }
    // derive(Clone): VecDeque::clone rebuilds the deque contiguously, so the copy's head is 0 (same logical state)
    int clone_into(IirObj &o) {
        YG_TRY(ensure_host());
        o.st = st; o.sos = sos; o.n = n; o.nb = nb; o.na = na; o.nsos = nsos;
        o.b = b; o.a = a; o.braw = braw; o.araw = araw; o.scale = scale;
        YG_TRY(o.build());
        o.hs = hs;
        o.head = 0;
        return YAGI_OK;
    }
    // freqresponse (:416-451), Complex32 arithmetic as the reference spells it
    cf32 freqresponse(float fc) const {
        const float tp = 2.0f * 3.14159265358979323846f;
        cf32 h;
        if (!sos) {
            cf32 hb{0.0f, 0.0f}, ha{0.0f, 0.0f};
            for (size_t i = 0; i < nb; ++i) hb = c_add32(hb, c_mul32(c_f32(b[i]), c_polar(tp * fc * (float)i)));
            for (size_t i = 0; i < na; ++i) ha = c_add32(ha, c_mul32(c_f32(a[i]), c_polar(tp * fc * (float)i)));
            h = c_div(hb, ha);
        } else {
            h = cf32{1.0f, 0.0f};
            for (size_t k = 0; k < nsos; ++k) {
                const cf32 hb = c_add32(c_add32(c_mul32(c_f32(braw[3 * k]), c_polar(tp * fc * 0.0f)),
                                                c_mul32(c_f32(braw[3 * k + 1]), c_polar(tp * fc * 1.0f))),
                                        c_mul32(c_f32(braw[3 * k + 2]), c_polar(tp * fc * 2.0f)));
                const cf32 ha = c_add32(c_add32(c_mul32(c_f32(araw[3 * k]), c_polar(tp * fc * 0.0f)),
                                                c_mul32(c_f32(araw[3 * k + 1]), c_polar(tp * fc * 1.0f))),
                                        c_mul32(c_f32(araw[3 * k + 2]), c_polar(tp * fc * 2.0f)));
                h = c_mul32(h, c_div(hb, ha));
            }
        }
        return c_mul32(h, c_f32(scale));
    }
    int groupdelay(float fc, float *out) const {                             // :454-480
        if (!sos) {
            std::vector<float> br(nb), ar(na);
            for (size_t i = 0; i < nb; ++i) br[i] = c_re(b[i]);
            for (size_t i = 0; i < na; ++i) ar[i] = c_re(a[i]);
            return iir_group_delay(br.data(), nb, ar.data(), na, fc, out);
        }
        float gd = 0.0f;
        for (size_t k = 0; k < nsos; ++k) {                                  // iirfiltsos.rs:120-126
            const float bs[3] = {c_re(b[3 * k]), c_re(b[3 * k + 1]), c_re(b[3 * k + 2])};
            const float as[3] = {c_re(a[3 * k]), c_re(a[3 * k + 1]), c_re(a[3 * k + 2])};
            float g = 0.0f;
            YG_TRY(iir_group_delay(bs, 3, as, 3, fc, &g));
            gd += (g + 2.0f) - 2.0f;
        }
        *out = gd;
        return YAGI_OK;
    }
};

}  // namespace yagi

#define YAGI_IIRFILT_IMPL(K, KT, T, C)                                                              \
    struct yagi_hip_iirfilt_##K##_s : IirObj<KT> {};                                                \
    extern "C" {                                                                                    \
    int yagi_hip_iirfilt_##K##_create(const C *b, size_t nb, const C *a, size_t na,                 \
                                      yagi_hip_iirfilt_##K *q) try {                                \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        YG_TRY(require_device());                                                                   \
        if (nb) CHECK_PTR(b);                                                                       \
        if (na) CHECK_PTR(a);                                                                       \
        auto o = std::make_unique<yagi_hip_iirfilt_##K##_s>();                                      \
        YG_TRY(o->init_tf(b, nb, a, na));                                                           \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_create_sos(const C *b, const C *a, size_t nsos,                      \
                                          yagi_hip_iirfilt_##K *q) try {                            \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        YG_TRY(require_device());                                                                   \
        if (nsos) { CHECK_PTR(b); CHECK_PTR(a); }                                                   \
        auto o = std::make_unique<yagi_hip_iirfilt_##K##_s>();                                      \
        YG_TRY(o->init_sos(b, a, nsos));                                                            \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_create_dc_blocker(float alpha, yagi_hip_iirfilt_##K *q) try {  /* :290-305 */ \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        YG_TRY(require_device());                                                                   \
        if (alpha <= 0.0f) return fail(YAGI_ERR_CONFIG, "DC-blocking filter bandwidth must be greater than zero"); \
        const C bf[2] = {to_c(1.0f, (C *)nullptr), to_c(-1.0f, (C *)nullptr)};                     \
        const C af[2] = {to_c(1.0f, (C *)nullptr), to_c(-1.0f + alpha, (C *)nullptr)};              \
        YG_TRY(yagi_hip_iirfilt_##K##_create(bf, 2, af, 2, q));                                     \
        (*q)->scale = to_c(std::sqrt(1.0f - alpha), (C *)nullptr);                                  \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    static int iirfilt_##K##_pintelon(bool diff, yagi_hip_iirfilt_##K *q) {                         \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        YG_TRY(require_device());                                                                   \
        float bf[12] = {}, af[12] = {};                                                             \
        YG_TRY(design_iir_pintelon(diff, bf, af));                                                  \
        C bc[12], ac[12];                                                                           \
        for (int i = 0; i < 12; ++i) { bc[i] = to_c(bf[i], (C *)nullptr); ac[i] = to_c(af[i], (C *)nullptr); } \
        return yagi_hip_iirfilt_##K##_create_sos(bc, ac, 4, q);                                     \
    }                                                                                               \
    int yagi_hip_iirfilt_##K##_create_integrator(yagi_hip_iirfilt_##K *q) try {  /* :204-246 */     \
        return iirfilt_##K##_pintelon(false, q);                                                    \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_create_differentiator(yagi_hip_iirfilt_##K *q) try {  /* :248-288 */ \
        return iirfilt_##K##_pintelon(true, q);                                                     \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_create_pll(float w, float zeta, float k, yagi_hip_iirfilt_##K *q) try { /* :310-330 */ \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        YG_TRY(require_device());                                                                   \
        if (w <= 0.0f || w >= 1.0f) return fail(YAGI_ERR_CONFIG, "PLL bandwidth must be in (0,1)"); \
        if (zeta <= 0.0f || zeta >= 1.0f) return fail(YAGI_ERR_CONFIG, "PLL damping factor must be in (0,1)"); \
        if (k <= 0.0f) return fail(YAGI_ERR_CONFIG, "PLL loop gain must be greater than zero");     \
        float bf[3], af[3];                                                                         \
        YG_TRY(design_pll_active_lag(w, zeta, k, bf, af));                                          \
        C bc[3], ac[3];                                                                             \
        for (int i = 0; i < 3; ++i) { bc[i] = to_c(bf[i], (C *)nullptr); ac[i] = to_c(af[i], (C *)nullptr); } \
        return yagi_hip_iirfilt_##K##_create_sos(bc, ac, 1, q);                                     \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_destroy(yagi_hip_iirfilt_##K q) try {                                \
        if (q) (void)hipStreamSynchronize(q->st);                                                   \
        delete q;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_clone(yagi_hip_iirfilt_##K q, yagi_hip_iirfilt_##K *out) try {       \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        auto o = std::make_unique<yagi_hip_iirfilt_##K##_s>();                                      \
        YG_TRY(q->clone_into(*o));                                                                  \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_set_stream(yagi_hip_iirfilt_##K q, yagi_stream_t s) try {            \
        CHECK_Q(q);                                                                                 \
        if (q->st == to_stream(s)) return YAGI_OK;                                                  \
        YG_HIP(hipStreamSynchronize(q->st));                                                        \
        q->st = to_stream(s);                                                                       \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_reset(yagi_hip_iirfilt_##K q) try {                                  \
        CHECK_Q(q);                                                                                 \
        return q->reset();                                                                          \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_set_scale(yagi_hip_iirfilt_##K q, C scale) try {                     \
        CHECK_Q(q);                                                                                 \
        q->scale = scale;                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_get_scale(yagi_hip_iirfilt_##K q, C *scale) try {                    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(scale);                                                                           \
        *scale = q->scale;                                                                          \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_get_length(yagi_hip_iirfilt_##K q, size_t *len) try {                \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(len);                                                                             \
        *len = q->n;                                                                                \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_execute(yagi_hip_iirfilt_##K q, T x, T *y) try {                     \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(y);                                                                               \
        return q->block_host_mirror(&x, 1, y);                                                      \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_execute_block(yagi_hip_iirfilt_##K q, const T *x, size_t nx, T *y,   \
                                             size_t ny) try {                                       \
        CHECK_Q(q);                                                                                 \
        if (nx != ny) return fail(YAGI_ERR_CONFIG, "input and output block lengths must be equal"); \
        if (nx == 0) return YAGI_OK;                                                                \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        return q->block_host(x, nx, y);                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_execute_block_dev(yagi_hip_iirfilt_##K q, const T *x, size_t n, T *y) try { \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        CHECK_NOALIAS(x, n, y, n);                                                                  \
        return q->block_dev(x, n, y);                                                               \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_freqresponse(yagi_hip_iirfilt_##K q, float fc, yagi_cf32 *H) try {   \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(H);                                                                               \
        *H = q->freqresponse(fc);                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_get_psd(yagi_hip_iirfilt_##K q, float fc, float *psd) try { /* :453-457 */ \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(psd);                                                                             \
        const yagi_cf32 h = q->freqresponse(fc);                                                    \
        *psd = 10.0f * std::log10(h.re * h.re - h.im * -h.im);                                      \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_groupdelay(yagi_hip_iirfilt_##K q, float fc, float *gd) try {        \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(gd);                                                                              \
        return q->groupdelay(fc, gd);                                                               \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_IIRFILT_IMPL(rrrf, RRRF, float, float)
YAGI_IIRFILT_IMPL(crcf, CRCF, yagi_cf32, float)
YAGI_IIRFILT_IMPL(cccf, CCCF, yagi_cf32, yagi_cf32)

// ---- IIR design and the prototype constructors of IirFilter (iirfilt.rs:148-201) ---------------------------------------
namespace yagi {
// IirFilter::new_prototype on the low-pass / second-order-section branch
template <class K>
static int iir_init_prototype(IirObj<K> &o, int shape, size_t order, float fc, float ap, float as_) {
    using C = typename K::C;
    if (order > 4096) return fail(YAGI_ERR_CONFIG, "iir design: filter order %zu too large", order);
    const size_t ns = (order + 1) / 2;
    std::vector<float> bf(3 * ns + 3), af(3 * ns + 3);
    YG_TRY(design_iir_lowpass_sos(shape, order, fc, ap, as_, bf.data(), af.data()));
    std::vector<C> bc(3 * ns), ac(3 * ns);
    for (size_t i = 0; i < 3 * ns; ++i) { bc[i] = to_c(bf[i], (C *)nullptr); ac[i] = to_c(af[i], (C *)nullptr); }
    return o.init_sos(bc.data(), ac.data(), ns);
}
}  // namespace yagi

extern "C" int yagi_hip_iir_design_lowpass_sos(int shape, size_t order, float fc, float ap, float as_, float *b, float *a) try {
    if (order) { CHECK_PTR(b); CHECK_PTR(a); }
    return design_iir_lowpass_sos(shape, order, fc, ap, as_, b, a);
} catch (...) { return ::yagi::api_exception(); }

#define YAGI_IIRFILT_PROTO_IMPL(K)                                                                  \
    extern "C" {                                                                                    \
    int yagi_hip_iirfilt_##K##_create_prototype(int shape, size_t order, float fc, float ap, float as_, \
                                                yagi_hip_iirfilt_##K *q) try {                      \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        YG_TRY(require_device());                                                                   \
        auto o = std::make_unique<yagi_hip_iirfilt_##K##_s>();                                      \
        YG_TRY(iir_init_prototype(*o, shape, order, fc, ap, as_));                                  \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_iirfilt_##K##_create_lowpass(size_t order, float fc, yagi_hip_iirfilt_##K *q) try { \
        return yagi_hip_iirfilt_##K##_create_prototype(YAGI_IIRDES_BUTTER, order, fc, 0.1f, 60.0f, q); \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }
YAGI_IIRFILT_PROTO_IMPL(rrrf)
YAGI_IIRFILT_PROTO_IMPL(crcf)
YAGI_IIRFILT_PROTO_IMPL(cccf)

// ---- IirDecimationFilter / IirInterpolationFilter (src/filter/iir/iirdecim.rs, iirinterp.rs) -------------------------
// One IirObj run over the virtual stream of n M filter steps: the decimator keeps the output of step i M, the
// interpolator feeds x[i] at step i M and +0.0 elsewhere.  The kernels map the indices (iir_kernels.hip), so no buffer
// of n M samples exists on the sparse side.
namespace yagi {

template <class K, bool INTERP>
struct IirRateObj {
    using T = typename K::T;
    using C = typename K::C;
    IirObj<K> f;
    size_t M = 0;

    int set_rate(size_t m) {
        if (m < 2) return fail(YAGI_ERR_CONFIG, INTERP ? "interp factor must be greater than 1" : "decimation factor must be greater than 1");
        if (m > kIirMaxRate) return fail(YAGI_ERR_CONFIG, "rates above %u are not built", kIirMaxRate);
        M = m;
        return YAGI_OK;
    }
    int init_prototype(size_t m, int shape, size_t order, float fc, float ap, float as_) {
        YG_TRY(set_rate(m));
        YG_TRY(iir_init_prototype(f, shape, order, fc, ap, as_));
        if (INTERP) f.scale = to_c((float)M, (C *)nullptr);                 // iirinterp.rs:66-69
        return YAGI_OK;
    }
    void unit_host(const T *x, T *y) {                                       // execute(): iirdecim.rs:128-137, iirinterp.rs:93-103
        for (size_t i = 0; i < M; ++i) {
            if (INTERP) {
                y[i] = f.one_host(i == 0 ? *x : T{});
            } else {
                const T v = f.one_host(x[i]);
                if (i == 0) *y = v;
            }
        }
    }
    int block_host_mirror(const T *x, size_t nunits, T *y) {
        YG_TRY(f.ensure_host());
        f.mirror.host_written();
        for (size_t i = 0; i < nunits; ++i) unit_host(x + i * (INTERP ? 1 : M), y + i * (INTERP ? M : 1));
        return YAGI_OK;
    }
    int block_dev(const T *x, size_t nunits, T *y) {
        if (nunits == 0) return YAGI_OK;
        if (nunits > ((size_t)1 << 62) / M) return fail(YAGI_ERR_CONFIG, "block of %zu units too long", nunits);
        const size_t steps = nunits * M;
        return f.run_groups(steps, [&](IirGroup<K> &G, const T *in, T *out) -> int {
            const bool sparse_in = INTERP && !in, sparse_out = !INTERP && !out;
            const T *xi = in ? in : x;
            T *yo = out ? out : y;
            if (!sparse_in && !sparse_out) return G.run(xi, steps, yo, f.st);        // the plain kernel at the filter's rate
            return G.run_rate(IirRateIo<K>{xi, yo, (uint32_t)M, sparse_in, sparse_out}, steps, f.st);
        });
    }
    int block_host(const T *x, size_t nunits, T *y) {
        if (nunits == 0) return YAGI_OK;
        if (nunits <= kIirHostMax / M) return block_host_mirror(x, nunits, y);
        const size_t nx = INTERP ? nunits : nunits * M, ny = INTERP ? nunits * M : nunits;
        return f.ws.run(f.st, x, nx, y, ny, [&](const T *xd, T *yd) { return block_dev(xd, nunits, yd); });
    }
    int groupdelay(float fc, float *out) const {
        YG_TRY(f.groupdelay(fc, out));
        if (INTERP) *out = *out / (float)M;                                  // iirinterp.rs:118-120
        return YAGI_OK;
    }
};

}  // namespace yagi

#define YAGI_IIRRATE_IMPL(NAME, INTERP, GET, K, KT, T, C, EXEC_X, EXEC_XP)                          \
    struct yagi_hip_##NAME##_##K##_s : IirRateObj<KT, INTERP> {};                                   \
    extern "C" {                                                                                    \
    int yagi_hip_##NAME##_##K##_create(size_t M, const C *b, size_t nb, const C *a, size_t na,      \
                                       yagi_hip_##NAME##_##K *q) try {                              \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        YG_TRY(require_device());                                                                   \
        if (nb) CHECK_PTR(b);                                                                       \
        if (na) CHECK_PTR(a);                                                                       \
        auto o = std::make_unique<yagi_hip_##NAME##_##K##_s>();                                     \
        YG_TRY(o->set_rate(M));                                                                     \
        YG_TRY(o->f.init_tf(b, nb, a, na));                                                         \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_create_sos(size_t M, const C *b, const C *a, size_t nsos,           \
                                           yagi_hip_##NAME##_##K *q) try {                          \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        YG_TRY(require_device());                                                                   \
        if (nsos) { CHECK_PTR(b); CHECK_PTR(a); }                                                   \
        auto o = std::make_unique<yagi_hip_##NAME##_##K##_s>();                                     \
        YG_TRY(o->set_rate(M));                                                                     \
        YG_TRY(o->f.init_sos(b, a, nsos));                                                          \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_create_prototype(size_t M, int shape, size_t order, float fc, float ap, float as_, \
                                                 yagi_hip_##NAME##_##K *q) try {                    \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        YG_TRY(require_device());                                                                   \
        auto o = std::make_unique<yagi_hip_##NAME##_##K##_s>();                                     \
        YG_TRY(o->init_prototype(M, shape, order, fc, ap, as_));                                    \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_create_default(size_t M, size_t order, yagi_hip_##NAME##_##K *q) try { \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        return yagi_hip_##NAME##_##K##_create_prototype(M, INTERP ? YAGI_IIRDES_CHEBY2 : YAGI_IIRDES_BUTTER, order, \
                                                        0.5f / (float)M, 0.1f, 60.0f, q);           \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_destroy(yagi_hip_##NAME##_##K q) try {                              \
        if (q) (void)hipStreamSynchronize(q->f.st);                                                 \
        delete q;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_clone(yagi_hip_##NAME##_##K q, yagi_hip_##NAME##_##K *out) try {    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        auto o = std::make_unique<yagi_hip_##NAME##_##K##_s>();                                     \
        YG_TRY(q->f.clone_into(o->f));                                                              \
        o->M = q->M;                                                                                \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_set_stream(yagi_hip_##NAME##_##K q, yagi_stream_t s) try {          \
        CHECK_Q(q);                                                                                 \
        if (q->f.st == to_stream(s)) return YAGI_OK;                                                \
        YG_HIP(hipStreamSynchronize(q->f.st));                                                      \
        q->f.st = to_stream(s);                                                                     \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_reset(yagi_hip_##NAME##_##K q) try {                                \
        CHECK_Q(q);                                                                                 \
        return q->f.reset();                                                                        \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_execute(yagi_hip_##NAME##_##K q, EXEC_X x, T *y) try {              \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(y);                                                                               \
        CHECK_PTR(EXEC_XP);                                                                         \
        return q->block_host_mirror(EXEC_XP, 1, y);                                                 \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_execute_block(yagi_hip_##NAME##_##K q, const T *x, size_t n, T *y) try { \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        return q->block_host(x, n, y);                                                              \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_execute_block_dev(yagi_hip_##NAME##_##K q, const T *x, size_t n, T *y) try { \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        if (n > ((size_t)1 << 58) / q->M) return fail(YAGI_ERR_CONFIG, "block of %zu units too long", n); \
        CHECK_NOALIAS(x, INTERP ? n : n * q->M, y, INTERP ? n * q->M : n);                          \
        return q->block_dev(x, n, y);                                                               \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_groupdelay(yagi_hip_##NAME##_##K q, float fc, float *gd) try {      \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(gd);                                                                              \
        return q->groupdelay(fc, gd);                                                               \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_##GET(yagi_hip_##NAME##_##K q, size_t *M) try {                     \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(M);                                                                               \
        *M = q->M;                                                                                  \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_set_scale(yagi_hip_##NAME##_##K q, C scale) try {                   \
        CHECK_Q(q);                                                                                 \
        q->f.scale = scale;                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_##NAME##_##K##_get_scale(yagi_hip_##NAME##_##K q, C *scale) try {                  \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(scale);                                                                           \
        *scale = q->f.scale;                                                                        \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_IIRRATE_IMPL(iirdecim, false, get_decim, rrrf, RRRF, float, float, const float *, x)
YAGI_IIRRATE_IMPL(iirdecim, false, get_decim, crcf, CRCF, yagi_cf32, float, const yagi_cf32 *, x)
YAGI_IIRRATE_IMPL(iirdecim, false, get_decim, cccf, CCCF, yagi_cf32, yagi_cf32, const yagi_cf32 *, x)
YAGI_IIRRATE_IMPL(iirinterp, true, get_interp, rrrf, RRRF, float, float, float, &x)
YAGI_IIRRATE_IMPL(iirinterp, true, get_interp, crcf, CRCF, yagi_cf32, float, yagi_cf32, &x)
YAGI_IIRRATE_IMPL(iirinterp, true, get_interp, cccf, CCCF, yagi_cf32, yagi_cf32, yagi_cf32, &x)

// ---- IirHilbertFilter (src/filter/iir/iirhilb.rs) -------------------------------------------------------------------
// filt_0 and filt_1 share their coefficients and each takes exactly one step per call, so the pair is one crcf filter
// over u = (input of filt_0, input of filt_1): real coefficients act on re and im separately, in the same operations.
// The 2-bit state lives on the host and advances by the call's length at once, with no wait on the kernel.
namespace yagi {

struct IirHilbObj {
    enum Mode { R2C = 0, C2R = 1, DECIM = 2, INTERP = 3 };
    IirObj<CRCF> f;
    uint8_t state = 0;

    int init(int shape, size_t n, float ap, float as_) {                     // new() :15-36
        if (n == 0) return fail(YAGI_ERR_CONFIG, "filter order must be greater than zero");
        return iir_init_prototype(f, shape, n, 0.25f, ap, as_);
    }
    int reset() {                                                            // :49-53
        state = 0;
        return f.reset();
    }
    // decim / interp compute 1 - state on a u8 (:137, :157)
    int check_toggle() const {
        if (state > 1) return fail(YAGI_ERR_MODE, "iirhilbf: decim / interp after r2c / c2r left the state at %d: reset first", (int)state);
        return YAGI_OK;
    }
    cf32 r2c_one(float x) {                                                  // :55-82
        cf32 y;
        switch (state) {
        case 0: { const cf32 v = f.one_host(cf32{x, 0.0f}); y = cf32{2.0f * v.re, 2.0f * v.im}; break; }
        case 1: { const cf32 v = f.one_host(cf32{0.0f, -x}); y = cf32{2.0f * -v.im, 2.0f * v.re}; break; }
        case 2: { const cf32 v = f.one_host(cf32{-x, 0.0f}); y = cf32{2.0f * -v.re, 2.0f * -v.im}; break; }
        default: { const cf32 v = f.one_host(cf32{0.0f, x}); y = cf32{2.0f * v.im, 2.0f * -v.re}; break; }
        }
        state = (state + 1) & 3;
        return y;
    }
    float c2r_one(cf32 x) {                                                  // :90-117
        float y;
        switch (state) {
        case 0: y = f.one_host(cf32{x.re, x.im}).re; break;
        case 1: y = -f.one_host(cf32{x.im, -x.re}).im; break;
        case 2: y = -f.one_host(cf32{-x.re, -x.im}).re; break;
        default: y = f.one_host(cf32{-x.im, x.re}).im; break;
        }
        state = (state + 1) & 3;
        return y;
    }
    cf32 decim_one(const float *x) {                                         // :125-139
        const float xi = state ? -x[0] : x[0], xq = state ? x[1] : -x[1];
        const cf32 v = f.one_host(cf32{xi, 0.0f});
        (void)f.one_host(cf32{0.0f, xq});
        state = 1 - state;
        return cf32{2.0f * v.re, 2.0f * v.im};
    }
    void interp_one(cf32 x, float *y) {                                      // :147-158
        const cf32 v0 = f.one_host(x), v1 = f.one_host(cf32{0.0f, 0.0f});
        y[0] = state ? -2.0f * v0.re : 2.0f * v0.re;
        y[1] = state ? 2.0f * v1.im : -2.0f * v1.im;
        state = 1 - state;
    }
    static size_t in_bytes(int mode, size_t n) { return mode == R2C ? 4 * n : 8 * n; }
    static size_t out_bytes(int mode, size_t n) { return mode == C2R ? 4 * n : 8 * n; }
    int block_host_mirror(int mode, const void *x, size_t n, void *y) {
        if (mode >= DECIM) YG_TRY(check_toggle());
        YG_TRY(f.ensure_host());
        f.mirror.host_written();
        for (size_t i = 0; i < n; ++i) {
            if (mode == R2C) static_cast<cf32 *>(y)[i] = r2c_one(static_cast<const float *>(x)[i]);
            else if (mode == C2R) static_cast<float *>(y)[i] = c2r_one(static_cast<const cf32 *>(x)[i]);
            else if (mode == DECIM) static_cast<cf32 *>(y)[i] = decim_one(static_cast<const float *>(x) + 2 * i);
            else interp_one(static_cast<const cf32 *>(x)[i], static_cast<float *>(y) + 2 * i);
        }
        return YAGI_OK;
    }
    int block_dev(int mode, const void *x, size_t n, void *y) {
        if (mode >= DECIM) YG_TRY(check_toggle());
        if (n == 0) return YAGI_OK;
        if (n > ((size_t)1 << 60)) return fail(YAGI_ERR_CONFIG, "block of %zu units too long", n);
        const size_t steps = mode >= DECIM ? 2 * n : n;
        const uint32_t phase = mode >= DECIM ? 2u * state : state;
        static const int imodes[4] = {kHilbInReal, kHilbInCplx, kHilbInReal, kHilbInEven};
        static const int omodes[4] = {kHilbOutRot2, kHilbOutProj, kHilbOutEven2, kHilbOutProj2};
        YG_TRY(f.run_groups(steps, [&](IirGroup<CRCF> &G, const cf32 *in, cf32 *out) -> int {
            if (in && out) return G.run(in, steps, out, f.st);
            return G.run_hilb(IirHilbIo{in ? (const void *)in : x, out ? (void *)out : y, phase,
                                        in ? (int)kHilbInPlain : imodes[mode], out ? (int)kHilbOutPlain : omodes[mode]},
                              steps, f.st);
        }));
        state = mode >= DECIM ? (uint8_t)(state ^ (n & 1)) : (uint8_t)((state + n) & 3);
        return YAGI_OK;
    }
    int block_host(int mode, const void *x, size_t n, void *y) {
        if (n == 0) return YAGI_OK;
        if ((mode >= DECIM ? 2 * n : n) <= kIirHostMax) return block_host_mirror(mode, x, n, y);
        if (mode >= DECIM) YG_TRY(check_toggle());
        YG_TRY(f.ws.x.ensure(in_bytes(mode, n)));
        YG_TRY(f.ws.y.ensure(out_bytes(mode, n)));
        YG_TRY(upload(f.ws.x.p, x, in_bytes(mode, n), f.st));
        YG_TRY(block_dev(mode, f.ws.x.p, n, f.ws.y.p));
        return download(y, f.ws.y.p, out_bytes(mode, n), f.st);
    }
    // device buffers: decim and interp move the same bytes per unit and every tile row is loaded before it is stored,
    // so x == y is allowed there
    int block_dev_checked(int mode, const void *x, size_t n, void *y) {
        if (n == 0) return mode >= DECIM ? check_toggle() : YAGI_OK;
        if (n > ((size_t)1 << 60)) return fail(YAGI_ERR_CONFIG, "block of %zu units too long", n);
        if (!(mode >= DECIM && x == y)) YG_TRY(check_noalias(x, in_bytes(mode, n), y, out_bytes(mode, n)));
        return block_dev(mode, x, n, y);
    }
};

}  // namespace yagi

struct yagi_hip_iirhilbf_s : IirHilbObj {};
extern "C" {
int yagi_hip_iirhilbf_create(int shape, size_t n, float ap, float as_, yagi_hip_iirhilbf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    YG_TRY(require_device());
    auto o = std::make_unique<yagi_hip_iirhilbf_s>();
    YG_TRY(o->init(shape, n, ap, as_));
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_iirhilbf_create_default(size_t n, yagi_hip_iirhilbf *q) try {       // :38-47
    return yagi_hip_iirhilbf_create(YAGI_IIRDES_BUTTER, n, 0.1f, 60.0f, q);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_iirhilbf_create_sos(const float *b, const float *a, size_t nsos, yagi_hip_iirhilbf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    YG_TRY(require_device());
    if (nsos) { CHECK_PTR(b); CHECK_PTR(a); }
    auto o = std::make_unique<yagi_hip_iirhilbf_s>();
    YG_TRY(o->f.init_sos(b, a, nsos));
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_iirhilbf_destroy(yagi_hip_iirhilbf q) try {
    if (q) (void)hipStreamSynchronize(q->f.st);
    delete q;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_iirhilbf_clone(yagi_hip_iirhilbf q, yagi_hip_iirhilbf *out) try {
    CHECK_Q(q);
    CHECK_PTR(out);
    *out = nullptr;
    auto o = std::make_unique<yagi_hip_iirhilbf_s>();
    YG_TRY(q->f.clone_into(o->f));
    o->state = q->state;
    *out = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_iirhilbf_set_stream(yagi_hip_iirhilbf q, yagi_stream_t s) try {
    CHECK_Q(q);
    if (q->f.st == to_stream(s)) return YAGI_OK;
    YG_HIP(hipStreamSynchronize(q->f.st));
    q->f.st = to_stream(s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_iirhilbf_reset(yagi_hip_iirhilbf q) try {
    CHECK_Q(q);
    return q->reset();
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_iirhilbf_get_state(yagi_hip_iirhilbf q, int *state) try {
    CHECK_Q(q);
    CHECK_PTR(state);
    *state = q->state;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_iirhilbf_r2c_execute(yagi_hip_iirhilbf q, float x, yagi_cf32 *y) try {
    CHECK_Q(q);
    CHECK_PTR(y);
    return q->block_host_mirror(IirHilbObj::R2C, &x, 1, y);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_iirhilbf_c2r_execute(yagi_hip_iirhilbf q, yagi_cf32 x, float *y) try {
    CHECK_Q(q);
    CHECK_PTR(y);
    return q->block_host_mirror(IirHilbObj::C2R, &x, 1, y);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_iirhilbf_decim_execute(yagi_hip_iirhilbf q, const float *x, yagi_cf32 *y) try {
    CHECK_Q(q);
    CHECK_PTR(x);
    CHECK_PTR(y);
    return q->block_host_mirror(IirHilbObj::DECIM, x, 1, y);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_iirhilbf_interp_execute(yagi_hip_iirhilbf q, yagi_cf32 x, float *y) try {
    CHECK_Q(q);
    CHECK_PTR(y);
    return q->block_host_mirror(IirHilbObj::INTERP, &x, 1, y);
} catch (...) { return ::yagi::api_exception(); }
#define YAGI_IIRHILB_BLOCK(NAME, MODE, TX, TY)                                                                      \
    int yagi_hip_iirhilbf_##NAME##_execute_block(yagi_hip_iirhilbf q, const TX *x, size_t n, TY *y) try {           \
        CHECK_Q(q);                                                                                                 \
        if (n) { CHECK_PTR(x); CHECK_PTR(y); }                                                                      \
        return q->block_host(IirHilbObj::MODE, x, n, y);                                                            \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_iirhilbf_##NAME##_execute_block_dev(yagi_hip_iirhilbf q, const TX *x, size_t n, TY *y) try {       \
        CHECK_Q(q);                                                                                                 \
        if (n) { CHECK_PTR(x); CHECK_PTR(y); }                                                                      \
        return q->block_dev_checked(IirHilbObj::MODE, x, n, y);                                                     \
    } catch (...) { return ::yagi::api_exception(); }
YAGI_IIRHILB_BLOCK(r2c, R2C, float, yagi_cf32)
YAGI_IIRHILB_BLOCK(c2r, C2R, yagi_cf32, float)
YAGI_IIRHILB_BLOCK(decim, DECIM, float, yagi_cf32)
YAGI_IIRHILB_BLOCK(interp, INTERP, yagi_cf32, float)
}  // extern "C"

// ---- Osc (src/nco/osc.rs, nco.rs, vco.rs) -----------------------------------------------------------------------------
// The state is the reference's: two u32 words and the PLL gains, kept on the host.  A block call passes theta0 and
// d_theta to the kernel by value and advances theta by n d_theta mod 2^32 at once, so device calls need no
// synchronisation and the per-sample calls on the host (host.cpp) always see the carried phase.
namespace yagi {

void osc_device_table(int vco, std::vector<float> &out);                 // host.cpp
int osc_constrain(float theta, uint32_t *out);
float osc_phase(uint32_t theta);
float osc_frequency(uint32_t d_theta);
void osc_sin_cos(int vco, uint32_t theta, float *s, float *c);
cf32 osc_mix(int vco, uint32_t theta, bool down, cf32 x);

constexpr size_t kOscHostMax = 4096;    // mix_block on host slices: up to this many samples on the host

struct OscObj {
    hipStream_t st = nullptr;
    int vco = 0;
    uint32_t theta = 0, d_theta = 0;
    float alpha = 0.0f, beta = 0.0f;
    DevBuf tab;
    Staging ws;

    int init(int scheme) {                                                   // new() :37-57
        if (scheme != YAGI_OSC_NCO && scheme != YAGI_OSC_VCO) return fail(YAGI_ERR_CONFIG, "osc: unknown scheme %d", scheme);
        vco = scheme == YAGI_OSC_VCO;
        std::vector<float> h;
        osc_device_table(vco, h);
        YG_TRY(fill(tab, h.data(), h.size() * sizeof(float), st));
        YG_TRY(pll_set_bandwidth(0.1f));                                     // PLL_BANDWIDTH_DEFAULT
        theta = d_theta = 0;
        return YAGI_OK;
    }
    int pll_set_bandwidth(float bw) {                                        // :138-144
        if (bw < 0.0f) return fail(YAGI_ERR_CONFIG, "Bandwidth must be positive");
        alpha = bw;
        beta = std::sqrt(bw);
        return YAGI_OK;
    }
    int pll_step(float dphi) {                                               // :147-150 (both words first: no half update)
        uint32_t df = 0, dp = 0;
        YG_TRY(osc_constrain(dphi * alpha, &df));
        YG_TRY(osc_constrain(dphi * beta, &dp));
        d_theta += df;
        theta += dp;
        return YAGI_OK;
    }
    void block_host(const cf32 *x, size_t n, cf32 *y, bool down) {         // :161-188, mix then step
        for (size_t i = 0; i < n; ++i) {
            y[i] = osc_mix(vco, theta, down, x[i]);
            theta += d_theta;
        }
    }
    int block_dev(const cf32 *x, size_t n, cf32 *y, bool down) {
        if (n == 0) return YAGI_OK;
        YG_TRY(launch_osc_mix(vco, down, tab.p, theta, d_theta, x, y, n, st));
        theta += (uint32_t)n * d_theta;
        return YAGI_OK;
    }
    int block_host_slices(const cf32 *x, size_t n, cf32 *y, bool down) {
        if (n <= kOscHostMax) {
            block_host(x, n, y, down);
            return YAGI_OK;
        }
        return ws.run(st, x, n, y, n, [&](const cf32 *xd, cf32 *yd) { return block_dev(xd, n, yd, down); });
    }
};

}  // namespace yagi

struct yagi_hip_osc_s : OscObj {};

extern "C" {

int yagi_hip_osc_create(int scheme, yagi_hip_osc *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    YG_TRY(require_device());
    auto o = std::make_unique<yagi_hip_osc_s>();
    YG_TRY(o->init(scheme));
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_destroy(yagi_hip_osc q) try {
    if (q) (void)hipStreamSynchronize(q->st);
    delete q;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_clone(yagi_hip_osc q, yagi_hip_osc *out) try {                  // derive(Clone)
    CHECK_Q(q);
    CHECK_PTR(out);
    *out = nullptr;
    auto o = std::make_unique<yagi_hip_osc_s>();
    o->st = q->st;
    YG_TRY(o->init(q->vco ? YAGI_OSC_VCO : YAGI_OSC_NCO));
    o->theta = q->theta;
    o->d_theta = q->d_theta;
    o->alpha = q->alpha;
    o->beta = q->beta;
    *out = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_set_stream(yagi_hip_osc q, yagi_stream_t s) try {
    CHECK_Q(q);
    if (q->st == to_stream(s)) return YAGI_OK;
    YG_HIP(hipStreamSynchronize(q->st));
    q->st = to_stream(s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_reset(yagi_hip_osc q) try {                                     // :60-63
    CHECK_Q(q);
    q->theta = q->d_theta = 0;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_set_frequency(yagi_hip_osc q, float dtheta) try {               // :66-68
    CHECK_Q(q);
    return osc_constrain(dtheta, &q->d_theta);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_adjust_frequency(yagi_hip_osc q, float df) try {                // :71-73
    CHECK_Q(q);
    uint32_t w = 0;
    YG_TRY(osc_constrain(df, &w));
    q->d_theta += w;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_set_phase(yagi_hip_osc q, float phi) try {                      // :76-78
    CHECK_Q(q);
    return osc_constrain(phi, &q->theta);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_adjust_phase(yagi_hip_osc q, float dphi) try {                  // :81-83
    CHECK_Q(q);
    uint32_t w = 0;
    YG_TRY(osc_constrain(dphi, &w));
    q->theta += w;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_step(yagi_hip_osc q) try {                                      // :86-88
    CHECK_Q(q);
    q->theta += q->d_theta;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_get_phase(yagi_hip_osc q, float *phi) try {                     // :91-93
    CHECK_Q(q);
    CHECK_PTR(phi);
    *phi = osc_phase(q->theta);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_get_frequency(yagi_hip_osc q, float *f) try {                   // :96-103
    CHECK_Q(q);
    CHECK_PTR(f);
    *f = osc_frequency(q->d_theta);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_get_state(yagi_hip_osc q, uint32_t *theta, uint32_t *d_theta) try {   // extension
    CHECK_Q(q);
    CHECK_PTR(theta);
    CHECK_PTR(d_theta);
    *theta = q->theta;
    *d_theta = q->d_theta;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_sin(yagi_hip_osc q, float *s) try {                             // :106-111
    CHECK_Q(q);
    CHECK_PTR(s);
    float c = 0.0f;
    osc_sin_cos(q->vco, q->theta, s, &c);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_cos(yagi_hip_osc q, float *c) try {                             // :114-119
    CHECK_Q(q);
    CHECK_PTR(c);
    float s = 0.0f;
    osc_sin_cos(q->vco, q->theta, &s, c);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_sin_cos(yagi_hip_osc q, float *s, float *c) try {               // :122-127
    CHECK_Q(q);
    CHECK_PTR(s);
    CHECK_PTR(c);
    osc_sin_cos(q->vco, q->theta, s, c);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_cexp(yagi_hip_osc q, yagi_cf32 *y) try {                        // :130-133
    CHECK_Q(q);
    CHECK_PTR(y);
    float s = 0.0f, c = 0.0f;
    osc_sin_cos(q->vco, q->theta, &s, &c);
    *y = yagi_cf32{c, s};
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_pll_set_bandwidth(yagi_hip_osc q, float bw) try {
    CHECK_Q(q);
    return q->pll_set_bandwidth(bw);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_pll_step(yagi_hip_osc q, float dphi) try {
    CHECK_Q(q);
    return q->pll_step(dphi);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_mix_up(yagi_hip_osc q, yagi_cf32 x, yagi_cf32 *y) try {         // :155-158
    CHECK_Q(q);
    CHECK_PTR(y);
    *y = osc_mix(q->vco, q->theta, false, x);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_mix_down(yagi_hip_osc q, yagi_cf32 x, yagi_cf32 *y) try {       // :173-176
    CHECK_Q(q);
    CHECK_PTR(y);
    *y = osc_mix(q->vco, q->theta, true, x);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
static int osc_mix_block(yagi_hip_osc q, const yagi_cf32 *x, size_t nx, yagi_cf32 *y, size_t ny, bool down) {
    CHECK_Q(q);
    if (nx != ny) return fail(YAGI_ERR_RANGE, "Input and output slices must have the same length");
    if (nx == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    return q->block_host_slices(x, nx, y, down);
}
int yagi_hip_osc_mix_block_up(yagi_hip_osc q, const yagi_cf32 *x, size_t nx, yagi_cf32 *y, size_t ny) try {   // :161-170
    return osc_mix_block(q, x, nx, y, ny, false);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_mix_block_down(yagi_hip_osc q, const yagi_cf32 *x, size_t nx, yagi_cf32 *y, size_t ny) try { // :179-188
    return osc_mix_block(q, x, nx, y, ny, true);
} catch (...) { return ::yagi::api_exception(); }
static int osc_mix_block_dev(yagi_hip_osc q, const yagi_cf32 *x, size_t n, yagi_cf32 *y, bool down) {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    // in place (x == y) is fine: each lane reads its samples, then writes them; a partial overlap is not
    if (x != y && x < y + n && y < x + n)
        return fail(YAGI_ERR_CONFIG, "input and output buffers overlap without being the same buffer");
    return q->block_dev(x, n, y, down);
}
int yagi_hip_osc_mix_block_up_dev(yagi_hip_osc q, const yagi_cf32 *x, size_t n, yagi_cf32 *y) try {
    return osc_mix_block_dev(q, x, n, y, false);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_osc_mix_block_down_dev(yagi_hip_osc q, const yagi_cf32 *x, size_t n, yagi_cf32 *y) try {
    return osc_mix_block_dev(q, x, n, y, true);
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- FirHilbertFilter (src/filter/fir/firhilb.rs) ---------------------------------------------------------------------
// The state is the reference's: four Window<f32> of 2m samples and the toggle.  The per-sample calls run on a host
// mirror of the four windows (host.cpp: firhilb_dot, the reference's order); block calls run firhilb_kernels.hip on the
// device copy, which the kernels' state launch rewrites into the other of two buffers.  The two copies are synchronised
// lazily (DevWindow's pattern), and the host advances the toggle by the call's length at the call, so every mode may
// follow every other without a reset and without waiting for a kernel.
namespace yagi {

int firhilb_design(size_t m, float as_, std::vector<float> &hq);          // host.cpp
float firhilb_dot(const float *hq, const float *w, size_t L);

constexpr size_t kFirhilbHostMax = 4096;    // block calls on host slices: up to this many units on the host

struct FirHilbObj {
    hipStream_t st = nullptr;
    int m = 0, L = 0;
    bool toggle = false;
    std::vector<float> hq;
    std::vector<float> hw;               // host mirror: w0, w1, w2, w3, L each, oldest first
    DevBuf taps;
    PingPong<> win;
    Staging ws;
    Mirror mirror;

    int init(size_t m_, float as_) {                                         // new() :38-84
        YG_TRY(firhilb_design(m_, as_, hq));
        m = (int)m_;
        L = 2 * m;
        YG_TRY(fill(taps, hq.data(), hq.size() * sizeof(float), st));
        YG_TRY(win.alloc((size_t)4 * L * sizeof(float)));
        return reset();
    }
    int reset() {                                                            // :87-93
        hw.assign((size_t)4 * L, 0.0f);
        YG_HIP(hipMemsetAsync(win.cur(), 0, (size_t)4 * L * sizeof(float), st));
        toggle = false;
        mirror.in_sync();
        return YAGI_OK;
    }
    int ensure_host() {
        return mirror.need_host([&] { return download(hw.data(), win.cur(), hw.size() * sizeof(float), st); });
    }
    int ensure_dev() {
        return mirror.need_dev([&] { return upload(win.cur(), hw.data(), hw.size() * sizeof(float), st); });
    }
    // entry to the per-sample path: the host mirror is current and about to be written
    int enter_host() {
        YG_TRY(ensure_host());
        mirror.host_written();
        return YAGI_OK;
    }
    float *w(int i) { return hw.data() + (size_t)i * L; }
    void push(int i, float v) {                                              // Window::push: drop the oldest
        float *p = w(i);
        std::memmove(p, p + 1, (size_t)(L - 1) * sizeof(float));
        p[L - 1] = v;
    }
    float index(int i) { return w(i)[m - 1]; }                               // Window::index(m - 1)
    float dot(int i) { return firhilb_dot(hq.data(), w(i), (size_t)L); }     // hq.dotprod(window.read())

    // the per-sample calls (after enter_host)
    cf32 r2c(float x) {                                                      // :104-137
        cf32 y;
        if (!toggle) { push(0, x); y = cf32{index(0), dot(1)}; }
        else         { push(1, x); y = cf32{index(1), dot(0)}; }
        toggle = !toggle;
        return y;
    }
    void c2r(cf32 x, float *y) {                                             // :149-180
        float yi, yq;
        if (!toggle) { push(0, x.re); push(1, x.im); yi = index(0); yq = dot(3); }
        else         { push(2, x.re); push(3, x.im); yi = index(2); yq = dot(1); }
        toggle = !toggle;
        y[0] = yi + yq;
        y[1] = yi - yq;
    }
    cf32 decim(const float *x) {                                             // :191-211
        push(1, x[0]);
        const float yq = dot(1);
        push(0, x[1]);
        const float yi = index(0);
        cf32 y = toggle ? cf32{-yi, -yq} : cf32{yi, yq};
        toggle = !toggle;
        return y;
    }
    void interp(cf32 x, float *y) {                                          // :233-248
        const float vi = toggle ? -x.re : x.re, vq = toggle ? -x.im : x.im;
        push(0, vq);
        y[0] = index(0);
        push(1, vi);
        y[1] = dot(1);
        toggle = !toggle;
    }
    void block_host(int mode, const float *x, size_t n, float *y) {
        for (size_t i = 0; i < n; ++i) {
            switch (mode) {
            case FIRHILB_R2C: { const cf32 v = r2c(x[i]); y[2 * i] = v.re; y[2 * i + 1] = v.im; break; }
            case FIRHILB_C2R: c2r(cf32{x[2 * i], x[2 * i + 1]}, y + 2 * i); break;
            case FIRHILB_DECIM: { const cf32 v = decim(x + 2 * i); y[2 * i] = v.re; y[2 * i + 1] = v.im; break; }
            default: interp(cf32{x[2 * i], x[2 * i + 1]}, y + 2 * i); break;
            }
        }
    }
    int block_dev(int mode, const float *x, size_t n, float *y) {
        if (n == 0) return YAGI_OK;
        YG_TRY(ensure_dev());
        YG_TRY(launch_firhilb(mode, m, taps.as<float>(), win.cur<float>(), win.next<float>(), toggle ? 1 : 0, x, n, y, st));
        win.flip();
        mirror.dev_written();
        if (n & 1) toggle = !toggle;
        return YAGI_OK;
    }
    int block_host_slices(int mode, const float *x, size_t n, float *y) {
        const size_t xf = (mode == FIRHILB_R2C) ? n : 2 * n;                  // floats in and out
        const size_t yf = 2 * n;
        if (n <= kFirhilbHostMax) {
            YG_TRY(enter_host());
            block_host(mode, x, n, y);
            return YAGI_OK;
        }
        return ws.run(st, x, xf, y, yf, [&](const float *xd, float *yd) { return block_dev(mode, xd, n, yd); });
    }
};

}  // namespace yagi

struct yagi_hip_firhilb_s : FirHilbObj {};

extern "C" {

int yagi_hip_firhilb_create(size_t m, float as_, yagi_hip_firhilb *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    YG_TRY(require_device());
    auto o = std::make_unique<yagi_hip_firhilb_s>();
    YG_TRY(o->init(m, as_));
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_destroy(yagi_hip_firhilb q) try {
    if (q) (void)hipStreamSynchronize(q->st);
    delete q;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_clone(yagi_hip_firhilb q, yagi_hip_firhilb *out) try {       // derive(Clone)
    CHECK_Q(q);
    CHECK_PTR(out);
    *out = nullptr;
    YG_TRY(q->ensure_host());
    auto o = std::make_unique<yagi_hip_firhilb_s>();
    o->st = q->st;
    o->m = q->m;
    o->L = q->L;
    o->hq = q->hq;
    YG_TRY(fill(o->taps, o->hq.data(), o->hq.size() * sizeof(float), o->st));
    YG_TRY(o->win.alloc((size_t)4 * o->L * sizeof(float)));
    o->hw = q->hw;
    o->toggle = q->toggle;
    o->mirror.host_written();
    *out = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_set_stream(yagi_hip_firhilb q, yagi_stream_t s) try {
    CHECK_Q(q);
    if (q->st == to_stream(s)) return YAGI_OK;
    YG_HIP(hipStreamSynchronize(q->st));
    q->st = to_stream(s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_reset(yagi_hip_firhilb q) try {                              // :87-93
    CHECK_Q(q);
    return q->reset();
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_r2c_execute(yagi_hip_firhilb q, float x, yagi_cf32 *y) try {          // :104-137
    CHECK_Q(q);
    CHECK_PTR(y);
    YG_TRY(q->enter_host());
    *y = q->r2c(x);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_c2r_execute(yagi_hip_firhilb q, yagi_cf32 x, float *y0, float *y1) try {   // :149-180
    CHECK_Q(q);
    CHECK_PTR(y0);
    CHECK_PTR(y1);
    YG_TRY(q->enter_host());
    float y[2];
    q->c2r(x, y);
    *y0 = y[0];
    *y1 = y[1];
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_decim_execute(yagi_hip_firhilb q, const float *x, yagi_cf32 *y) try { // :191-211, x[0..2)
    CHECK_Q(q);
    CHECK_PTR(x);
    CHECK_PTR(y);
    YG_TRY(q->enter_host());
    *y = q->decim(x);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_interp_execute(yagi_hip_firhilb q, yagi_cf32 x, float *y) try {       // :233-248, y[0..2)
    CHECK_Q(q);
    CHECK_PTR(y);
    YG_TRY(q->enter_host());
    q->interp(x, y);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
// host slices: nx and ny are element counts of the caller's arrays; n = the number of units
static int firhilb_block(yagi_hip_firhilb q, int mode, const void *x, size_t nx, void *y, size_t ny) {
    CHECK_Q(q);
    size_t n = 0;
    bool ok = false;
    switch (mode) {
    case FIRHILB_R2C: n = nx; ok = ny == nx; break;                // n real -> n complex
    case FIRHILB_C2R: n = nx; ok = ny == 2 * nx; break;            // n complex -> 2n real
    case FIRHILB_DECIM: n = ny; ok = nx == 2 * ny; break;          // 2n real -> n complex
    default: n = nx; ok = ny == 2 * nx; break;                     // n complex -> 2n real
    }
    if (!ok) return fail(YAGI_ERR_RANGE, "firhilb: input (%zu) and output (%zu) lengths do not match", nx, ny);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    return q->block_host_slices(mode, static_cast<const float *>(x), n, static_cast<float *>(y));
}
static int firhilb_block_dev(yagi_hip_firhilb q, int mode, const void *x, size_t n, void *y) {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    const size_t xb = (mode == FIRHILB_R2C ? n : 2 * n) * sizeof(float), yb = 2 * n * sizeof(float);
    YG_TRY(check_noalias(x, xb, y, yb));
    return q->block_dev(mode, static_cast<const float *>(x), n, static_cast<float *>(y));
}
int yagi_hip_firhilb_r2c_execute_block(yagi_hip_firhilb q, const float *x, size_t nx, yagi_cf32 *y, size_t ny) try {
    return firhilb_block(q, FIRHILB_R2C, x, nx, y, ny);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_c2r_execute_block(yagi_hip_firhilb q, const yagi_cf32 *x, size_t nx, float *y, size_t ny) try {
    return firhilb_block(q, FIRHILB_C2R, x, nx, y, ny);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_decim_execute_block(yagi_hip_firhilb q, const float *x, size_t nx, yagi_cf32 *y, size_t ny) try {
    return firhilb_block(q, FIRHILB_DECIM, x, nx, y, ny);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_interp_execute_block(yagi_hip_firhilb q, const yagi_cf32 *x, size_t nx, float *y, size_t ny) try {
    return firhilb_block(q, FIRHILB_INTERP, x, nx, y, ny);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_r2c_execute_block_dev(yagi_hip_firhilb q, const float *x_dev, size_t n, yagi_cf32 *y_dev) try {
    return firhilb_block_dev(q, FIRHILB_R2C, x_dev, n, y_dev);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_c2r_execute_block_dev(yagi_hip_firhilb q, const yagi_cf32 *x_dev, size_t n, float *y_dev) try {
    return firhilb_block_dev(q, FIRHILB_C2R, x_dev, n, y_dev);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_decim_execute_block_dev(yagi_hip_firhilb q, const float *x_dev, size_t n, yagi_cf32 *y_dev) try {
    return firhilb_block_dev(q, FIRHILB_DECIM, x_dev, n, y_dev);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_firhilb_interp_execute_block_dev(yagi_hip_firhilb q, const yagi_cf32 *x_dev, size_t n, float *y_dev) try {
    return firhilb_block_dev(q, FIRHILB_INTERP, x_dev, n, y_dev);
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- Fdelay (src/filter/fdelay.rs) ---------------------------------------------------------------------------------
// The state is the reference's, cut to what its outputs depend on: the last nmax input samples (its Window of nmax + 1
// before the next push), the bank's window of Ls delayed samples, and (delay, w_index, f_index).  The per-sample calls
// run on a host mirror (host.cpp: host_fir_window_dot, the bank's own sum); block and track calls run
// fdelay_kernels.hip on the device copy, whose state launch writes the other of two buffers.  The two copies are
// synchronised lazily (DevWindow's pattern).  After a device track the delay in force is known to the device only:
// the state launch stores it behind the histories and the host fetches those four bytes when it next needs the lag.
namespace yagi {

// set_delay :72-97 in f32
static int fdelay_lag(float d, int nmax, int npfb, int *w, int *f) {
    if (d < 0.0f) return fail(YAGI_ERR_CONFIG, "delay cannot be negative");
    if (!(d <= (float)nmax)) return fail(YAGI_ERR_CONFIG, "delay (%g) cannot exceed maximum (%d)", (double)d, nmax);
    const float offset = (float)nmax - d;
    const float ip = std::floor(offset);
    const float frac = offset - ip;
    int wi = (int)ip, fi = (int)std::round((float)npfb * frac);
    while (fi >= npfb) { ++wi; fi -= npfb; }
    if (wi > nmax) return fail(YAGI_ERR_INTERNAL, "window index exceeds maximum");
    *w = wi;
    *f = fi;
    return YAGI_OK;
}

// the last len values of a stream on the host, oldest first; slack behind them so that a push appends
template <class T>
struct FdHist {
    static constexpr size_t kSlack = 4096;
    std::vector<T> buf;
    size_t end = 0, len = 0;
    void init(size_t n) { len = n; buf.assign(n + kSlack, T{}); end = n; }
    void zero() { std::fill(buf.begin(), buf.begin() + len, T{}); end = len; }
    T *data() { return buf.data() + (end - len); }
    void load(const T *src) { std::memcpy(buf.data(), src, len * sizeof(T)); end = len; }
    void push(T v) {
        if (end == buf.size()) {
            std::memmove(buf.data(), data() + 1, (len - 1) * sizeof(T));
            end = len - 1;
        }
        buf[end++] = v;
    }
};

template <class K>
struct FdelayObj {
    using T = typename K::T;
    using C = typename K::C;
    hipStream_t st = nullptr;
    int nmax = 0, m = 0, npfb = 0, Ls = 0;
    float delay = 0.0f;
    int w_index = 0, f_index = 0;
    bool lag_on_dev = false;             // a device track ran last: (delay, w, f) are behind the device histories
    std::vector<C> hb;                   // [npfb][Ls], natural order: hb[i][k] = h[i + k npfb]
    C scale = one_of<C>();
    DevBuf taps;                         // [npfb][Ls] against the window oldest first
    PingPong<> state;                    // [nmax X][Ls V][delay]
    FdHist<T> hx, hv;                    // host mirror of the two histories
    Staging ws;
    DevBuf wd;                           // host track form: the delays on the device
    Mirror mirror;

    size_t state_bytes() const { return fdelay_state_bytes<T>(nmax, Ls); }
    size_t lag_offset() const { return ((size_t)nmax + (size_t)Ls) * sizeof(T); }
    FdelayDims dims() const { return FdelayDims{nmax, Ls, npfb}; }

    int alloc_dev() {
        std::vector<C> hd(hb.size());
        for (int i = 0; i < npfb; ++i)
            for (int k = 0; k < Ls; ++k) hd[(size_t)i * Ls + k] = hb[(size_t)i * Ls + (Ls - 1 - k)];
        YG_TRY(fill(taps, hd.data(), hd.size() * sizeof(C), st));
        return state.alloc(state_bytes());
    }
    int init(size_t nmax_, size_t m_, size_t npfb_) {                        // new() :26-53
        if (nmax_ == 0) return fail(YAGI_ERR_CONFIG, "maximum delay must be greater than zero");
        if (m_ == 0) return fail(YAGI_ERR_CONFIG, "filter semi-length must be greater than zero");
        if (npfb_ == 0) return fail(YAGI_ERR_CONFIG, "number of filters must be greater than zero");
        if (nmax_ > (size_t)1 << 24)                                         // set_delay's f32 steps are exact up to here
            return fail(YAGI_ERR_CONFIG, "maximum delay too large");
        if (npfb_ > (size_t)1 << 20 || m_ > (size_t)kFdMaxLs || 2 * npfb_ * m_ + 1 > (size_t)1 << 24)
            return fail(YAGI_ERR_CONFIG, "filter bank too large");
        const size_t h_len = 2 * npfb_ * m_ + 1;                             // FirPfbFilter::default(npfb, m)
        if (h_len / npfb_ > (size_t)kFdMaxLs) return fail(YAGI_ERR_CONFIG, "filter bank too large");
        YG_TRY(require_device());
        std::vector<float> hf;
        YG_TRY(design_kaiser(h_len, 0.5f / (float)npfb_, 60.0f, 0.0f, hf));
        nmax = (int)nmax_;
        m = (int)m_;
        npfb = (int)npfb_;
        Ls = (int)(h_len / npfb_);                                           // firpfb.rs:42: 2m, and 2m + 1 for npfb = 1
        hb.resize((size_t)npfb * Ls);
        for (int i = 0; i < npfb; ++i)
            for (int k = 0; k < Ls; ++k) hb[(size_t)i * Ls + k] = to_c(hf[i + (size_t)k * npfb], (C *)nullptr);
        YG_TRY(alloc_dev());
        hx.init((size_t)nmax);
        hv.init((size_t)Ls);
        return reset();
    }
    int reset() {                                                            // :59-65
        delay = 0.0f;
        w_index = nmax - 1;
        f_index = 0;
        lag_on_dev = false;
        hx.zero();
        hv.zero();
        YG_HIP(hipMemsetAsync(state.cur(), 0, state_bytes(), st));
        mirror.in_sync();
        return YAGI_OK;
    }
    // (delay, w, f) after a device track: the four bytes the state launch left behind the histories
    int sync_lag() {
        if (!lag_on_dev) return YAGI_OK;
        float d = 0.0f;
        YG_TRY(download(&d, state.cur<char>() + lag_offset(), sizeof(float), st));
        YG_TRY(fdelay_lag(d, nmax, npfb, &w_index, &f_index));
        delay = d;
        lag_on_dev = false;
        return YAGI_OK;
    }
    int ensure_host() {
        YG_TRY(sync_lag());
        return mirror.need_host([&] {
            std::vector<T> tmp((size_t)nmax + Ls);
            YG_TRY(download(tmp.data(), state.cur(), tmp.size() * sizeof(T), st));
            hx.load(tmp.data());
            hv.load(tmp.data() + nmax);
            return (int)YAGI_OK;
        });
    }
    int ensure_dev() {
        return mirror.need_dev([&] {
            std::vector<T> tmp((size_t)nmax + Ls + 1, T{});
            std::memcpy(tmp.data(), hx.data(), (size_t)nmax * sizeof(T));
            std::memcpy(tmp.data() + nmax, hv.data(), (size_t)Ls * sizeof(T));
            std::memcpy(tmp.data() + nmax + Ls, &delay, sizeof(float));
            return upload(state.cur(), tmp.data(), state_bytes(), st);
        });
    }
    int enter_host() {
        YG_TRY(ensure_host());
        mirror.host_written();
        return YAGI_OK;
    }
    int set_delay(float d) {                                                 // :71-97
        int w, f;
        YG_TRY(fdelay_lag(d, nmax, npfb, &w, &f));
        w_index = w;
        f_index = f;
        delay = d;
        lag_on_dev = false;
        return YAGI_OK;
    }
    void push(T x) {                                                         // :115-118 (after enter_host)
        const int D = nmax - w_index;
        const T v = D == 0 ? x : hx.data()[nmax - D];
        hx.push(x);
        hv.push(v);
    }
    T execute() {                                                            // :126-128
        return host_fir_window_dot<T, C>(hv.data(), (size_t)Ls, hb.data() + (size_t)f_index * Ls, scale);
    }
    int block_dev(const T *x, size_t n, T *y) {
        if (n == 0) return YAGI_OK;
        YG_TRY(sync_lag());
        YG_TRY(ensure_dev());
        YG_TRY((launch_fdelay<K>(dims(), taps.template as<C>(), scale, state.template cur<T>(), state.template next<T>(),
                                 nmax - w_index, f_index, delay, nullptr, x, n, y, st)));
        state.flip();
        mirror.dev_written();
        return YAGI_OK;
    }
    int track_dev(const float *d, const T *x, size_t n, T *y) {
        if (n == 0) return YAGI_OK;
        YG_TRY(ensure_dev());
        YG_TRY((launch_fdelay<K>(dims(), taps.template as<C>(), scale, state.template cur<T>(), state.template next<T>(),
                                 0, 0, delay, d, x, n, y, st)));
        state.flip();
        mirror.dev_written();
        lag_on_dev = true;
        return YAGI_OK;
    }
    int track_host(const float *d, const T *x, size_t n, T *y) {
        if (n == 0) return YAGI_OK;
        int w = 0, f = 0;
        for (size_t i = 0; i < n; ++i) YG_TRY(fdelay_lag(d[i], nmax, npfb, &w, &f));   // all of it, before any state moves
        YG_TRY(wd.ensure(n * sizeof(float)));
        YG_TRY(upload(wd.p, d, n * sizeof(float), st));
        YG_TRY(ws.run(st, x, n, y, n, [&](const T *xd, T *yd) { return track_dev(wd.as<float>(), xd, n, yd); }));
        w_index = w;
        f_index = f;
        delay = d[n - 1];
        lag_on_dev = false;
        return YAGI_OK;
    }
};

}  // namespace yagi

#define YAGI_FDELAY_IMPL(K, KT, T)                                                                  \
    struct yagi_hip_fdelay_##K##_s : FdelayObj<KT> {};                                              \
    extern "C" {                                                                                    \
    int yagi_hip_fdelay_##K##_create(size_t nmax, size_t m, size_t npfb, yagi_hip_fdelay_##K *q) try { \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        auto o = std::make_unique<yagi_hip_fdelay_##K##_s>();                                       \
        YG_TRY(o->init(nmax, m, npfb));                                                             \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_create_default(size_t nmax, yagi_hip_fdelay_##K *q) try {             \
        return yagi_hip_fdelay_##K##_create(nmax, 8, 64, q);                                        \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_destroy(yagi_hip_fdelay_##K q) try {                                  \
        if (q) (void)hipStreamSynchronize(q->st);                                                   \
        delete q;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_clone(yagi_hip_fdelay_##K q, yagi_hip_fdelay_##K *out) try {          \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        YG_TRY(q->ensure_host());                                                                   \
        auto o = std::make_unique<yagi_hip_fdelay_##K##_s>();                                       \
        o->st = q->st;                                                                              \
        o->nmax = q->nmax;                                                                          \
        o->m = q->m;                                                                                \
        o->npfb = q->npfb;                                                                          \
        o->Ls = q->Ls;                                                                              \
        o->delay = q->delay;                                                                        \
        o->w_index = q->w_index;                                                                    \
        o->f_index = q->f_index;                                                                    \
        o->hb = q->hb;                                                                              \
        o->scale = q->scale;                                                                        \
        YG_TRY(o->alloc_dev());                                                                     \
        o->hx.init((size_t)o->nmax);                                                                \
        o->hv.init((size_t)o->Ls);                                                                  \
        o->hx.load(q->hx.data());                                                                   \
        o->hv.load(q->hv.data());                                                                   \
        o->mirror.host_written();                                                                   \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_set_stream(yagi_hip_fdelay_##K q, yagi_stream_t s) try {              \
        CHECK_Q(q);                                                                                 \
        if (q->st == to_stream(s)) return YAGI_OK;                                                  \
        YG_HIP(hipStreamSynchronize(q->st));                                                        \
        q->st = to_stream(s);                                                                       \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_reset(yagi_hip_fdelay_##K q) try {                                    \
        CHECK_Q(q);                                                                                 \
        return q->reset();                                                                          \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_get_delay(yagi_hip_fdelay_##K q, float *delay) try {                  \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(delay);                                                                           \
        YG_TRY(q->sync_lag());                                                                      \
        *delay = q->delay;                                                                          \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_set_delay(yagi_hip_fdelay_##K q, float delay) try {                   \
        CHECK_Q(q);                                                                                 \
        return q->set_delay(delay);                                                                 \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_adjust_delay(yagi_hip_fdelay_##K q, float delta) try {                \
        CHECK_Q(q);                                                                                 \
        YG_TRY(q->sync_lag());                                                                      \
        return q->set_delay(q->delay + delta);                                                      \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_get_nmax(yagi_hip_fdelay_##K q, size_t *nmax) try {                   \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(nmax);                                                                            \
        *nmax = (size_t)q->nmax;                                                                    \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_get_m(yagi_hip_fdelay_##K q, size_t *m) try {                         \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(m);                                                                               \
        *m = (size_t)q->m;                                                                          \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_get_npfb(yagi_hip_fdelay_##K q, size_t *npfb) try {                   \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(npfb);                                                                            \
        *npfb = (size_t)q->npfb;                                                                    \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_push(yagi_hip_fdelay_##K q, T x) try {                                \
        CHECK_Q(q);                                                                                 \
        YG_TRY(q->enter_host());                                                                    \
        q->push(x);                                                                                 \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_write(yagi_hip_fdelay_##K q, const T *x, size_t n) try {              \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        YG_TRY(q->enter_host());                                                                    \
        for (size_t i = 0; i < n; ++i) q->push(x[i]);                                               \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_execute(yagi_hip_fdelay_##K q, T *y) try {                            \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(y);                                                                               \
        YG_TRY(q->ensure_host());                                                                   \
        *y = q->execute();                                                                          \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_execute_block(yagi_hip_fdelay_##K q, const T *x, size_t nx, T *y,     \
                                            size_t ny) try {                                        \
        CHECK_Q(q);                                                                                 \
        const size_t n = nx < ny ? nx : ny;       /* zip() stops at the shorter slice (:131) */     \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        return q->ws.run(q->st, x, n, y, n, [&](const T *xd, T *yd) { return q->block_dev(xd, n, yd); }); \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_execute_block_dev(yagi_hip_fdelay_##K q, const T *x_dev, size_t n,    \
                                                T *y_dev) try {                                     \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x_dev);                                                                           \
        CHECK_PTR(y_dev);                                                                           \
        CHECK_NOALIAS(x_dev, n, y_dev, n);                                                          \
        return q->block_dev(x_dev, n, y_dev);                                                       \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_execute_track(yagi_hip_fdelay_##K q, const float *delay, const T *x,  \
                                            size_t n, T *y) try {                                   \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(delay);                                                                           \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(y);                                                                               \
        return q->track_host(delay, x, n, y);                                                       \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_fdelay_##K##_execute_track_dev(yagi_hip_fdelay_##K q, const float *delay_dev,      \
                                                const T *x_dev, size_t n, T *y_dev) try {           \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(delay_dev);                                                                       \
        CHECK_PTR(x_dev);                                                                           \
        CHECK_PTR(y_dev);                                                                           \
        CHECK_NOALIAS(x_dev, n, y_dev, n);                                                          \
        CHECK_NOALIAS(delay_dev, n, y_dev, n);                                                      \
        return q->track_dev(delay_dev, x_dev, n, y_dev);                                            \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_FDELAY_IMPL(rrrf, RRRF, float)
YAGI_FDELAY_IMPL(crcf, CRCF, yagi_cf32)
YAGI_FDELAY_IMPL(cccf, CCCF, yagi_cf32)

// ---- Modem (src/modem/modem.rs) ------------------------------------------------------------------------------------
// Construction, the per-sample arithmetic and the kernels are modem_kernels.hip (the file built with contraction off);
// this is the object: the tables on both sides, and one ModemState (r, x_hat, DPSK's demodulator phase and modulator
// index) as a host mirror and a device copy that the kernels rewrite into the other of two buffers.  The two copies
// are synchronised lazily (Mirror), so per-sample and block calls mix freely.
struct yagi_hip_modem_s {
    hipStream_t st = nullptr;
    int scheme = 0;
    ModemParams P{};
    std::vector<cf32> map;
    std::vector<uint8_t> nbr;
    ModemState hs{};                      // host mirror
    DevBuf dmap, dnbr, partials, flag;
    PingPong<> state;
    Staging ws;                           // host-pointer block calls: x / symbols in, the first output out
    DevBuf w2;                            // their second output (xhat, soft bits)
    Mirror mirror;

    static int kind_of(int scheme, int *kind, int *bps) {
        if (scheme >= YAGI_MODEM_PSK2 && scheme <= YAGI_MODEM_PSK256) return *kind = MODEM_PSK, *bps = scheme - YAGI_MODEM_PSK2 + 1, YAGI_OK;
        if (scheme >= YAGI_MODEM_DPSK2 && scheme <= YAGI_MODEM_DPSK256) return *kind = MODEM_DPSK, *bps = scheme - YAGI_MODEM_DPSK2 + 1, YAGI_OK;
        if (scheme >= YAGI_MODEM_ASK2 && scheme <= YAGI_MODEM_ASK256) return *kind = MODEM_ASK, *bps = scheme - YAGI_MODEM_ASK2 + 1, YAGI_OK;
        if (scheme >= YAGI_MODEM_QAM4 && scheme <= YAGI_MODEM_QAM256) return *kind = MODEM_QAM, *bps = scheme - YAGI_MODEM_QAM4 + 2, YAGI_OK;
        if (scheme == YAGI_MODEM_BPSK) return *kind = MODEM_BPSK, *bps = 1, YAGI_OK;
        if (scheme == YAGI_MODEM_QPSK) return *kind = MODEM_QPSK, *bps = 2, YAGI_OK;
        if (scheme == YAGI_MODEM_OOK) return *kind = MODEM_OOK, *bps = 1, YAGI_OK;
        if (scheme == YAGI_MODEM_ARB) return fail(YAGI_ERR_CONFIG, "modem: an arbitrary constellation needs create_from_table");
        if (scheme > YAGI_MODEM_UNKNOWN && scheme < YAGI_MODEM_ARB)
            return fail(YAGI_ERR_CONFIG, "modem: scheme %d is not built (its constellation is not part of this library)", scheme);
        return fail(YAGI_ERR_CONFIG, "modulation scheme not supported");
    }
    int alloc_dev() {
        YG_TRY(fill(dmap, map.data(), map.size() * sizeof(cf32), st));
        YG_TRY(fill(dnbr, nbr.data(), nbr.size(), st));
        YG_TRY(flag.alloc(sizeof(int)));
        return state.alloc(sizeof(ModemState));
    }
    int init(int scheme_, int kind, int bps, const cf32 *table) {
        YG_TRY(modem_design(kind, bps, table, P, map, nbr));
        YG_TRY(require_device());
        scheme = scheme_;
        YG_TRY(alloc_dev());
        return reset();
    }
    int reset() {                                                            // :218-224
        hs = ModemState{cf32{1.0f, 0.0f}, cf32{1.0f, 0.0f}, 0.0f, 0u};
        mirror.in_sync();
        mirror.host_written();
        return YAGI_OK;
    }
    int ensure_host() {
        return mirror.need_host([&] { return download(&hs, state.cur(), sizeof(ModemState), st); });
    }
    int ensure_dev() {
        return mirror.need_dev([&] { return upload(state.cur(), &hs, sizeof(ModemState), st); });
    }
    int enter_host() {
        YG_TRY(ensure_host());
        mirror.host_written();
        return YAGI_OK;
    }
    int modulate(unsigned sym, cf32 *y) {                                    // :243-253
        if (sym >= (unsigned)P.M) return fail(YAGI_ERR_RANGE, "input symbol exceeds constellation size");
        if (P.kind == MODEM_DPSK) {
            YG_TRY(enter_host());
            hs.k = modem_host_modulate_dpsk(P, sym, hs.k);
            *y = hs.r = map[hs.k];
        } else {
            *y = map[sym];
        }
        return YAGI_OK;
    }
    int demodulate(cf32 x, unsigned *sym, uint8_t *soft) {
        YG_TRY(enter_host());
        *sym = modem_host_demod(P, map.data(), nbr.data(), x, hs, soft);
        return YAGI_OK;
    }
    int modulate_dev(const uint8_t *sym, size_t n, cf32 *y) {
        if (n == 0) return YAGI_OK;
        const bool dpsk = P.kind == MODEM_DPSK;
        if (dpsk) {
            YG_TRY(ensure_dev());
            YG_TRY(partials.ensure(modem_num_partials(n) * sizeof(unsigned)));
        }
        YG_TRY(launch_modem_modulate(P, dmap.as<cf32>(), state.cur<ModemState>(), state.next<ModemState>(), sym, n, y,
                                     partials.as<unsigned>(), flag.as<int>(), st));
        int bad = 0;
        YG_TRY(download(&bad, flag.p, sizeof(int), st));
        if (bad) return fail(YAGI_ERR_RANGE, "input symbol exceeds constellation size");
        if (dpsk) {
            state.flip();
            mirror.dev_written();
        }
        return YAGI_OK;
    }
    int demodulate_dev(const cf32 *x, size_t n, uint8_t *sym, cf32 *xhat, uint8_t *soft) {
        if (n == 0) return YAGI_OK;
        YG_TRY(ensure_dev());
        YG_TRY(launch_modem_demod(P, dmap.as<cf32>(), dnbr.as<uint8_t>(), state.cur<ModemState>(), state.next<ModemState>(),
                                  x, n, sym, xhat, soft, st));
        state.flip();
        mirror.dev_written();
        return YAGI_OK;
    }
    // host slices: x through the staging pair, the second output through w2
    int demodulate_host(const cf32 *x, size_t n, uint8_t *sym, cf32 *xhat, uint8_t *soft) {
        if (n == 0) return YAGI_OK;
        const size_t b2 = xhat ? n * sizeof(cf32) : soft ? n * (size_t)P.bps : 0;
        YG_TRY(ws.put(st, x, n));
        YG_TRY(ws.y.ensure(n));
        if (b2) YG_TRY(w2.ensure(b2));
        YG_TRY(demodulate_dev(ws.x.as<cf32>(), n, ws.y.as<uint8_t>(), xhat ? w2.as<cf32>() : nullptr,
                              soft ? w2.as<uint8_t>() : nullptr));
        YG_TRY(download(sym, ws.y.p, n, st));
        if (b2) YG_TRY(download(xhat ? (void *)xhat : (void *)soft, w2.p, b2, st));
        return YAGI_OK;
    }
};

#define MODEM_CREATE(...)                                                                           \
    CHECK_PTR(q);                                                                                   \
    *q = nullptr;                                                                                   \
    auto o = std::make_unique<yagi_hip_modem_s>();                                                  \
    YG_TRY(o->init(__VA_ARGS__));                                                                   \
    *q = o.release();                                                                               \
    return YAGI_OK

extern "C" {

int yagi_hip_modem_create(int scheme, yagi_hip_modem *q) try {
    int kind = 0, bps = 0;
    YG_TRY(yagi_hip_modem_s::kind_of(scheme, &kind, &bps));
    MODEM_CREATE(scheme, kind, bps, nullptr);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_create_from_table(const yagi_cf32 *table, size_t n, yagi_hip_modem *q) try {
    CHECK_PTR(table);
    int bps = 0;
    while (bps < 8 && ((size_t)1 << bps) < n) ++bps;
    if (n < 2 || ((size_t)1 << bps) != n) return fail(YAGI_ERR_CONFIG, "table size must be a power of 2 in 2..256");
    MODEM_CREATE(YAGI_MODEM_ARB, MODEM_ARB, bps, table);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_destroy(yagi_hip_modem q) try {
    if (q) (void)hipStreamSynchronize(q->st);
    delete q;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_clone(yagi_hip_modem q, yagi_hip_modem *out) try {
    CHECK_Q(q);
    CHECK_PTR(out);
    *out = nullptr;
    YG_TRY(q->ensure_host());
    auto o = std::make_unique<yagi_hip_modem_s>();
    o->st = q->st;
    o->scheme = q->scheme;
    o->P = q->P;
    o->map = q->map;
    o->nbr = q->nbr;
    o->hs = q->hs;
    YG_TRY(o->alloc_dev());
    o->mirror.host_written();
    *out = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_set_stream(yagi_hip_modem q, yagi_stream_t s) try {
    CHECK_Q(q);
    if (q->st == to_stream(s)) return YAGI_OK;
    YG_HIP(hipStreamSynchronize(q->st));
    q->st = to_stream(s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_reset(yagi_hip_modem q) try {
    CHECK_Q(q);
    return q->reset();
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_get_bps(yagi_hip_modem q, size_t *bps) try {
    CHECK_Q(q);
    CHECK_PTR(bps);
    *bps = (size_t)q->P.bps;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_get_scheme(yagi_hip_modem q, int *scheme) try {
    CHECK_Q(q);
    CHECK_PTR(scheme);
    *scheme = q->scheme;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_get_constellation_size(yagi_hip_modem q, size_t *m) try {
    CHECK_Q(q);
    CHECK_PTR(m);
    *m = (size_t)q->P.M;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_get_constellation(yagi_hip_modem q, yagi_cf32 *map) try {
    CHECK_Q(q);
    CHECK_PTR(map);
    std::memcpy(map, q->map.data(), q->map.size() * sizeof(cf32));
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_get_neighbours(yagi_hip_modem q, uint8_t *nbr, size_t cap, size_t *p) try {
    CHECK_Q(q);
    CHECK_PTR(p);
    *p = (size_t)q->P.p;
    if (!nbr) return YAGI_OK;
    if (cap < q->nbr.size()) return fail(YAGI_ERR_RANGE, "neighbour table needs %zu bytes", q->nbr.size());
    if (!q->nbr.empty()) std::memcpy(nbr, q->nbr.data(), q->nbr.size());
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_modulate(yagi_hip_modem q, unsigned sym, yagi_cf32 *y) try {
    CHECK_Q(q);
    CHECK_PTR(y);
    return q->modulate(sym, y);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_demodulate(yagi_hip_modem q, yagi_cf32 x, unsigned *sym) try {
    CHECK_Q(q);
    CHECK_PTR(sym);
    return q->demodulate(x, sym, nullptr);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_demodulate_soft(yagi_hip_modem q, yagi_cf32 x, unsigned *sym, uint8_t *soft) try {
    CHECK_Q(q);
    CHECK_PTR(sym);
    CHECK_PTR(soft);
    return q->demodulate(x, sym, soft);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_get_demodulator_sample(yagi_hip_modem q, yagi_cf32 *x_hat) try {             // :273-275
    CHECK_Q(q);
    CHECK_PTR(x_hat);
    YG_TRY(q->ensure_host());
    *x_hat = q->hs.x_hat;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_get_demodulator_phase_error(yagi_hip_modem q, float *e) try {                // :277-279
    CHECK_Q(q);
    CHECK_PTR(e);
    YG_TRY(q->ensure_host());
    const std::complex<float> r(q->hs.r.re, q->hs.r.im), xh(q->hs.x_hat.re, -q->hs.x_hat.im);
    *e = r.real() * xh.imag() + r.imag() * xh.real();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_get_demodulator_evm(yagi_hip_modem q, float *evm) try {                      // :281-283
    CHECK_Q(q);
    CHECK_PTR(evm);
    YG_TRY(q->ensure_host());
    *evm = std::hypot(q->hs.x_hat.re - q->hs.r.re, q->hs.x_hat.im - q->hs.r.im);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_modulate_block(yagi_hip_modem q, const uint8_t *sym, size_t n, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(sym);
    CHECK_PTR(y);
    for (size_t i = 0; i < n; ++i)
        if ((int)sym[i] >= q->P.M) return fail(YAGI_ERR_RANGE, "input symbol %zu exceeds constellation size", i);
    YG_TRY(q->ws.put(q->st, sym, n));
    YG_TRY(q->ws.y.ensure(n * sizeof(cf32)));
    YG_TRY(q->modulate_dev(q->ws.x.as<uint8_t>(), n, q->ws.y.as<cf32>()));
    return download(y, q->ws.y.p, n * sizeof(cf32), q->st);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_modulate_block_dev(yagi_hip_modem q, const uint8_t *sym_dev, size_t n, yagi_cf32 *y_dev) try {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(sym_dev);
    CHECK_PTR(y_dev);
    CHECK_NOALIAS(sym_dev, n, y_dev, n);
    return q->modulate_dev(sym_dev, n, y_dev);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_demodulate_block(yagi_hip_modem q, const yagi_cf32 *x, size_t n, uint8_t *sym, yagi_cf32 *xhat) try {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(sym);
    return q->demodulate_host(x, n, sym, xhat, nullptr);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_demodulate_block_dev(yagi_hip_modem q, const yagi_cf32 *x_dev, size_t n, uint8_t *sym_dev,
                                        yagi_cf32 *xhat_dev) try {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x_dev);
    CHECK_PTR(sym_dev);
    CHECK_NOALIAS(x_dev, n, sym_dev, n);
    if (xhat_dev) {
        CHECK_NOALIAS(x_dev, n, xhat_dev, n);
        CHECK_NOALIAS(sym_dev, n, xhat_dev, n);
    }
    return q->demodulate_dev(x_dev, n, sym_dev, xhat_dev, nullptr);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_demodulate_soft_block(yagi_hip_modem q, const yagi_cf32 *x, size_t n, uint8_t *sym, uint8_t *soft) try {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(sym);
    CHECK_PTR(soft);
    return q->demodulate_host(x, n, sym, nullptr, soft);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_modem_demodulate_soft_block_dev(yagi_hip_modem q, const yagi_cf32 *x_dev, size_t n, uint8_t *sym_dev,
                                             uint8_t *soft_dev) try {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x_dev);
    CHECK_PTR(sym_dev);
    CHECK_PTR(soft_dev);
    const size_t ns = n * (size_t)q->P.bps;
    CHECK_NOALIAS(x_dev, n, sym_dev, n);
    CHECK_NOALIAS(x_dev, n, soft_dev, ns);
    CHECK_NOALIAS(sym_dev, n, soft_dev, ns);
    return q->demodulate_dev(x_dev, n, sym_dev, nullptr, soft_dev);
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- OrdFilt (src/filter/ordfilt.rs) -------------------------------------------------------------------------------
// The state is the reference's Window: the last n samples, oldest first.  The per-sample calls run on a host mirror
// (ordfilt_host_select: a stable sort of a copy under the key order); block calls run ordfilt_kernels.hip on the device
// copy, whose launch writes the window it leaves into the other of two buffers.  The two copies are synchronised lazily
// (Mirror).  The kernel needs only the newest n - 1 samples; the device keeps all n so that an execute() right after a
// block call sees the reference's window.
struct yagi_hip_ordfilt_rrrf_s {
    hipStream_t st = nullptr;
    int n = 0, k = 0;
    int form = yagi::ORDFILT_AUTO;                        // set_kernel
    yagi::FdHist<float> win;                              // host mirror
    yagi::PingPong<> hist;                                // device copy, n floats
    yagi::Staging ws;
    yagi::Mirror mirror;
    std::vector<std::pair<unsigned, unsigned>> tmp;       // execute()'s sorted copy

    size_t bytes() const { return (size_t)n * sizeof(float); }
    int init(size_t n_, size_t k_) {                                         // new() :16-30
        if (n_ == 0) return yagi::fail(YAGI_ERR_CONFIG, "filter length must be greater than zero");
        if (k_ >= n_) return yagi::fail(YAGI_ERR_CONFIG, "filter index must be in [0,n-1]");
        if (n_ > (size_t)YAGI_ORDFILT_NMAX)
            return yagi::fail(YAGI_ERR_CONFIG, "filter length %zu exceeds YAGI_ORDFILT_NMAX = %d", n_, YAGI_ORDFILT_NMAX);
        YG_TRY(yagi::require_device());
        n = (int)n_;
        k = (int)k_;
        YG_TRY(hist.alloc(bytes()));
        win.init((size_t)n);
        return reset();
    }
    int reset() {                                                            // :36-38
        win.zero();
        YG_HIP(hipMemsetAsync(hist.cur(), 0, bytes(), st));
        mirror.in_sync();
        return YAGI_OK;
    }
    int ensure_host() {
        return mirror.need_host([&] {
            std::vector<float> t((size_t)n);
            YG_TRY(yagi::download(t.data(), hist.cur(), bytes(), st));
            win.load(t.data());
            return (int)YAGI_OK;
        });
    }
    int ensure_dev() {
        return mirror.need_dev([&] { return yagi::upload(hist.cur(), win.data(), bytes(), st); });
    }
    int enter_host() {
        YG_TRY(ensure_host());
        mirror.host_written();
        return YAGI_OK;
    }
    float execute() { return yagi::ordfilt_host_select(win.data(), n, k, tmp); }        // :48-53 (after ensure_host)
    int block_dev(const float *x, size_t nb, float *y) {
        if (nb == 0) return YAGI_OK;
        YG_TRY(ensure_dev());
        YG_TRY(yagi::launch_ordfilt(n, k, form, hist.cur<float>(), hist.next<float>(), x, nb, y, st));
        hist.flip();
        mirror.dev_written();
        return YAGI_OK;
    }
};

extern "C" {

int yagi_hip_ordfilt_rrrf_create(size_t n, size_t k, yagi_hip_ordfilt_rrrf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    auto o = std::make_unique<yagi_hip_ordfilt_rrrf_s>();
    YG_TRY(o->init(n, k));
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_ordfilt_rrrf_create_medfilt(size_t m, yagi_hip_ordfilt_rrrf *q) try {    // new_medfilt() :32-34
    if (m > (size_t)YAGI_ORDFILT_NMAX) return yagi_hip_ordfilt_rrrf_create((size_t)YAGI_ORDFILT_NMAX + 1, 0, q);
    return yagi_hip_ordfilt_rrrf_create(2 * m + 1, m, q);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_ordfilt_rrrf_destroy(yagi_hip_ordfilt_rrrf q) try {
    if (q) (void)hipStreamSynchronize(q->st);
    delete q;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_ordfilt_rrrf_clone(yagi_hip_ordfilt_rrrf q, yagi_hip_ordfilt_rrrf *out) try {
    CHECK_Q(q);
    CHECK_PTR(out);
    *out = nullptr;
    YG_TRY(q->ensure_host());
    auto o = std::make_unique<yagi_hip_ordfilt_rrrf_s>();
    o->st = q->st;
    o->n = q->n;
    o->k = q->k;
    o->form = q->form;
    YG_TRY(o->hist.alloc(o->bytes()));
    o->win.init((size_t)o->n);
    o->win.load(q->win.data());
    o->mirror.host_written();
    *out = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_ordfilt_rrrf_set_stream(yagi_hip_ordfilt_rrrf q, yagi_stream_t s) try {
    CHECK_Q(q);
    if (q->st == to_stream(s)) return YAGI_OK;
    YG_HIP(hipStreamSynchronize(q->st));
    q->st = to_stream(s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
// which kernel the block calls run: 0 auto, 1 the LDS form, 2 the register form (2 <= n <= YAGI_ORDFILT_REG_NMAX)
int yagi_hip_ordfilt_rrrf_set_kernel(yagi_hip_ordfilt_rrrf q, int choice) try {
    CHECK_Q(q);
    if (choice < yagi::ORDFILT_AUTO || choice > yagi::ORDFILT_REG) return fail(YAGI_ERR_CONFIG, "unknown kernel choice %d", choice);
    if (choice == yagi::ORDFILT_REG && (q->n < 2 || q->n > YAGI_ORDFILT_REG_NMAX))
        return fail(YAGI_ERR_CONFIG, "the register form needs 2 <= n <= %d", YAGI_ORDFILT_REG_NMAX);
    q->form = choice;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_ordfilt_rrrf_reset(yagi_hip_ordfilt_rrrf q) try {
    CHECK_Q(q);
    return q->reset();
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_ordfilt_rrrf_get_n(yagi_hip_ordfilt_rrrf q, size_t *n) try {
    CHECK_Q(q);
    CHECK_PTR(n);
    *n = (size_t)q->n;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_ordfilt_rrrf_get_k(yagi_hip_ordfilt_rrrf q, size_t *k) try {
    CHECK_Q(q);
    CHECK_PTR(k);
    *k = (size_t)q->k;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_ordfilt_rrrf_push(yagi_hip_ordfilt_rrrf q, float x) try {               // :40-42
    CHECK_Q(q);
    YG_TRY(q->enter_host());
    q->win.push(x);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_ordfilt_rrrf_write(yagi_hip_ordfilt_rrrf q, const float *x, size_t n) try {   // :44-46
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x);
    YG_TRY(q->enter_host());
    for (size_t i = 0; i < n; ++i) q->win.push(x[i]);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_ordfilt_rrrf_execute(yagi_hip_ordfilt_rrrf q, float *y) try {            // :48-53
    CHECK_Q(q);
    CHECK_PTR(y);
    YG_TRY(q->ensure_host());
    *y = q->execute();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_ordfilt_rrrf_execute_one(yagi_hip_ordfilt_rrrf q, float x, float *y) try {    // :55-58
    CHECK_Q(q);
    CHECK_PTR(y);
    YG_TRY(q->enter_host());
    q->win.push(x);
    *y = q->execute();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_ordfilt_rrrf_execute_block(yagi_hip_ordfilt_rrrf q, const float *x, size_t n, float *y) try {   // :60-65
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(y);
    return q->ws.run(q->st, x, n, y, n, [&](const float *xd, float *yd) { return q->block_dev(xd, n, yd); });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_ordfilt_rrrf_execute_block_dev(yagi_hip_ordfilt_rrrf q, const float *x_dev, size_t n, float *y_dev) try {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x_dev);
    CHECK_PTR(y_dev);
    CHECK_NOALIAS(x_dev, n, y_dev, n);
    return q->block_dev(x_dev, n, y_dev);
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- Autocorr (yagi_hip.h; src/filter/autocorr.rs is empty) ---------------------------------------------------------
// The state is the last W + d samples, oldest first: the window w is its newest W, and conj of its oldest W is v.  The
// per-sample calls run on a host mirror (autocorr_host, the kernel's arithmetic); block calls run autocorr_kernels.hip on
// the device copy, whose launch writes the history it leaves into the other of two buffers.  The two copies are
// synchronised lazily (Mirror).
namespace yagi {

template <class T>
struct AutocorrObj {
    hipStream_t st = nullptr;
    int W = 0, d = 0;
    FdHist<T> win;                                        // host mirror
    PingPong<> hist;                                      // device copy, W + d samples
    Staging ws;
    DevBuf we;                                            // host block form: the energies on the device
    Mirror mirror;

    size_t len() const { return (size_t)W + (size_t)d; }
    size_t bytes() const { return len() * sizeof(T); }
    int init(size_t W_, size_t d_) {
        if (W_ == 0) return fail(YAGI_ERR_CONFIG, "window size must be greater than zero");
        if (W_ > (size_t)YAGI_AUTOCORR_WMAX)
            return fail(YAGI_ERR_CONFIG, "window size %zu exceeds YAGI_AUTOCORR_WMAX = %d", W_, YAGI_AUTOCORR_WMAX);
        if (d_ > (size_t)YAGI_AUTOCORR_DMAX)
            return fail(YAGI_ERR_CONFIG, "delay %zu exceeds YAGI_AUTOCORR_DMAX = %d", d_, YAGI_AUTOCORR_DMAX);
        YG_TRY(require_device());
        W = (int)W_;
        d = (int)d_;
        YG_TRY(hist.alloc(bytes()));
        win.init(len());
        return reset();
    }
    int reset() {
        win.zero();
        YG_HIP(hipMemsetAsync(hist.cur(), 0, bytes(), st));
        mirror.in_sync();
        return YAGI_OK;
    }
    int ensure_host() {
        return mirror.need_host([&] {
            std::vector<T> t(len());
            YG_TRY(download(t.data(), hist.cur(), bytes(), st));
            win.load(t.data());
            return (int)YAGI_OK;
        });
    }
    int ensure_dev() {
        return mirror.need_dev([&] { return upload(hist.cur(), win.data(), bytes(), st); });
    }
    int enter_host() {
        YG_TRY(ensure_host());
        mirror.host_written();
        return YAGI_OK;
    }
    void execute(T *rxx, float *energy) { autocorr_host<T>(win.data(), W, d, rxx, energy); }   // after ensure_host
    int block_dev(const T *x, size_t nb, T *rxx, float *energy) {
        if (nb == 0) return YAGI_OK;
        YG_TRY(ensure_dev());
        YG_TRY(launch_autocorr<T>(W, d, hist.cur<T>(), hist.next<T>(), x, nb, rxx, energy, st));
        hist.flip();
        mirror.dev_written();
        return YAGI_OK;
    }
};

}  // namespace yagi

#define YAGI_AUTOCORR_IMPL(K, T)                                                                    \
    struct yagi_hip_autocorr_##K##_s : AutocorrObj<T> {};                                           \
    extern "C" {                                                                                    \
    int yagi_hip_autocorr_##K##_create(size_t window_size, size_t delay, yagi_hip_autocorr_##K *q) try { \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        auto o = std::make_unique<yagi_hip_autocorr_##K##_s>();                                     \
        YG_TRY(o->init(window_size, delay));                                                        \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_autocorr_##K##_destroy(yagi_hip_autocorr_##K q) try {                              \
        if (q) (void)hipStreamSynchronize(q->st);                                                   \
        delete q;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_autocorr_##K##_clone(yagi_hip_autocorr_##K q, yagi_hip_autocorr_##K *out) try {    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        YG_TRY(q->ensure_host());                                                                   \
        auto o = std::make_unique<yagi_hip_autocorr_##K##_s>();                                     \
        o->st = q->st;                                                                              \
        o->W = q->W;                                                                                \
        o->d = q->d;                                                                                \
        YG_TRY(o->hist.alloc(o->bytes()));                                                          \
        o->win.init(o->len());                                                                      \
        o->win.load(q->win.data());                                                                 \
        o->mirror.host_written();                                                                   \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_autocorr_##K##_set_stream(yagi_hip_autocorr_##K q, yagi_stream_t s) try {          \
        CHECK_Q(q);                                                                                 \
        if (q->st == to_stream(s)) return YAGI_OK;                                                  \
        YG_HIP(hipStreamSynchronize(q->st));                                                        \
        q->st = to_stream(s);                                                                       \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_autocorr_##K##_reset(yagi_hip_autocorr_##K q) try {                                \
        CHECK_Q(q);                                                                                 \
        return q->reset();                                                                          \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_autocorr_##K##_get_window_size(yagi_hip_autocorr_##K q, size_t *window_size) try { \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(window_size);                                                                     \
        *window_size = (size_t)q->W;                                                                \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_autocorr_##K##_get_delay(yagi_hip_autocorr_##K q, size_t *delay) try {             \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(delay);                                                                           \
        *delay = (size_t)q->d;                                                                      \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_autocorr_##K##_push(yagi_hip_autocorr_##K q, T x) try {                            \
        CHECK_Q(q);                                                                                 \
        YG_TRY(q->enter_host());                                                                    \
        q->win.push(x);                                                                             \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_autocorr_##K##_write(yagi_hip_autocorr_##K q, const T *x, size_t n) try {          \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        YG_TRY(q->enter_host());                                                                    \
        for (size_t i = 0; i < n; ++i) q->win.push(x[i]);                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_autocorr_##K##_execute(yagi_hip_autocorr_##K q, T *rxx) try {                      \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(rxx);                                                                             \
        YG_TRY(q->ensure_host());                                                                   \
        float e;                                                                                    \
        q->execute(rxx, &e);                                                                        \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_autocorr_##K##_get_energy(yagi_hip_autocorr_##K q, float *energy) try {            \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(energy);                                                                          \
        YG_TRY(q->ensure_host());                                                                   \
        T r;                                                                                        \
        q->execute(&r, energy);                                                                     \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_autocorr_##K##_execute_block(yagi_hip_autocorr_##K q, const T *x, size_t n, T *rxx, \
                                              float *energy) try {                                  \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        CHECK_PTR(rxx);                                                                             \
        if (energy) YG_TRY(q->we.ensure(n * sizeof(float)));                                        \
        float *ed = energy ? q->we.as<float>() : nullptr;                                           \
        YG_TRY(q->ws.run(q->st, x, n, rxx, n, [&](const T *xd, T *yd) { return q->block_dev(xd, n, yd, ed); })); \
        if (energy) YG_TRY(download(energy, ed, n * sizeof(float), q->st));                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_autocorr_##K##_execute_block_dev(yagi_hip_autocorr_##K q, const T *x_dev, size_t n, T *rxx_dev, \
                                                  float *energy_dev) try {                          \
        CHECK_Q(q);                                                                                 \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x_dev);                                                                           \
        CHECK_PTR(rxx_dev);                                                                         \
        CHECK_NOALIAS(x_dev, n, rxx_dev, n);                                                        \
        if (energy_dev) {                                                                           \
            CHECK_NOALIAS(x_dev, n, energy_dev, n);                                                 \
            CHECK_NOALIAS(rxx_dev, n, energy_dev, n);                                               \
        }                                                                                           \
        return q->block_dev(x_dev, n, rxx_dev, energy_dev);                                         \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_AUTOCORR_IMPL(cccf, cf32)
YAGI_AUTOCORR_IMPL(rrrf, float)
#undef YAGI_AUTOCORR_IMPL

// ---- BurstDetector (yagi_hip.h; absent from the reference) ----------------------------------------------------------
// The state is Autocorr's history (the last W + d samples) plus a BurstState: the sample counter and the pending run.
// Block calls run burstdet_kernels.hip on the device copy: the tile kernel writes the history the call leaves into the
// other of two buffers, the stitch kernel updates the BurstState in place.  Getters, flush and clone work on a host
// mirror; the two copies are synchronised lazily (Mirror).
namespace yagi {

static int burstdet_check(float threshold, float energy_floor, uint64_t min_length) {
    if (!std::isfinite(threshold) || !(threshold > 0.0f))
        return fail(YAGI_ERR_CONFIG, "threshold must be finite and greater than zero");
    if (!std::isfinite(energy_floor) || !(energy_floor >= 0.0f))
        return fail(YAGI_ERR_CONFIG, "energy floor must be finite and not negative");
    if (min_length < 1) return fail(YAGI_ERR_CONFIG, "minimum length must be at least one");
    return YAGI_OK;
}
static int burstdet_check_window(size_t W, size_t d) {
    if (W == 0) return fail(YAGI_ERR_CONFIG, "window size must be greater than zero");
    if (W > (size_t)YAGI_AUTOCORR_WMAX)
        return fail(YAGI_ERR_CONFIG, "window size %zu exceeds YAGI_AUTOCORR_WMAX = %d", W, YAGI_AUTOCORR_WMAX);
    if (d > (size_t)YAGI_AUTOCORR_DMAX)
        return fail(YAGI_ERR_CONFIG, "delay %zu exceeds YAGI_AUTOCORR_DMAX = %d", d, YAGI_AUTOCORR_DMAX);
    return YAGI_OK;
}

// What the event detectors share: the threshold settings, the history and the State {position, pool_used, has_pending,
// pending} on the host and on the device, and the calls that move them.  D, the object itself, supplies the history
// length (to alloc_state), most_events(nb) and block_dev(x, nb, events, cap, status).
template <class D, class T, class State, class Ev>
struct EventDetObj {
    hipStream_t st = nullptr;
    float threshold = 0.0f, thr2 = 0.0f, floor_ = 0.0f;
    uint64_t min_length = 1;
    FdHist<T> win;                                        // host mirror: the history
    State hs{};                                           //              counter and pending run
    PingPong<> hist;                                      // device copy of the history
    DevBuf state;                                         //              one State
    DevBuf scratch;                                       // tile table and segment pool, grown with the block length
    Staging ws;                                           // host block form: x; y holds {status, events}
    Mirror mirror;

    size_t bytes() const { return win.len * sizeof(T); }
    int set_threshold(float threshold_, float floor__, uint64_t min_length_) {
        YG_TRY(burstdet_check(threshold_, floor__, min_length_));
        threshold = threshold_;
        thr2 = threshold_ * threshold_;
        floor_ = floor__;
        min_length = min_length_;
        return YAGI_OK;
    }
    int alloc_state(size_t len) {
        YG_TRY(require_device());
        YG_TRY(hist.alloc(len * sizeof(T)));
        YG_TRY(state.alloc(sizeof(State)));
        win.init(len);
        return YAGI_OK;
    }
    int reset() {
        win.zero();
        hs = State{};
        YG_HIP(hipMemsetAsync(hist.cur(), 0, bytes(), st));
        YG_HIP(hipMemsetAsync(state.p, 0, sizeof(State), st));
        mirror.in_sync();
        return YAGI_OK;
    }
    int ensure_host() {
        return mirror.need_host([&] {
            std::vector<T> t(win.len);
            YG_TRY(download(t.data(), hist.cur(), bytes(), st));
            win.load(t.data());
            return download(&hs, state.p, sizeof(State), st);
        });
    }
    int ensure_dev() {
        return mirror.need_dev([&] {
            YG_TRY(upload(hist.cur(), win.data(), bytes(), st));
            return upload(state.p, &hs, sizeof(State), st);
        });
    }
    int block(const T *x, size_t nb, Ev *events, size_t cap, size_t *count, int *overflow) {
        const size_t room = std::min(cap, D::most_events(nb));
        YG_TRY(ws.put(st, x, nb));
        YG_TRY(ws.y.ensure(16 + room * sizeof(Ev)));
        unsigned *sd = ws.y.template as<unsigned>();
        Ev *ed = reinterpret_cast<Ev *>(ws.y.template as<char>() + 16);
        YG_TRY(static_cast<D *>(this)->block_dev(ws.x.template as<T>(), nb, ed, room, sd));
        unsigned status[2];
        YG_TRY(download(status, sd, sizeof status, st));
        *count = status[0];
        *overflow = (int)status[1];
        return download(events, ed, std::min((size_t)status[0], room) * sizeof(Ev), st);
    }
    int flush(Ev *events, size_t cap, size_t *count) {
        YG_TRY(ensure_host());
        *count = 0;
        if (!hs.has_pending) return YAGI_OK;
        if (hs.pending.length >= min_length) {
            if (cap > 0) events[0] = hs.pending;
            *count = 1;
        }
        hs.has_pending = 0;
        mirror.host_written();
        return YAGI_OK;
    }
};

template <class T>
struct BurstDetObj : EventDetObj<BurstDetObj<T>, T, BurstState, yagi_burst_event> {
    int W = 0, d = 0;                                     // the history is W + d samples

    int configure(size_t W_, size_t d_, float threshold_, float floor__, uint64_t min_length_) {
        YG_TRY(burstdet_check_window(W_, d_));
        YG_TRY(this->set_threshold(threshold_, floor__, min_length_));
        W = (int)W_;
        d = (int)d_;
        return YAGI_OK;
    }
    int alloc() { return this->alloc_state((size_t)W + (size_t)d); }
    // events a call of nb samples can report: a run per segment, and the pending run of the call before
    static size_t most_events(size_t nb) {
        return (nb + kAutocorrTile - 1) / kAutocorrTile + (size_t)kBurstSegmax + 1;
    }
    int block_dev(const T *x, size_t nb, yagi_burst_event *events, size_t cap, unsigned *status) {
        YG_TRY(this->ensure_dev());
        YG_TRY(this->scratch.ensure(burstdet_scratch_bytes(nb)));
        YG_TRY(launch_burstdet<T>(W, d, this->thr2, this->floor_, this->min_length, this->hist.template cur<T>(),
                                  this->hist.template next<T>(), x, nb, this->scratch.p,
                                  this->state.template as<BurstState>(), events, cap, status, this->st));
        if (nb != 0) this->hist.flip();
        this->mirror.dev_written();
        return YAGI_OK;
    }
};

}  // namespace yagi

#define YAGI_BURSTDET_GET(K, name, type, expr)                                                      \
    int yagi_hip_burstdet_##K##_get_##name(yagi_hip_burstdet_##K q, type *out) try {                \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = (expr);                                                                              \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }

#define YAGI_BURSTDET_IMPL(K, T)                                                                    \
    struct yagi_hip_burstdet_##K##_s : BurstDetObj<T> {};                                           \
    extern "C" {                                                                                    \
    int yagi_hip_burstdet_##K##_create(size_t window_size, size_t delay, float threshold, float energy_floor, \
                                       uint64_t min_length, yagi_hip_burstdet_##K *q) try {         \
        CHECK_PTR(q);                                                                               \
        *q = nullptr;                                                                               \
        auto o = std::make_unique<yagi_hip_burstdet_##K##_s>();                                     \
        YG_TRY(o->configure(window_size, delay, threshold, energy_floor, min_length));              \
        YG_TRY(o->alloc());                                                                         \
        YG_TRY(o->reset());                                                                         \
        *q = o.release();                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_burstdet_##K##_destroy(yagi_hip_burstdet_##K q) try {                              \
        if (q) (void)hipStreamSynchronize(q->st);                                                   \
        delete q;                                                                                   \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_burstdet_##K##_clone(yagi_hip_burstdet_##K q, yagi_hip_burstdet_##K *out) try {    \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = nullptr;                                                                             \
        YG_TRY(q->ensure_host());                                                                   \
        auto o = std::make_unique<yagi_hip_burstdet_##K##_s>();                                     \
        o->st = q->st;                                                                              \
        YG_TRY(o->configure((size_t)q->W, (size_t)q->d, q->threshold, q->floor_, q->min_length));   \
        YG_TRY(o->alloc());                                                                         \
        o->win.load(q->win.data());                                                                 \
        o->hs = q->hs;                                                                              \
        o->mirror.host_written();                                                                   \
        *out = o.release();                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_burstdet_##K##_set_stream(yagi_hip_burstdet_##K q, yagi_stream_t s) try {          \
        CHECK_Q(q);                                                                                 \
        if (q->st == to_stream(s)) return YAGI_OK;                                                  \
        YG_HIP(hipStreamSynchronize(q->st));                                                        \
        q->st = to_stream(s);                                                                       \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_burstdet_##K##_reset(yagi_hip_burstdet_##K q) try {                                \
        CHECK_Q(q);                                                                                 \
        return q->reset();                                                                          \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    YAGI_BURSTDET_GET(K, window_size, size_t, (size_t)q->W)                                         \
    YAGI_BURSTDET_GET(K, delay, size_t, (size_t)q->d)                                               \
    YAGI_BURSTDET_GET(K, threshold, float, q->threshold)                                            \
    YAGI_BURSTDET_GET(K, energy_floor, float, q->floor_)                                            \
    YAGI_BURSTDET_GET(K, min_length, uint64_t, q->min_length)                                       \
    int yagi_hip_burstdet_##K##_get_position(yagi_hip_burstdet_##K q, uint64_t *position) try {     \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(position);                                                                        \
        YG_TRY(q->ensure_host());                                                                   \
        *position = q->hs.position;                                                                 \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_burstdet_##K##_get_pending(yagi_hip_burstdet_##K q, int *has_pending, yagi_burst_event *ev) try { \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(has_pending);                                                                     \
        CHECK_PTR(ev);                                                                              \
        YG_TRY(q->ensure_host());                                                                   \
        *has_pending = q->hs.has_pending != 0;                                                      \
        *ev = *has_pending ? q->hs.pending : yagi_burst_event{};                                    \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_burstdet_##K##_detect_block(yagi_hip_burstdet_##K q, const T *x, size_t n, yagi_burst_event *events, \
                                             size_t cap, size_t *count, int *overflow) try {        \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(count);                                                                           \
        CHECK_PTR(overflow);                                                                        \
        *count = 0;                                                                                 \
        *overflow = 0;                                                                              \
        if (n == 0) return YAGI_OK;                                                                 \
        CHECK_PTR(x);                                                                               \
        if (cap != 0) CHECK_PTR(events);                                                            \
        return q->block(x, n, events, cap, count, overflow);                                        \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_burstdet_##K##_detect_block_dev(yagi_hip_burstdet_##K q, const T *x_dev, size_t n, \
                                                 yagi_burst_event *events_dev, size_t cap, uint32_t *status_dev) try { \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(status_dev);                                                                      \
        if (n != 0) CHECK_PTR(x_dev);                                                               \
        if (cap != 0) CHECK_PTR(events_dev);                                                        \
        if (n != 0) {                                                                               \
            if (cap != 0) CHECK_NOALIAS(x_dev, n, events_dev, cap);                                 \
            CHECK_NOALIAS(x_dev, n, status_dev, 2);                                                 \
        }                                                                                           \
        if (cap != 0) CHECK_NOALIAS(events_dev, cap, status_dev, 2);                                \
        return q->block_dev(x_dev, n, events_dev, cap, status_dev);                                 \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_burstdet_##K##_flush(yagi_hip_burstdet_##K q, yagi_burst_event *events, size_t cap, size_t *count) try { \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(count);                                                                           \
        if (cap != 0) CHECK_PTR(events);                                                            \
        return q->flush(events, cap, count);                                                        \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_burstdet_##K##_detect_host(size_t window_size, size_t delay, float threshold, float energy_floor, \
                                            uint64_t min_length, const T *x, size_t n, yagi_burst_event *events, \
                                            size_t cap, size_t *count, int *overflow, int *has_pending, \
                                            yagi_burst_event *pending) try {                        \
        CHECK_PTR(count);                                                                           \
        CHECK_PTR(overflow);                                                                        \
        CHECK_PTR(has_pending);                                                                     \
        CHECK_PTR(pending);                                                                         \
        if (n != 0) CHECK_PTR(x);                                                                   \
        if (cap != 0) CHECK_PTR(events);                                                            \
        YG_TRY(burstdet_check_window(window_size, delay));                                          \
        YG_TRY(burstdet_check(threshold, energy_floor, min_length));                                \
        std::vector<T> win(window_size + delay, T{});                                               \
        BurstState s{};                                                                             \
        YG_TRY(burstdet_host<T>((int)window_size, (int)delay, threshold * threshold, energy_floor, min_length, \
                                win.data(), &s, x, n, events, cap, count, overflow));               \
        *has_pending = s.has_pending != 0;                                                          \
        *pending = s.has_pending ? s.pending : yagi_burst_event{};                                  \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_BURSTDET_IMPL(cccf, cf32)
YAGI_BURSTDET_IMPL(rrrf, float)
#undef YAGI_BURSTDET_IMPL
#undef YAGI_BURSTDET_GET

// ---- PreambleDetector (yagi_hip.h; absent from the reference) -------------------------------------------------------
// The state is the history (the last L samples) plus a PdetState: the sample counter and the pending run.  Block calls
// run pdet_kernels.hip on the device copy: the tile kernel writes the history the call leaves into the other of two
// buffers, the stitch kernel updates the PdetState in place.  Getters, flush and clone work on a host mirror; the two
// copies are synchronised lazily (Mirror).  The templates are built once on the host and never change.
namespace yagi {

struct PdetObj : EventDetObj<PdetObj, cf32, PdetState, yagi_preamble_event> {
    int L = 0, K = 0;                                     // the history is L samples
    float ep = 0.0f;
    std::vector<float> dphi;                              // K
    std::vector<cf32> tmpl;                               // [K][L]
    DevBuf tmpl_dev;                                      // [K][pdet_pitch(L)]
    DevBuf we;                                            // host correlate form: the energies on the device (ws.y: rxy)

    // everything that needs no device
    int configure(const cf32 *p, size_t L_, const float *dphi_, size_t K_, float threshold_, float floor__,
                  uint64_t min_length_) {
        if (L_ == 0 || L_ > (size_t)YAGI_PDET_LMAX)
            return fail(YAGI_ERR_CONFIG, "preamble length %zu is outside 1 .. YAGI_PDET_LMAX = %d", L_, YAGI_PDET_LMAX);
        if (K_ == 0 || K_ > (size_t)YAGI_PDET_KMAX)
            return fail(YAGI_ERR_CONFIG, "%zu hypotheses are outside 1 .. YAGI_PDET_KMAX = %d", K_, YAGI_PDET_KMAX);
        if (!p || !dphi_) return fail(YAGI_ERR_CONFIG, "null pointer argument");
        for (size_t k = 0; k < K_; ++k)
            if (!std::isfinite(dphi_[k])) return fail(YAGI_ERR_CONFIG, "hypothesis %zu is not finite", k);
        YG_TRY(set_threshold(threshold_, floor__, min_length_));
        const float e = pdet_preamble_energy(p, L_);
        if (!std::isfinite(e) || !(e > 0.0f))
            return fail(YAGI_ERR_CONFIG, "the preamble's energy must be finite and greater than zero");
        L = (int)L_;
        K = (int)K_;
        ep = e;
        dphi.assign(dphi_, dphi_ + K_);
        tmpl.resize(K_ * L_);
        pdet_templates(p, L_, dphi_, K_, tmpl.data());
        return YAGI_OK;
    }
    int copy_config(const PdetObj &o) {
        L = o.L, K = o.K, threshold = o.threshold, thr2 = o.thr2, floor_ = o.floor_, ep = o.ep, min_length = o.min_length;
        dphi = o.dphi;
        tmpl = o.tmpl;
        return YAGI_OK;
    }
    int alloc() {
        YG_TRY(alloc_state((size_t)L));
        const size_t pitch = pdet_pitch((size_t)L);
        std::vector<cf32> rows((size_t)K * pitch, cf32{});
        for (int k = 0; k < K; ++k) {
            const cf32 *row = tmpl.data() + (size_t)k * (size_t)L;
            std::copy(row, row + L, rows.begin() + (size_t)k * pitch);
        }
        return fill(tmpl_dev, rows.data(), rows.size() * sizeof(cf32), st);
    }
    // events a call of nb samples can report: a run per segment, and the pending run of the call before
    static size_t most_events(size_t nb) { return (nb + kPdetTile - 1) / kPdetTile + (size_t)kPdetSegmax + 1; }
    int block_dev(const cf32 *x, size_t nb, yagi_preamble_event *events, size_t cap, unsigned *status) {
        YG_TRY(ensure_dev());
        YG_TRY(scratch.ensure(pdet_scratch_bytes(nb)));
        YG_TRY(launch_pdet(L, K, tmpl_dev.as<cf32>(), ep, thr2, floor_, min_length, hist.cur<cf32>(), hist.next<cf32>(), x,
                           nb, scratch.p, state.as<PdetState>(), events, cap, status, st));
        if (nb != 0) hist.flip();
        mirror.dev_written();
        return YAGI_OK;
    }
    int correlate_dev(const cf32 *x, size_t nb, cf32 *rxy, float *energy) {
        if (nb == 0) return YAGI_OK;
        YG_TRY(ensure_dev());
        YG_TRY(launch_pdet_correlate(L, K, tmpl_dev.as<cf32>(), hist.cur<cf32>(), hist.next<cf32>(), x, nb, rxy, energy,
                                     state.as<PdetState>(), st));
        hist.flip();
        mirror.dev_written();
        return YAGI_OK;
    }
};

}  // namespace yagi

struct yagi_hip_pdet_cccf_s : PdetObj {};

#define YAGI_PDET_GET(name, type, expr)                                                             \
    int yagi_hip_pdet_cccf_get_##name(yagi_hip_pdet_cccf q, type *out) try {                        \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(out);                                                                             \
        *out = (expr);                                                                              \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }

extern "C" {

int yagi_hip_pdet_templates(const cf32 *p, size_t L, const float *dphi, size_t K, cf32 *out) try {
    if (L == 0 || L > (size_t)YAGI_PDET_LMAX || K == 0 || K > (size_t)YAGI_PDET_KMAX)
        return fail(YAGI_ERR_CONFIG, "(length, hypotheses) = (%zu, %zu) out of range", L, K);
    CHECK_PTR(p);
    CHECK_PTR(dphi);
    CHECK_PTR(out);
    for (size_t k = 0; k < K; ++k)
        if (!std::isfinite(dphi[k])) return fail(YAGI_ERR_CONFIG, "hypothesis %zu is not finite", k);
    pdet_templates(p, L, dphi, K, out);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_create(const cf32 *p, size_t L, const float *dphi, size_t K, float threshold, float energy_floor,
                              uint64_t min_length, yagi_hip_pdet_cccf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    auto o = std::make_unique<yagi_hip_pdet_cccf_s>();
    YG_TRY(o->configure(p, L, dphi, K, threshold, energy_floor, min_length));
    YG_TRY(o->alloc());
    YG_TRY(o->reset());
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_destroy(yagi_hip_pdet_cccf q) try {
    if (q) (void)hipStreamSynchronize(q->st);
    delete q;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_clone(yagi_hip_pdet_cccf q, yagi_hip_pdet_cccf *out) try {
    CHECK_Q(q);
    CHECK_PTR(out);
    *out = nullptr;
    YG_TRY(q->ensure_host());
    auto o = std::make_unique<yagi_hip_pdet_cccf_s>();
    o->st = q->st;
    YG_TRY(o->copy_config(*q));
    YG_TRY(o->alloc());
    o->win.load(q->win.data());
    o->hs = q->hs;
    o->mirror.host_written();
    *out = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_set_stream(yagi_hip_pdet_cccf q, yagi_stream_t s) try {
    CHECK_Q(q);
    if (q->st == to_stream(s)) return YAGI_OK;
    YG_HIP(hipStreamSynchronize(q->st));
    q->st = to_stream(s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_reset(yagi_hip_pdet_cccf q) try {
    CHECK_Q(q);
    return q->reset();
} catch (...) { return ::yagi::api_exception(); }

YAGI_PDET_GET(length, size_t, (size_t)q->L)
YAGI_PDET_GET(hypotheses, size_t, (size_t)q->K)
YAGI_PDET_GET(threshold, float, q->threshold)
YAGI_PDET_GET(energy_floor, float, q->floor_)
YAGI_PDET_GET(min_length, uint64_t, q->min_length)
YAGI_PDET_GET(preamble_energy, float, q->ep)

int yagi_hip_pdet_cccf_get_dphi(yagi_hip_pdet_cccf q, float *dphi) try {
    CHECK_Q(q);
    CHECK_PTR(dphi);
    std::copy(q->dphi.begin(), q->dphi.end(), dphi);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_get_templates(yagi_hip_pdet_cccf q, cf32 *templates) try {
    CHECK_Q(q);
    CHECK_PTR(templates);
    std::copy(q->tmpl.begin(), q->tmpl.end(), templates);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_get_position(yagi_hip_pdet_cccf q, uint64_t *position) try {
    CHECK_Q(q);
    CHECK_PTR(position);
    YG_TRY(q->ensure_host());
    *position = q->hs.position;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_get_pending(yagi_hip_pdet_cccf q, int *has_pending, yagi_preamble_event *ev) try {
    CHECK_Q(q);
    CHECK_PTR(has_pending);
    CHECK_PTR(ev);
    YG_TRY(q->ensure_host());
    *has_pending = q->hs.has_pending != 0;
    *ev = *has_pending ? q->hs.pending : yagi_preamble_event{};
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_detect_block(yagi_hip_pdet_cccf q, const cf32 *x, size_t n, yagi_preamble_event *events, size_t cap,
                                    size_t *count, int *overflow) try {
    CHECK_Q(q);
    CHECK_PTR(count);
    CHECK_PTR(overflow);
    *count = 0;
    *overflow = 0;
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x);
    if (cap != 0) CHECK_PTR(events);
    return q->block(x, n, events, cap, count, overflow);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_detect_block_dev(yagi_hip_pdet_cccf q, const cf32 *x_dev, size_t n, yagi_preamble_event *events_dev,
                                        size_t cap, uint32_t *status_dev) try {
    CHECK_Q(q);
    CHECK_PTR(status_dev);
    if (n != 0) CHECK_PTR(x_dev);
    if (cap != 0) CHECK_PTR(events_dev);
    if (n != 0) {
        if (cap != 0) CHECK_NOALIAS(x_dev, n, events_dev, cap);
        CHECK_NOALIAS(x_dev, n, status_dev, 2);
    }
    if (cap != 0) CHECK_NOALIAS(events_dev, cap, status_dev, 2);
    return q->block_dev(x_dev, n, events_dev, cap, status_dev);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_correlate_block(yagi_hip_pdet_cccf q, const cf32 *x, size_t n, cf32 *rxy, float *energy) try {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x);
    CHECK_PTR(rxy);
    const size_t kn = (size_t)q->K * n;
    if (energy) YG_TRY(q->we.ensure(n * sizeof(float)));
    float *ed = energy ? q->we.as<float>() : nullptr;
    YG_TRY(q->ws.run(q->st, x, n, rxy, kn, [&](const cf32 *xd, cf32 *yd) { return q->correlate_dev(xd, n, yd, ed); }));
    if (energy) YG_TRY(download(energy, ed, n * sizeof(float), q->st));
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_correlate_block_dev(yagi_hip_pdet_cccf q, const cf32 *x_dev, size_t n, cf32 *rxy_dev,
                                           float *energy_dev) try {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x_dev);
    CHECK_PTR(rxy_dev);
    const size_t kn = (size_t)q->K * n;
    CHECK_NOALIAS(x_dev, n, rxy_dev, kn);
    if (energy_dev) {
        CHECK_NOALIAS(x_dev, n, energy_dev, n);
        CHECK_NOALIAS(rxy_dev, kn, energy_dev, n);
    }
    return q->correlate_dev(x_dev, n, rxy_dev, energy_dev);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_flush(yagi_hip_pdet_cccf q, yagi_preamble_event *events, size_t cap, size_t *count) try {
    CHECK_Q(q);
    CHECK_PTR(count);
    if (cap != 0) CHECK_PTR(events);
    return q->flush(events, cap, count);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_pdet_cccf_detect_host(const cf32 *p, size_t L, const float *dphi, size_t K, float threshold,
                                   float energy_floor, uint64_t min_length, const cf32 *x, size_t n,
                                   yagi_preamble_event *events, size_t cap, size_t *count, int *overflow, int *has_pending,
                                   yagi_preamble_event *pending) try {
    CHECK_PTR(count);
    CHECK_PTR(overflow);
    CHECK_PTR(has_pending);
    CHECK_PTR(pending);
    if (n != 0) CHECK_PTR(x);
    if (cap != 0) CHECK_PTR(events);
    PdetObj o;
    YG_TRY(o.configure(p, L, dphi, K, threshold, energy_floor, min_length));
    std::vector<cf32> win(L, cf32{});
    PdetState s{};
    YG_TRY(pdet_host(o.L, o.K, o.tmpl.data(), o.ep, o.thr2, energy_floor, min_length, win.data(), &s, x, n, events, cap,
                     count, overflow));
    *has_pending = s.has_pending != 0;
    *pending = s.has_pending ? s.pending : yagi_preamble_event{};
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"
#undef YAGI_PDET_GET

// ---- SymSync (src/filter/symsync.rs, one object per channel) --------------------------------------------------------
// The state is the [Ls][channels] history plus one SymsyncChan per channel; symsync_kernels.hip updates both in place on
// the device.  Setters that touch per-channel state (set_output_rate, reset_channel), the getters and clone work on a
// host mirror; the two copies are synchronised lazily (Mirror).  The loop filter, the lock flag and k_out travel to the
// kernel by value with every call.
namespace yagi {

// everything that needs no device
struct SymsyncHost {
    size_t C = 0, k = 0, npfb = 0, Ls = 0, k_out = 1;
    SymsyncLoop p{};
    std::vector<float> taps;                              // [npfb][Ls] entries (H, D)
    std::vector<SymsyncChan> hs;                          // host mirror
    std::vector<cf32> hh;

    void reset_chan(size_t c) { symsync_reset_chan(&hs[c], k, k_out); }
    int configure(size_t channels, size_t k_, size_t npfb_, const float *h, size_t h_len) {
        if (channels == 0 || channels > (size_t)YAGI_SYMSYNC_CHANNELS_MAX)
            return fail(YAGI_ERR_CONFIG, "symsync: %zu channels are outside 1 .. YAGI_SYMSYNC_CHANNELS_MAX", channels);
        YG_TRY(symsync_design(k_, npfb_, h, h_len, taps, &Ls));
        C = channels, k = k_, npfb = npfb_, k_out = 1;
        p = SymsyncLoop{};
        p.kf = (float)k;
        p.knorm = p.kf * p.kf + 0.0f * 0.0f;
        p.npfbf = (float)npfb;
        p.npfb = (unsigned)npfb, p.Ls = (unsigned)Ls, p.locked = 0, p.k_out = 1;
        YG_TRY(symsync_set_bw(0.01f, &p));
        hs.assign(C, SymsyncChan{});
        hh.assign(Ls * C, cf32{});
        for (size_t c = 0; c < C; ++c) reset_chan(c);
        return YAGI_OK;
    }
    // the output rate of a design that has not run yet: every channel starts over at it
    int start_at_rate(size_t k_out_) {
        if (k_out_ == 0) return fail(YAGI_ERR_CONFIG, "output rate must be greater than 0");
        k_out = k_out_;
        p.k_out = k_out_;
        for (size_t c = 0; c < C; ++c) reset_chan(c);
        return YAGI_OK;
    }
    static int check_block(size_t C, size_t x_pitch, size_t n, size_t y_pitch, size_t ycap) {
        if (n >= ((size_t)1 << 31) || ycap >= ((size_t)1 << 31))
            return fail(YAGI_ERR_CONFIG, "symsync: n and ycap must be below 2^31");
        if (x_pitch < C || y_pitch < C || x_pitch >= ((size_t)1 << 31) || y_pitch >= ((size_t)1 << 31))
            return fail(YAGI_ERR_CONFIG, "symsync: the pitches are in samples, at least the channel count and below 2^31");
        return YAGI_OK;
    }
};

struct SymsyncObj : SymsyncHost, BankObj<SymsyncObj> {
    using Host = SymsyncHost;
    static constexpr const char *kFamily = "symsync";
    DevBuf taps_dev, state_dev, hist_dev, wstatus;

    int alloc() {
        YG_TRY(require_device());
        YG_TRY(fill(taps_dev, taps.data(), taps.size() * sizeof(float), st));
        YG_TRY(state_dev.alloc(C * sizeof(SymsyncChan)));
        YG_TRY(hist_dev.alloc(Ls * C * sizeof(cf32)));
        YG_TRY(wstatus.alloc(2 * C * sizeof(unsigned)));
        mirror.host_written();
        return YAGI_OK;
    }
    template <class F>
    int each_array(F &&f) {
        YG_TRY(f(state_dev, hs.data(), C * sizeof(SymsyncChan)));
        return f(hist_dev, hh.data(), Ls * C * sizeof(cf32));
    }
    int set_output_rate(size_t k_out_) {
        if (k_out_ == 0) return fail(YAGI_ERR_CONFIG, "output rate must be greater than 0");
        return edit([&] {
            k_out = k_out_;
            p.k_out = k_out_;
            for (auto &s : hs) {
                s.rate = (float)k / (float)k_out;
                s.del = s.rate;
            }
        });
    }
    int block_dev(const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch, size_t ycap, unsigned *status) {
        YG_TRY(ensure_dev());
        YG_TRY(launch_symsync(p, taps_dev.as<float>(), state_dev.as<SymsyncChan>(), hist_dev.as<cf32>(), C, x, x_pitch, n,
                              y, y_pitch, ycap, status, st));
        mirror.dev_written();
        return YAGI_OK;
    }
};

}  // namespace yagi

struct yagi_hip_symsync_crcf_s : SymsyncObj {};

namespace {

// create_rnyquist (:112-131) and create_kaiser (:133-158): the prototype
int symsync_rnyquist_taps(int ftype, size_t k, size_t m, float beta, size_t npfb, std::vector<float> &h) {
    if (k < 2) return fail(YAGI_ERR_CONFIG, "samples/symbol must be at least 2");
    if (m == 0) return fail(YAGI_ERR_CONFIG, "filter delay must be greater than 0");
    if (!(beta >= 0.0f && beta <= 1.0f)) return fail(YAGI_ERR_CONFIG, "excess bandwidth factor must be in [0,1]");
    if (npfb == 0) return fail(YAGI_ERR_CONFIG, "number of filters must be greater than 0");
    if (npfb > (size_t)YAGI_SYMSYNC_NPFB_MAX || 2 * k * m > (size_t)YAGI_SYMSYNC_LS_MAX)
        return fail(YAGI_ERR_CONFIG, "symsync: (npfb, 2 k m) = (%zu, %zu) out of range", npfb, 2 * k * m);
    return design_prototype(ftype, k * npfb, m, beta, 0.0f, h);
}
int symsync_kaiser_taps(size_t k, size_t m, float beta, size_t npfb, std::vector<float> &h) {
    if (k < 2) return fail(YAGI_ERR_CONFIG, "samples/symbol must be at least 2");
    if (m == 0) return fail(YAGI_ERR_CONFIG, "filter delay must be greater than 0");
    if (!(beta > 0.0f && beta <= 1.0f)) return fail(YAGI_ERR_CONFIG, "excess bandwidth factor must be in [0,1]");
    if (npfb == 0) return fail(YAGI_ERR_CONFIG, "number of filters must be greater than 0");
    if (npfb > (size_t)YAGI_SYMSYNC_NPFB_MAX || 2 * k * m > (size_t)YAGI_SYMSYNC_LS_MAX)
        return fail(YAGI_ERR_CONFIG, "symsync: (npfb, 2 k m) = (%zu, %zu) out of range", npfb, 2 * k * m);
    const float fc = 0.75f;
    YG_TRY(design_kaiser(2 * npfb * k * m + 1, fc / ((float)k * (float)npfb), 40.0f, 0.0f, h));
    for (float &c : h) c *= 2.0f * fc;
    return YAGI_OK;
}

}  // namespace

extern "C" {

int yagi_hip_symsync_crcf_create(size_t channels, size_t k, size_t npfb, const float *h, size_t h_len,
                                 yagi_hip_symsync_crcf *q) try {
    return bank_create(q, channels, k, npfb, h, h_len);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_create_rnyquist(size_t channels, int ftype, size_t k, size_t m, float beta, size_t npfb,
                                          yagi_hip_symsync_crcf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    std::vector<float> h;
    YG_TRY(symsync_rnyquist_taps(ftype, k, m, beta, npfb, h));
    return bank_create(q, channels, k, npfb, h.data(), h.size());
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_create_kaiser(size_t channels, size_t k, size_t m, float beta, size_t npfb,
                                        yagi_hip_symsync_crcf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    std::vector<float> h;
    YG_TRY(symsync_kaiser_taps(k, m, beta, npfb, h));
    return bank_create(q, channels, k, npfb, h.data(), h.size());
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_rnyquist_taps(int ftype, size_t k, size_t m, float beta, size_t npfb, float *h) try {
    CHECK_PTR(h);
    std::vector<float> v;
    YG_TRY(symsync_rnyquist_taps(ftype, k, m, beta, npfb, v));
    std::copy(v.begin(), v.end(), h);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_kaiser_taps(size_t k, size_t m, float beta, size_t npfb, float *h) try {
    CHECK_PTR(h);
    std::vector<float> v;
    YG_TRY(symsync_kaiser_taps(k, m, beta, npfb, v));
    std::copy(v.begin(), v.end(), h);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_destroy(yagi_hip_symsync_crcf q) try {
    return bank_destroy(q);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_clone(yagi_hip_symsync_crcf q, yagi_hip_symsync_crcf *out) try {
    return bank_clone(q, out);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_set_stream(yagi_hip_symsync_crcf q, yagi_stream_t s) try {
    return bank_set_stream(q, s);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_reset(yagi_hip_symsync_crcf q) try {
    CHECK_Q(q);
    return q->reset();
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_reset_channel(yagi_hip_symsync_crcf q, size_t c) try {
    CHECK_Q(q);
    return q->reset_channel(c);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_lock(yagi_hip_symsync_crcf q) try {
    CHECK_Q(q);
    q->p.locked = 1;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_unlock(yagi_hip_symsync_crcf q) try {
    CHECK_Q(q);
    q->p.locked = 0;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_is_locked(yagi_hip_symsync_crcf q, int *locked) try {
    return bank_get(q, locked, [](auto &o) { return o.p.locked != 0; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_set_output_rate(yagi_hip_symsync_crcf q, size_t k_out) try {
    CHECK_Q(q);
    return q->set_output_rate(k_out);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_set_lf_bw(yagi_hip_symsync_crcf q, float bw) try {
    CHECK_Q(q);
    return symsync_set_bw(bw, &q->p);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_get_channels(yagi_hip_symsync_crcf q, size_t *channels) try {
    return bank_get(q, channels, [](auto &o) { return o.C; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_get_branch_length(yagi_hip_symsync_crcf q, size_t *Ls) try {
    return bank_get(q, Ls, [](auto &o) { return o.Ls; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_get_tau(yagi_hip_symsync_crcf q, float *tau) try {
    return bank_get_each(q, tau, [](auto &o, size_t c) { return o.hs[c].tau_decim; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_get_stalled(yagi_hip_symsync_crcf q, uint32_t *stalled) try {
    return bank_get_each(q, stalled, [](auto &o, size_t c) { return o.hs[c].stalled; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_execute_dev(yagi_hip_symsync_crcf q, const cf32 *x_dev, size_t x_pitch, size_t n, cf32 *y_dev,
                                      size_t y_pitch, size_t ycap, uint32_t *status_dev) try {
    CHECK_Q(q);
    CHECK_PTR(status_dev);
    YG_TRY(SymsyncHost::check_block(q->C, x_pitch, n, y_pitch, ycap));
    if (n != 0) CHECK_PTR(x_dev);
    if (ycap != 0) CHECK_PTR(y_dev);
    return q->block_dev(x_dev, x_pitch, n, y_dev, y_pitch, ycap, status_dev);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_execute(yagi_hip_symsync_crcf q, const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch,
                                  size_t ycap, uint32_t *ny, uint32_t *stalled) try {
    CHECK_Q(q);
    CHECK_PTR(ny);
    CHECK_PTR(stalled);
    const size_t C = q->C;
    YG_TRY(SymsyncHost::check_block(C, x_pitch, n, y_pitch, ycap));
    if (n != 0) CHECK_PTR(x);
    if (ycap != 0) CHECK_PTR(y);
    const size_t nx = n ? (n - 1) * x_pitch + C : 0;
    YG_TRY(q->ws.put(q->st, x, nx));
    YG_TRY(q->ws.y.ensure(ycap * C * sizeof(cf32)));
    YG_TRY(q->block_dev(q->ws.x.as<cf32>(), x_pitch, n, q->ws.y.as<cf32>(), C, ycap, q->wstatus.as<unsigned>()));
    return q->fetch_ragged(q->wstatus, 2 * C, ny, stalled, y, y_pitch);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symsync_crcf_execute_host(size_t channels, size_t k, size_t npfb, const float *h, size_t h_len, size_t k_out,
                                       float bw, int locked, const cf32 *x, size_t x_pitch, size_t n, cf32 *y,
                                       size_t y_pitch, size_t ycap, uint32_t *ny, uint32_t *stalled, float *tau) try {
    CHECK_PTR(ny);
    CHECK_PTR(stalled);
    SymsyncHost o;
    YG_TRY(o.configure(channels, k, npfb, h, h_len));
    YG_TRY(o.start_at_rate(k_out));
    YG_TRY(symsync_set_bw(bw, &o.p));
    o.p.locked = locked != 0;
    YG_TRY(SymsyncHost::check_block(channels, x_pitch, n, y_pitch, ycap));
    if (n != 0) CHECK_PTR(x);
    if (ycap != 0) CHECK_PTR(y);
    symsync_host(o.p, o.taps.data(), o.hs.data(), o.hh.data(), channels, x, x_pitch, n, y, y_pitch, ycap, ny, stalled);
    if (tau)
        for (size_t c = 0; c < channels; ++c) tau[c] = o.hs[c].tau_decim;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- EqLms (src/equalization/eqlms.rs, one object per channel) -----------------------------------------------------
// The state is the weights and the window, [h_len][channels] each, plus one EqlmsChan per channel; eqlms_kernels.hip
// updates all three in place on the device.  reset, reset_channel, the getters and clone work on a host mirror; the two
// copies are synchronised lazily (Mirror).  mu, k and the mode travel to the kernel by value with every call.
namespace yagi {

// set_constellation's table, of EqLms and EqRls alike
static int eq_check_table(const cf32 *t, size_t M) {
    if (M == 0 || M > (size_t)YAGI_EQLMS_TABLE_MAX)
        return fail(YAGI_ERR_CONFIG, "eqlms: a constellation of %zu points is outside 1 .. YAGI_EQLMS_TABLE_MAX", M);
    if (!t) return fail(YAGI_ERR_CONFIG, "null pointer argument");
    return YAGI_OK;
}

// What the device halves of EqLms and EqRls share: DECISION's table and the host block form.  D supplies kTrain,
// check_block(..) and block_dev(..), and its host struct the table.
template <class D>
struct EqBankObj : BankObj<D> {
    DevBuf table_dev;
    Staging wsd;                                          // host block form: the rows of d

    int alloc_table() {
        D &o = this->self();
        if (o.table.empty()) return YAGI_OK;
        return fill(table_dev, o.table.data(), o.table.size() * sizeof(cf32), this->st);
    }
    int set_constellation(const cf32 *table, size_t M) {
        D &o = this->self();
        YG_TRY(eq_check_table(table, M));
        YG_HIP(hipStreamSynchronize(this->st));              // a launch in flight may still read the table
        o.table.assign(table, table + M);
        return fill(table_dev, o.table.data(), M * sizeof(cf32), this->st);
    }
    int block_host(int mode, size_t k, const cf32 *x, size_t x_pitch, size_t n, const cf32 *d, size_t d_pitch, cf32 *y,
                   size_t y_pitch) {
        D &o = this->self();
        const size_t C = o.C;
        Staging &ws = this->ws;
        size_t rows = 0;
        YG_TRY(D::check_block(C, mode, k, x_pitch, n, d != nullptr, d_pitch, o.table.size(), y_pitch, &rows));
        if (n == 0) return YAGI_OK;
        if (!x || !y) return fail(YAGI_ERR_CONFIG, "null pointer argument");
        YG_TRY(ws.put(this->st, x, (n - 1) * x_pitch + C));
        const bool train = mode == D::kTrain;
        if (train) {
            YG_TRY(wsd.put(this->st, d, (rows - 1) * d_pitch + C));
        }
        YG_TRY(ws.y.ensure(rows * C * sizeof(cf32)));
        YG_TRY(o.block_dev(mode, k, ws.x.as<cf32>(), x_pitch, n, train ? wsd.x.as<cf32>() : nullptr, d_pitch, ws.y.as<cf32>(), C));
        return download_rows(this->st, ws.y, rows, C, y, y_pitch);
    }
};

// everything that needs no device
struct EqlmsHost {
    size_t C = 0, h_len = 0;
    float mu = 0.5f;
    std::vector<cf32> h0, table;
    std::vector<cf32> hw, hh;                             // host mirror: [h_len][C]
    std::vector<EqlmsChan> hs;

    void reset_chan(size_t c) {
        for (size_t i = 0; i < h_len; ++i) {
            hw[i * C + c] = h0[i];
            hh[i * C + c] = cf32{0.0f, 0.0f};
        }
        hs[c] = EqlmsChan{};
    }
    // new (:25-49)
    int configure(size_t channels, const cf32 *h, size_t h_len_) {
        if (channels == 0 || channels > (size_t)YAGI_EQLMS_CHANNELS_MAX)
            return fail(YAGI_ERR_CONFIG, "eqlms: %zu channels are outside 1 .. YAGI_EQLMS_CHANNELS_MAX", channels);
        if (h_len_ == 0) return fail(YAGI_ERR_CONFIG, "filter length must be greater than 0");
        if (h_len_ > (size_t)YAGI_EQLMS_LEN_MAX)
            return fail(YAGI_ERR_CONFIG, "eqlms: %zu taps are more than YAGI_EQLMS_LEN_MAX", h_len_);
        C = channels, h_len = h_len_, mu = 0.5f;
        h0.assign(h_len, cf32{0.0f, 0.0f});
        if (h)
            for (size_t i = 0; i < h_len; ++i) h0[i] = cf32{h[h_len - i - 1].re, -h[h_len - i - 1].im};
        else
            h0[h_len / 2] = cf32{1.0f, 0.0f};
        hw.assign(h_len * C, cf32{});
        hh.assign(h_len * C, cf32{});
        hs.assign(C, EqlmsChan{});
        for (size_t c = 0; c < C; ++c) reset_chan(c);
        return YAGI_OK;
    }
    static int set_bw(float mu_, float *mu) {               // (:105-111)
        if (mu_ < 0.0f) return fail(YAGI_ERR_CONFIG, "learning rate cannot be less than zero");
        *mu = mu_;
        return YAGI_OK;
    }
    // call = a mode (decim_block) or YAGI_EQLMS_EXECUTE; sets the rows of y
    static int check_block(size_t C, int call, size_t k, size_t x_pitch, size_t n, bool have_d, size_t d_pitch, size_t M,
                           size_t y_pitch, size_t *rows) {
        if (call < YAGI_EQLMS_NONE || call > YAGI_EQLMS_EXECUTE)
            return fail(YAGI_ERR_CONFIG, "eqlms: unknown update mode %d", call);
        if (k == 0) return fail(YAGI_ERR_CONFIG, "down-sampling rate 'k' must be greater than 0");
        if (n >= ((size_t)1 << 31) || k >= ((size_t)1 << 31)) return fail(YAGI_ERR_CONFIG, "eqlms: n and k must be below 2^31");
        if (x_pitch < C || y_pitch < C || x_pitch >= ((size_t)1 << 31) || y_pitch >= ((size_t)1 << 31))
            return fail(YAGI_ERR_CONFIG, "eqlms: the pitches are in samples, at least the channel count and below 2^31");
        *rows = n;
        if (call == YAGI_EQLMS_EXECUTE) return YAGI_OK;
        if (n % k != 0) return fail(YAGI_ERR_CONFIG, "eqlms: decim_block takes whole symbols, %zu rows at k = %zu", n, k);
        *rows = n / k;
        if (call == YAGI_EQLMS_TRAIN && *rows != 0) {
            if (!have_d) return fail(YAGI_ERR_CONFIG, "eqlms: TRAIN needs the known symbols d");
            if (d_pitch < C || d_pitch >= ((size_t)1 << 31))
                return fail(YAGI_ERR_CONFIG, "eqlms: the pitches are in samples, at least the channel count and below 2^31");
        }
        if (call == YAGI_EQLMS_DECISION && M == 0)
            return fail(YAGI_ERR_CONFIG, "eqlms: DECISION needs set_constellation first");
        return YAGI_OK;
    }
    void coefficients(cf32 *w0) const {
        for (size_t c = 0; c < C; ++c)
            for (size_t i = 0; i < h_len; ++i) w0[c * h_len + i] = hw[i * C + c];
    }
    void weights(cf32 *w) const {                           // get_weights (:121-123)
        for (size_t c = 0; c < C; ++c)
            for (size_t i = 0; i < h_len; ++i) {
                const cf32 v = hw[(h_len - 1 - i) * C + c];
                w[c * h_len + i] = cf32{v.re, -v.im};
            }
    }
};

struct EqlmsObj : EqlmsHost, EqBankObj<EqlmsObj> {
    using Host = EqlmsHost;
    static constexpr const char *kFamily = "eqlms";
    static constexpr int kTrain = YAGI_EQLMS_TRAIN;
    DevBuf w_dev, hist_dev, state_dev;

    int alloc() {
        YG_TRY(require_device());
        YG_TRY(w_dev.alloc(h_len * C * sizeof(cf32)));
        YG_TRY(hist_dev.alloc(h_len * C * sizeof(cf32)));
        YG_TRY(state_dev.alloc(C * sizeof(EqlmsChan)));
        YG_TRY(alloc_table());
        mirror.host_written();
        return YAGI_OK;
    }
    template <class F>
    int each_array(F &&f) {
        YG_TRY(f(w_dev, hw.data(), h_len * C * sizeof(cf32)));
        YG_TRY(f(hist_dev, hh.data(), h_len * C * sizeof(cf32)));
        return f(state_dev, hs.data(), C * sizeof(EqlmsChan));
    }
    int block_dev(int call, size_t k, const cf32 *x, size_t x_pitch, size_t n, const cf32 *d, size_t d_pitch, cf32 *y,
                  size_t y_pitch) {
        if (n == 0) return YAGI_OK;
        YG_TRY(ensure_dev());
        YG_TRY(launch_eqlms(call, h_len, mu, w_dev.as<cf32>(), hist_dev.as<cf32>(), state_dev.as<EqlmsChan>(), C, k, x,
                            x_pitch, n, d, d_pitch, table_dev.as<cf32>(), table.size(), y, y_pitch, st));
        mirror.dev_written();
        return YAGI_OK;
    }
};

}  // namespace yagi

struct yagi_hip_eqlms_cccf_s : EqlmsObj {};

namespace {

// new_rnyquist (:51-76): the prototype over fl(k), as complex taps
int eqlms_rnyquist_taps(int ftype, size_t k, size_t m, float beta, float dt, std::vector<cf32> &hc) {
    if (k < 2) return fail(YAGI_ERR_CONFIG, "samples/symbol must be greater than 1");
    if (m == 0) return fail(YAGI_ERR_CONFIG, "filter delay must be greater than 0");
    if (!(beta >= 0.0f && beta <= 1.0f)) return fail(YAGI_ERR_CONFIG, "filter excess bandwidth factor must be in [0,1]");
    if (!(dt >= -1.0f && dt <= 1.0f)) return fail(YAGI_ERR_CONFIG, "filter fractional sample delay must be in [-1,1]");
    if (k > (size_t)YAGI_EQLMS_LEN_MAX || m > (size_t)YAGI_EQLMS_LEN_MAX || 2 * k * m + 1 > (size_t)YAGI_EQLMS_LEN_MAX)
        return fail(YAGI_ERR_CONFIG, "eqlms: 2 k m + 1 taps at (k, m) = (%zu, %zu) are more than YAGI_EQLMS_LEN_MAX", k, m);
    std::vector<float> h;
    YG_TRY(design_prototype(ftype, k, m, beta, dt, h));
    hc.resize(h.size());
    const float kf = (float)k;
    for (size_t i = 0; i < h.size(); ++i) hc[i] = cf32{h[i] / kf, 0.0f};
    return YAGI_OK;
}
// new_lowpass (:78-90): x * Complex(2, 0) * fc
int eqlms_lowpass_taps(size_t h_len, float fc, std::vector<cf32> &hc) {
    if (h_len == 0) return fail(YAGI_ERR_CONFIG, "filter length must be greater than 0");
    if (!(fc >= 0.0f && fc <= 0.5f)) return fail(YAGI_ERR_CONFIG, "filter cutoff must be in (0,0.5]");
    if (h_len > (size_t)YAGI_EQLMS_LEN_MAX)
        return fail(YAGI_ERR_CONFIG, "eqlms: %zu taps are more than YAGI_EQLMS_LEN_MAX", h_len);
    std::vector<float> h;
    YG_TRY(design_kaiser(h_len, fc, 40.0f, 0.0f, h));
    hc.resize(h.size());
    for (size_t i = 0; i < h.size(); ++i) {
        const float re = h[i] * 2.0f, im = h[i] * 0.0f;
        hc[i] = cf32{re * fc, im * fc};
    }
    return YAGI_OK;
}

}  // namespace

extern "C" {

int yagi_hip_eqlms_cccf_create(size_t channels, const cf32 *h, size_t h_len, yagi_hip_eqlms_cccf *q) try {
    return bank_create(q, channels, h, h_len);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_create_rnyquist(size_t channels, int ftype, size_t k, size_t m, float beta, float dt,
                                        yagi_hip_eqlms_cccf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    std::vector<cf32> hc;
    YG_TRY(eqlms_rnyquist_taps(ftype, k, m, beta, dt, hc));
    return bank_create(q, channels, hc.data(), hc.size());
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_create_lowpass(size_t channels, size_t h_len, float fc, yagi_hip_eqlms_cccf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    std::vector<cf32> hc;
    YG_TRY(eqlms_lowpass_taps(h_len, fc, hc));
    return bank_create(q, channels, hc.data(), hc.size());
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_destroy(yagi_hip_eqlms_cccf q) try {
    return bank_destroy(q);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_clone(yagi_hip_eqlms_cccf q, yagi_hip_eqlms_cccf *out) try {
    return bank_clone(q, out);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_set_stream(yagi_hip_eqlms_cccf q, yagi_stream_t s) try {
    return bank_set_stream(q, s);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_reset(yagi_hip_eqlms_cccf q) try {
    CHECK_Q(q);
    return q->reset();
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_reset_channel(yagi_hip_eqlms_cccf q, size_t c) try {
    CHECK_Q(q);
    return q->reset_channel(c);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_set_bw(yagi_hip_eqlms_cccf q, float mu) try {
    CHECK_Q(q);
    return EqlmsHost::set_bw(mu, &q->mu);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_get_bw(yagi_hip_eqlms_cccf q, float *mu) try {
    return bank_get(q, mu, [](auto &o) { return o.mu; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_get_length(yagi_hip_eqlms_cccf q, size_t *h_len) try {
    return bank_get(q, h_len, [](auto &o) { return o.h_len; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_get_channels(yagi_hip_eqlms_cccf q, size_t *channels) try {
    return bank_get(q, channels, [](auto &o) { return o.C; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_get_coefficients(yagi_hip_eqlms_cccf q, cf32 *w0) try {
    CHECK_Q(q);
    CHECK_PTR(w0);
    YG_TRY(q->ensure_host());
    q->coefficients(w0);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_get_weights(yagi_hip_eqlms_cccf q, cf32 *w) try {
    CHECK_Q(q);
    CHECK_PTR(w);
    YG_TRY(q->ensure_host());
    q->weights(w);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_set_constellation(yagi_hip_eqlms_cccf q, const cf32 *table, size_t M) try {
    CHECK_Q(q);
    return q->set_constellation(table, M);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_execute_block(yagi_hip_eqlms_cccf q, size_t k, const cf32 *x, size_t x_pitch, size_t n, cf32 *y,
                                      size_t y_pitch) try {
    CHECK_Q(q);
    return q->block_host(YAGI_EQLMS_EXECUTE, k, x, x_pitch, n, nullptr, 0, y, y_pitch);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_execute_block_dev(yagi_hip_eqlms_cccf q, size_t k, const cf32 *x_dev, size_t x_pitch, size_t n,
                                          cf32 *y_dev, size_t y_pitch) try {
    CHECK_Q(q);
    size_t rows = 0;
    YG_TRY(EqlmsHost::check_block(q->C, YAGI_EQLMS_EXECUTE, k, x_pitch, n, false, 0, 0, y_pitch, &rows));
    if (n != 0) {
        CHECK_PTR(x_dev);
        CHECK_PTR(y_dev);
    }
    return q->block_dev(YAGI_EQLMS_EXECUTE, k, x_dev, x_pitch, n, nullptr, 0, y_dev, y_pitch);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_decim_block(yagi_hip_eqlms_cccf q, size_t k, int mode, const cf32 *x, size_t x_pitch, size_t n,
                                    const cf32 *d, size_t d_pitch, cf32 *y, size_t y_pitch) try {
    CHECK_Q(q);
    if (mode == YAGI_EQLMS_EXECUTE) return fail(YAGI_ERR_CONFIG, "eqlms: unknown update mode %d", mode);
    return q->block_host(mode, k, x, x_pitch, n, d, d_pitch, y, y_pitch);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_decim_block_dev(yagi_hip_eqlms_cccf q, size_t k, int mode, const cf32 *x_dev, size_t x_pitch,
                                        size_t n, const cf32 *d_dev, size_t d_pitch, cf32 *y_dev, size_t y_pitch) try {
    CHECK_Q(q);
    if (mode == YAGI_EQLMS_EXECUTE) return fail(YAGI_ERR_CONFIG, "eqlms: unknown update mode %d", mode);
    size_t rows = 0;
    YG_TRY(EqlmsHost::check_block(q->C, mode, k, x_pitch, n, d_dev != nullptr, d_pitch, q->table.size(), y_pitch, &rows));
    if (n != 0) {
        CHECK_PTR(x_dev);
        CHECK_PTR(y_dev);
    }
    return q->block_dev(mode, k, x_dev, x_pitch, n, d_dev, d_pitch, y_dev, y_pitch);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqlms_cccf_execute_host(size_t channels, const cf32 *h, size_t h_len, float mu, int call, size_t k,
                                     const cf32 *x, size_t x_pitch, size_t n, const cf32 *d, size_t d_pitch,
                                     const cf32 *table, size_t M, cf32 *y, size_t y_pitch, cf32 *w0) try {
    EqlmsHost o;
    YG_TRY(o.configure(channels, h, h_len));
    YG_TRY(EqlmsHost::set_bw(mu, &o.mu));
    if (call == YAGI_EQLMS_DECISION) {
        YG_TRY(eq_check_table(table, M));
    }
    size_t rows = 0;
    YG_TRY(EqlmsHost::check_block(channels, call, k, x_pitch, n, d != nullptr, d_pitch, M, y_pitch, &rows));
    if (n != 0) {
        CHECK_PTR(x);
        CHECK_PTR(y);
    }
    eqlms_host(call, h_len, o.mu, o.hw.data(), o.hh.data(), o.hs.data(), channels, k, x, x_pitch, n, d, d_pitch, table, M, y,
               y_pitch);
    if (w0) o.coefficients(w0);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- EqRls (src/equalization/eqrls.rs, one object per channel) -----------------------------------------------------
// The state is P0 [p p][channels], w0, w1 and the window, [p][channels] each; eqrls_kernels.hip updates all four in place
// on the device.  reset, reset_channel, recreate, train's preparation, the getters and clone work on a host mirror; the two
// copies are synchronised lazily (Mirror).  lambda, k, the mode and the lanes per channel travel to the kernel by value.
namespace yagi {

// everything that needs no device
struct EqrlsHost {
    size_t C = 0, p = 0, lanes = 0;                       // lanes: set_lanes' override, 0 = the planner's choice
    float lambda = 0.99f;
    std::vector<cf32> h0, table;
    std::vector<cf32> hP, hw0, hw1, hh;                   // host mirror: [p p][C] and [p][C]

    // reset (:76-88): w1 stays
    void reset_chan(size_t c) {
        const float d = 1.0f / 0.1f;
        for (size_t i = 0; i < p; ++i) {
            for (size_t j = 0; j < p; ++j) hP[(i * p + j) * C + c] = cf32{i == j ? d : 0.0f, 0.0f};
            hw0[i * C + c] = h0[i];
            hh[i * C + c] = cf32{0.0f, 0.0f};
        }
    }
    // new (:31-62)
    static int check_design(size_t channels, size_t p_) {
        if (channels == 0 || channels > (size_t)YAGI_EQRLS_CHANNELS_MAX)
            return fail(YAGI_ERR_CONFIG, "eqrls: %zu channels are outside 1 .. YAGI_EQRLS_CHANNELS_MAX", channels);
        if (p_ == 0) return fail(YAGI_ERR_CONFIG, "equalizer length must be greater than 0");
        if (p_ > (size_t)YAGI_EQRLS_LEN_MAX)
            return fail(YAGI_ERR_CONFIG, "eqrls: %zu taps are more than YAGI_EQRLS_LEN_MAX", p_);
        if (channels * p_ * p_ > (size_t)YAGI_EQRLS_MATRIX_MAX)
            return fail(YAGI_ERR_CONFIG, "eqrls: %zu channels of %zu x %zu are more than YAGI_EQRLS_MATRIX_MAX", channels, p_, p_);
        return YAGI_OK;
    }
    int configure(size_t channels, const cf32 *h, size_t p_) {
        YG_TRY(check_design(channels, p_));
        C = channels, p = p_, lambda = 0.99f, lanes = 0;
        h0.assign(p, cf32{0.0f, 0.0f});
        if (h)
            std::copy(h, h + p, h0.begin());
        else
            h0[p - 1] = cf32{1.0f, 0.0f};
        hP.assign(p * p * C, cf32{});
        hw0.assign(p * C, cf32{});
        hw1.assign(p * C, cf32{});
        hh.assign(p * C, cf32{});
        for (size_t c = 0; c < C; ++c) reset_chan(c);
        return YAGI_OK;
    }
    static int set_bw(float l, float *lambda) {             // (:94-100)
        if (!(l >= 0.0f && l <= 1.0f)) return fail(YAGI_ERR_CONFIG, "learning rate must be in (0,1)");
        *lambda = l;
        return YAGI_OK;
    }
    static int check_lanes(size_t p, size_t L) {
        unsigned b = 0;
        while (b < 6 && ((size_t)1 << b) < L) ++b;
        if (((size_t)1 << b) != L || !(eqrls_admissible(p) >> b & 1u))
            return fail(YAGI_ERR_CONFIG, "eqrls: %zu lanes per channel are not admissible at p = %zu", L, p);
        return YAGI_OK;
    }
    // sets the rows of y
    static int check_block(size_t C, int mode, size_t k, size_t x_pitch, size_t n, bool have_d, size_t d_pitch, size_t M,
                           size_t y_pitch, size_t *rows) {
        if (mode != YAGI_EQRLS_NONE && mode != YAGI_EQRLS_TRAIN && mode != YAGI_EQRLS_DECISION)
            return fail(YAGI_ERR_CONFIG, "eqrls: unknown update mode %d", mode);
        if (k == 0) return fail(YAGI_ERR_CONFIG, "eqrls: k must be greater than 0");
        if (n >= ((size_t)1 << 31) || k >= ((size_t)1 << 31)) return fail(YAGI_ERR_CONFIG, "eqrls: n and k must be below 2^31");
        if (x_pitch < C || y_pitch < C || x_pitch >= ((size_t)1 << 31) || y_pitch >= ((size_t)1 << 31))
            return fail(YAGI_ERR_CONFIG, "eqrls: the pitches are in samples, at least the channel count and below 2^31");
        if (n % k != 0) return fail(YAGI_ERR_CONFIG, "eqrls: step_block takes whole symbols, %zu rows at k = %zu", n, k);
        *rows = n / k;
        if (mode == YAGI_EQRLS_TRAIN && *rows != 0) {
            if (!have_d) return fail(YAGI_ERR_CONFIG, "eqrls: TRAIN needs the known symbols d");
            if (d_pitch < C || d_pitch >= ((size_t)1 << 31))
                return fail(YAGI_ERR_CONFIG, "eqrls: the pitches are in samples, at least the channel count and below 2^31");
        }
        if (mode == YAGI_EQRLS_DECISION && M == 0)
            return fail(YAGI_ERR_CONFIG, "eqrls: DECISION needs set_constellation first");
        return YAGI_OK;
    }
    // c-major copies of a mirrored array of `len` rows, as the getters hand them out
    void gather(const std::vector<cf32> &a, size_t len, cf32 *out) const {
        for (size_t c = 0; c < C; ++c)
            for (size_t e = 0; e < len; ++e) out[c * len + e] = a[e * C + c];
    }
    void weights(cf32 *w) const {                           // get_weights (:148-156): w1 reversed
        for (size_t c = 0; c < C; ++c)
            for (size_t i = 0; i < p; ++i) w[c * p + i] = hw1[(p - 1 - i) * C + c];
    }
};

struct EqrlsObj : EqrlsHost, EqBankObj<EqrlsObj> {
    using Host = EqrlsHost;
    static constexpr const char *kFamily = "eqrls";
    static constexpr int kTrain = YAGI_EQRLS_TRAIN;
    DevBuf P_dev, w0_dev, w1_dev, hist_dev;

    int alloc() {
        YG_TRY(require_device());
        YG_TRY(P_dev.alloc(p * p * C * sizeof(cf32)));
        YG_TRY(w0_dev.alloc(p * C * sizeof(cf32)));
        YG_TRY(w1_dev.alloc(p * C * sizeof(cf32)));
        YG_TRY(hist_dev.alloc(p * C * sizeof(cf32)));
        YG_TRY(alloc_table());
        mirror.host_written();
        return YAGI_OK;
    }
    template <class F>
    int each_array(F &&f) {
        YG_TRY(f(P_dev, hP.data(), p * p * C * sizeof(cf32)));
        YG_TRY(f(w0_dev, hw0.data(), p * C * sizeof(cf32)));
        YG_TRY(f(w1_dev, hw1.data(), p * C * sizeof(cf32)));
        return f(hist_dev, hh.data(), p * C * sizeof(cf32));
    }
    int block_dev(int mode, size_t k, const cf32 *x, size_t x_pitch, size_t n, const cf32 *d, size_t d_pitch, cf32 *y,
                  size_t y_pitch) {
        if (n == 0) return YAGI_OK;
        YG_TRY(ensure_dev());
        YG_TRY(launch_eqrls(mode, p, lanes ? lanes : eqrls_plan(C, p), lambda, P_dev.as<cf32>(), w0_dev.as<cf32>(),
                            w1_dev.as<cf32>(), hist_dev.as<cf32>(), C, k, x, x_pitch, n, d, d_pitch, table_dev.as<cf32>(),
                            table.size(), y, y_pitch, st));
        mirror.dev_written();
        return YAGI_OK;
    }
    // train (:158-176) up to its loop: the checks, reset() and w0[i] = w[p - 1 - i], on the host mirror
    int train_prepare(const cf32 *w, size_t x_pitch, size_t n, bool have_d, size_t d_pitch) {
        if (n < p) return fail(YAGI_ERR_CONFIG, "training sequence less than filter order");
        size_t rows = 0;
        YG_TRY(check_block(C, YAGI_EQRLS_TRAIN, 1, x_pitch, n, have_d, d_pitch, 0, C, &rows));
        if (!w) return fail(YAGI_ERR_CONFIG, "null pointer argument");
        YG_TRY(reset());
        for (size_t c = 0; c < C; ++c)
            for (size_t i = 0; i < p; ++i) hw0[i * C + c] = w[c * p + (p - 1 - i)];
        return YAGI_OK;
    }
};

}  // namespace yagi

struct yagi_hip_eqrls_cccf_s : EqrlsObj {};

extern "C" {

int yagi_hip_eqrls_plan(size_t channels, size_t p, size_t *L, size_t *lds_bytes, unsigned *admissible) try {
    CHECK_PTR(L);
    YG_TRY(EqrlsHost::check_design(channels, p));
    *L = eqrls_plan(channels, p);
    if (lds_bytes) *lds_bytes = eqrls_lds_bytes(p, *L);
    if (admissible) *admissible = eqrls_admissible(p);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_create(size_t channels, const cf32 *h, size_t p, yagi_hip_eqrls_cccf *q) try {
    return bank_create(q, channels, h, p);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_recreate(yagi_hip_eqrls_cccf q, const cf32 *h, size_t p) try {
    CHECK_Q(q);
    if (p == q->p) {
        if (h) std::copy(h, h + p, q->h0.begin());
        return YAGI_OK;
    }
    YG_TRY(EqrlsHost::check_design(q->C, p));                 // the object is left as it was where the new design is refused
    YG_HIP(hipStreamSynchronize(q->st));
    YG_TRY(q->configure(q->C, h, p));
    q->mirror.in_sync();
    return q->alloc();
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_destroy(yagi_hip_eqrls_cccf q) try {
    return bank_destroy(q);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_clone(yagi_hip_eqrls_cccf q, yagi_hip_eqrls_cccf *out) try {
    return bank_clone(q, out);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_set_stream(yagi_hip_eqrls_cccf q, yagi_stream_t s) try {
    return bank_set_stream(q, s);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_reset(yagi_hip_eqrls_cccf q) try {
    CHECK_Q(q);
    return q->reset();
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_reset_channel(yagi_hip_eqrls_cccf q, size_t c) try {
    CHECK_Q(q);
    return q->reset_channel(c);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_set_bw(yagi_hip_eqrls_cccf q, float lambda) try {
    CHECK_Q(q);
    return EqrlsHost::set_bw(lambda, &q->lambda);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_get_bw(yagi_hip_eqrls_cccf q, float *lambda) try {
    return bank_get(q, lambda, [](auto &o) { return o.lambda; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_get_length(yagi_hip_eqrls_cccf q, size_t *p) try {
    return bank_get(q, p, [](auto &o) { return o.p; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_get_channels(yagi_hip_eqrls_cccf q, size_t *channels) try {
    return bank_get(q, channels, [](auto &o) { return o.C; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_get_coefficients(yagi_hip_eqrls_cccf q, cf32 *w0) try {
    CHECK_Q(q);
    CHECK_PTR(w0);
    YG_TRY(q->ensure_host());
    q->gather(q->hw0, q->p, w0);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_get_weights(yagi_hip_eqrls_cccf q, cf32 *w) try {
    CHECK_Q(q);
    CHECK_PTR(w);
    YG_TRY(q->ensure_host());
    q->weights(w);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_get_matrix(yagi_hip_eqrls_cccf q, cf32 *P0) try {
    CHECK_Q(q);
    CHECK_PTR(P0);
    YG_TRY(q->ensure_host());
    q->gather(q->hP, q->p * q->p, P0);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_set_constellation(yagi_hip_eqrls_cccf q, const cf32 *table, size_t M) try {
    CHECK_Q(q);
    return q->set_constellation(table, M);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_set_lanes(yagi_hip_eqrls_cccf q, size_t L) try {
    CHECK_Q(q);
    if (L != 0) {
        YG_TRY(EqrlsHost::check_lanes(q->p, L));
    }
    q->lanes = L;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_get_lanes(yagi_hip_eqrls_cccf q, size_t *L) try {
    return bank_get(q, L, [](auto &o) { return o.lanes ? o.lanes : eqrls_plan(o.C, o.p); });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_step_block(yagi_hip_eqrls_cccf q, size_t k, int mode, const cf32 *x, size_t x_pitch, size_t n,
                                   const cf32 *d, size_t d_pitch, cf32 *y, size_t y_pitch) try {
    CHECK_Q(q);
    return q->block_host(mode, k, x, x_pitch, n, d, d_pitch, y, y_pitch);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_step_block_dev(yagi_hip_eqrls_cccf q, size_t k, int mode, const cf32 *x_dev, size_t x_pitch, size_t n,
                                       const cf32 *d_dev, size_t d_pitch, cf32 *y_dev, size_t y_pitch) try {
    CHECK_Q(q);
    size_t rows = 0;
    YG_TRY(EqrlsHost::check_block(q->C, mode, k, x_pitch, n, d_dev != nullptr, d_pitch, q->table.size(), y_pitch, &rows));
    if (n != 0) {
        CHECK_PTR(x_dev);
        CHECK_PTR(y_dev);
    }
    return q->block_dev(mode, k, x_dev, x_pitch, n, d_dev, d_pitch, y_dev, y_pitch);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_train(yagi_hip_eqrls_cccf q, cf32 *w, const cf32 *x, size_t x_pitch, size_t n, const cf32 *d,
                              size_t d_pitch) try {
    CHECK_Q(q);
    YG_TRY(q->train_prepare(w, x_pitch, n, d != nullptr, d_pitch));
    if (n != 0) {
        CHECK_PTR(x);
        std::vector<cf32> y(n * q->C);
        YG_TRY(q->block_host(YAGI_EQRLS_TRAIN, 1, x, x_pitch, n, d, d_pitch, y.data(), q->C));
    }
    YG_TRY(q->ensure_host());
    q->weights(w);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_train_dev(yagi_hip_eqrls_cccf q, const cf32 *w, const cf32 *x_dev, size_t x_pitch, size_t n,
                                  const cf32 *d_dev, size_t d_pitch) try {
    CHECK_Q(q);
    YG_TRY(q->train_prepare(w, x_pitch, n, d_dev != nullptr, d_pitch));
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x_dev);
    YG_TRY(q->ws.y.ensure(n * q->C * sizeof(cf32)));         // the outputs are dropped
    return q->block_dev(YAGI_EQRLS_TRAIN, 1, x_dev, x_pitch, n, d_dev, d_pitch, q->ws.y.as<cf32>(), q->C);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_eqrls_cccf_execute_host(size_t channels, const cf32 *h, size_t p, float lambda, int mode, size_t k, const cf32 *x,
                                     size_t x_pitch, size_t n, const cf32 *d, size_t d_pitch, const cf32 *table, size_t M,
                                     cf32 *y, size_t y_pitch, cf32 *w0, cf32 *w1, cf32 *P0) try {
    EqrlsHost o;
    YG_TRY(o.configure(channels, h, p));
    YG_TRY(EqrlsHost::set_bw(lambda, &o.lambda));
    if (mode == YAGI_EQRLS_DECISION) {
        YG_TRY(eq_check_table(table, M));
    }
    size_t rows = 0;
    YG_TRY(EqrlsHost::check_block(channels, mode, k, x_pitch, n, d != nullptr, d_pitch, M, y_pitch, &rows));
    if (n != 0) {
        CHECK_PTR(x);
        CHECK_PTR(y);
    }
    eqrls_host(mode, p, o.lambda, o.hP.data(), o.hw0.data(), o.hw1.data(), o.hh.data(), channels, k, x, x_pitch, n, d, d_pitch,
               table, M, y, y_pitch);
    if (w0) o.gather(o.hw0, p, w0);
    if (w1) o.gather(o.hw1, p, w1);
    if (P0) o.gather(o.hP, p * p, P0);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- Agc (src/agc/agc.rs, one object per channel) ------------------------------------------------------------------
// The state is one AgcChan per channel; agc_kernels.hip updates it in place on the device.  reset, the setters and getters
// that touch g, the locks and the squelch modes work on a host mirror; the two copies are synchronised lazily (Mirror).
// alpha, scale, threshold and timeout travel to the kernel by value with every call.
namespace yagi {

// everything that needs no device
struct AgcHost {
    size_t C = 0;
    AgcSettings g;
    std::vector<AgcChan> hs;                              // host mirror

    static void reset_chan(AgcChan &s) {                  // reset (:60-69)
        s.g = 1.0f, s.y2p = 1.0f, s.locked = 0;
        s.mode = s.mode == YAGI_AGC_SQUELCH_DISABLED ? YAGI_AGC_SQUELCH_DISABLED : YAGI_AGC_SQUELCH_ENABLED;
    }
    void reset_chan(size_t c) { reset_chan(hs[c]); }
    // new (:37-58)
    int configure(size_t channels) {
        if (channels == 0 || channels > (size_t)YAGI_AGC_CHANNELS_MAX)
            return fail(YAGI_ERR_CONFIG, "agc: %zu channels are outside 1 .. YAGI_AGC_CHANNELS_MAX", channels);
        C = channels;
        g = AgcSettings{};
        AgcChan s{};
        s.mode = YAGI_AGC_SQUELCH_DISABLED;
        reset_chan(s);
        hs.assign(C, s);
        return YAGI_OK;
    }
    static int check_bandwidth(float bt) {
        if (!(bt >= 0.0f && bt <= 1.0f)) return fail(YAGI_ERR_CONFIG, "bandwidth must be in [0, 1]");
        return YAGI_OK;
    }
    static int check_positive(float v, const char *what) {
        if (!(v > 0.0f)) return fail(YAGI_ERR_CONFIG, "%s must be greater than zero", what);
        return YAGI_OK;
    }
    static int check_timeout(uint64_t t) {
        if (t == 0 || t >= ((uint64_t)1 << 32)) return fail(YAGI_ERR_CONFIG, "agc: the squelch timeout is in 1 .. 2^32 - 1");
        return YAGI_OK;
    }
    static int check_rows(size_t C, size_t x_pitch, size_t n) {
        if (n >= ((size_t)1 << 31)) return fail(YAGI_ERR_CONFIG, "agc: n must be below 2^31");
        if (x_pitch < C) return fail(YAGI_ERR_CONFIG, "agc: the pitches are in elements, at least the channel count");
        return YAGI_OK;
    }
    template <class T>
    static int check_block(size_t C, const T *x, size_t x_pitch, size_t n, const T *y, size_t y_pitch, const uint8_t *status,
                           size_t status_pitch) {
        YG_TRY(check_rows(C, x_pitch, n));
        if (y_pitch < C || (status && status_pitch < C))
            return fail(YAGI_ERR_CONFIG, "agc: the pitches are in elements, at least the channel count");
        if (n == 0) return YAGI_OK;
        if (!x || !y) return fail(YAGI_ERR_CONFIG, "null pointer argument");
        const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y, sa = (uintptr_t)status;
        const uintptr_t xe = xa + ((n - 1) * x_pitch + C) * sizeof(T), ye = ya + ((n - 1) * y_pitch + C) * sizeof(T);
        const uintptr_t se = sa + (n - 1) * status_pitch + C;
        if (status && ((sa < xe && xa < se) || (sa < ye && ya < se)))
            return fail(YAGI_ERR_CONFIG, "agc: the status plane overlaps x or y");
        if (x == y && x_pitch == y_pitch) return YAGI_OK;   // in place
        if (xa < ye && ya < xe) return fail(YAGI_ERR_CONFIG, "agc: x and y overlap and are not the same block");
        return YAGI_OK;
    }
    template <class T>
    static int check_init(size_t C, const T *x, size_t x_pitch, size_t n) {
        if (n == 0) return fail(YAGI_ERR_CONFIG, "number of samples must be greater than zero");
        YG_TRY(check_rows(C, x_pitch, n));
        if (!x) return fail(YAGI_ERR_CONFIG, "null pointer argument");
        return YAGI_OK;
    }
};

template <class T>
struct AgcObj : AgcHost, BankObj<AgcObj<T>> {
    using Host = AgcHost;
    static constexpr const char *kFamily = "agc";
    DevBuf state_dev, sum_dev, stat_dev;                  // stat_dev: the status plane of the host block form

    int alloc() {
        YG_TRY(require_device());
        YG_TRY(state_dev.alloc(C * sizeof(AgcChan)));
        YG_TRY(sum_dev.alloc(C * sizeof(float)));
        this->mirror.host_written();
        return YAGI_OK;
    }
    template <class F>
    int each_array(F &&f) {
        return f(state_dev, hs.data(), C * sizeof(AgcChan));
    }
    template <class F>
    int each_chan(F &&f) {                                  // f(AgcChan &, channel) on the host mirror
        return this->edit([&] {
            for (size_t c = 0; c < C; ++c) f(hs[c], c);
        });
    }
    int block_dev(const T *x, size_t x_pitch, size_t n, T *y, size_t y_pitch, uint8_t *status, size_t status_pitch) {
        if (n == 0) return YAGI_OK;
        YG_TRY(this->ensure_dev());
        YG_TRY(launch_agc<T>(g, state_dev.as<AgcChan>(), C, x, x_pitch, n, y, y_pitch, status, status_pitch, this->st));
        this->mirror.dev_written();
        return YAGI_OK;
    }
    int block_host(const T *x, size_t x_pitch, size_t n, T *y, size_t y_pitch, uint8_t *status, size_t status_pitch) {
        Staging &ws = this->ws;
        YG_TRY(check_block(C, x, x_pitch, n, y, y_pitch, status, status_pitch));
        if (n == 0) return YAGI_OK;
        YG_TRY(ws.put(this->st, x, (n - 1) * x_pitch + C));
        YG_TRY(ws.y.ensure(n * C * sizeof(T)));
        if (status) {
            YG_TRY(stat_dev.ensure(n * C));
        }
        YG_TRY(block_dev(ws.x.as<T>(), x_pitch, n, ws.y.as<T>(), C, status ? stat_dev.as<uint8_t>() : nullptr, C));
        YG_TRY(download_rows(this->st, ws.y, n, C, y, y_pitch));
        return status ? download_rows(this->st, stat_dev, n, C, status, status_pitch) : YAGI_OK;
    }
    int init_dev(const T *x, size_t x_pitch, size_t n) {    // init (:171-178)
        YG_TRY(launch_agc_init<T>(x, x_pitch, n, C, sum_dev.as<float>(), this->st));
        std::vector<float> sum(C);
        YG_TRY(download(sum.data(), sum_dev.p, C * sizeof(float), this->st));
        return each_chan([&](AgcChan &s, size_t c) { s.g = agc_level_gain(sum[c], n), s.y2p = 1.0f; });
    }
};

}  // namespace yagi

#define YAGI_AGC_API(K, T)                                                                          \
    struct yagi_hip_agc_##K##_s : AgcObj<T> {};                                                     \
    extern "C" {                                                                                    \
    int yagi_hip_agc_##K##_create(size_t channels, yagi_hip_agc_##K *q) try {                       \
        return bank_create(q, channels);                                                            \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_destroy(yagi_hip_agc_##K q) try {                                        \
        return bank_destroy(q);                                                                     \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_clone(yagi_hip_agc_##K q, yagi_hip_agc_##K *out) try {                   \
        return bank_clone(q, out);                                                                  \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_set_stream(yagi_hip_agc_##K q, yagi_stream_t s) try {                    \
        return bank_set_stream(q, s);                                                               \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_reset(yagi_hip_agc_##K q) try {                                          \
        CHECK_Q(q);                                                                                 \
        return q->reset();                                                                          \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_reset_channel(yagi_hip_agc_##K q, size_t c) try {                        \
        CHECK_Q(q);                                                                                 \
        return q->reset_channel(c);                                                                 \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_lock(yagi_hip_agc_##K q) try {                                           \
        CHECK_Q(q);                                                                                 \
        return q->each_chan([](AgcChan &s, size_t) { s.locked = 1; });                              \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_unlock(yagi_hip_agc_##K q) try {                                         \
        CHECK_Q(q);                                                                                 \
        return q->each_chan([](AgcChan &s, size_t) { s.locked = 0; });                              \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_is_locked(yagi_hip_agc_##K q, int *locked) try {                         \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(locked);                                                                          \
        YG_TRY(q->ensure_host());                                                                   \
        *locked = 1;                                                                                \
        for (const AgcChan &s : q->hs) *locked &= s.locked ? 1 : 0;                                 \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_set_locked(yagi_hip_agc_##K q, const uint8_t *locked) try {              \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(locked);                                                                          \
        return q->each_chan([locked](AgcChan &s, size_t c) { s.locked = locked[c] ? 1 : 0; });      \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_get_locked(yagi_hip_agc_##K q, uint8_t *locked) try {                    \
        return bank_get_each(q, locked, [](auto &o, size_t c) { return o.hs[c].locked; });          \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_set_bandwidth(yagi_hip_agc_##K q, float bt) try {                        \
        CHECK_Q(q);                                                                                 \
        YG_TRY(AgcHost::check_bandwidth(bt));                                                       \
        q->g.alpha = bt;                                                                            \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_get_bandwidth(yagi_hip_agc_##K q, float *bt) try {                       \
        return bank_get(q, bt, [](auto &o) { return o.g.alpha; });                                  \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_set_scale(yagi_hip_agc_##K q, float scale) try {                         \
        CHECK_Q(q);                                                                                 \
        YG_TRY(AgcHost::check_positive(scale, "scale"));                                            \
        q->g.scale = scale;                                                                         \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_get_scale(yagi_hip_agc_##K q, float *scale) try {                        \
        return bank_get(q, scale, [](auto &o) { return o.g.scale; });                               \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_set_gain(yagi_hip_agc_##K q, float gain) try {                           \
        CHECK_Q(q);                                                                                 \
        YG_TRY(AgcHost::check_positive(gain, "gain"));                                              \
        return q->each_chan([gain](AgcChan &s, size_t) { s.g = gain; });                            \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_set_signal_level(yagi_hip_agc_##K q, float x2) try {                     \
        CHECK_Q(q);                                                                                 \
        YG_TRY(AgcHost::check_positive(x2, "signal level"));                                        \
        const float gain = 1.0f / x2;                                                               \
        return q->each_chan([gain](AgcChan &s, size_t) { s.g = gain, s.y2p = 1.0f; });              \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_set_rssi(yagi_hip_agc_##K q, float rssi) try {                           \
        CHECK_Q(q);                                                                                 \
        const float gain = agc_rssi_gain(rssi);                                                     \
        return q->each_chan([gain](AgcChan &s, size_t) { s.g = gain, s.y2p = 1.0f; });              \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_set_gains(yagi_hip_agc_##K q, const float *gain) try {                   \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(gain);                                                                            \
        for (size_t c = 0; c < q->C; ++c) YG_TRY(AgcHost::check_positive(gain[c], "gain"));         \
        return q->each_chan([gain](AgcChan &s, size_t c) { s.g = gain[c]; });                       \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_get_gain(yagi_hip_agc_##K q, float *gain) try {                          \
        return bank_get_each(q, gain, [](auto &o, size_t c) { return o.hs[c].g; });                 \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_get_signal_level(yagi_hip_agc_##K q, float *level) try {                 \
        return bank_get_each(q, level, [](auto &o, size_t c) { return 1.0f / o.hs[c].g; });         \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_get_rssi(yagi_hip_agc_##K q, float *rssi) try {                          \
        return bank_get_each(q, rssi, [](auto &o, size_t c) { return agc_rssi(o.hs[c].g); });       \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_get_channels(yagi_hip_agc_##K q, size_t *channels) try {                 \
        return bank_get(q, channels, [](auto &o) { return o.C; });                                  \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_squelch_enable(yagi_hip_agc_##K q) try {                                 \
        CHECK_Q(q);                                                                                 \
        q->g.squelch = true;                                                                        \
        return q->each_chan([](AgcChan &s, size_t) { s.mode = YAGI_AGC_SQUELCH_ENABLED; });         \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_squelch_disable(yagi_hip_agc_##K q) try {                                \
        CHECK_Q(q);                                                                                 \
        q->g.squelch = false;                                                                       \
        return q->each_chan([](AgcChan &s, size_t) { s.mode = YAGI_AGC_SQUELCH_DISABLED; });        \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_squelch_is_enabled(yagi_hip_agc_##K q, int *enabled) try {               \
        return bank_get(q, enabled, [](auto &o) { return o.g.squelch ? 1 : 0; });                   \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_squelch_set_threshold(yagi_hip_agc_##K q, float threshold) try {         \
        CHECK_Q(q);                                                                                 \
        q->g.threshold = threshold;                                                                 \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_squelch_get_threshold(yagi_hip_agc_##K q, float *threshold) try {        \
        return bank_get(q, threshold, [](auto &o) { return o.g.threshold; });                       \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_squelch_set_timeout(yagi_hip_agc_##K q, uint64_t timeout) try {          \
        CHECK_Q(q);                                                                                 \
        YG_TRY(AgcHost::check_timeout(timeout));                                                    \
        q->g.timeout = (unsigned)timeout;                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_squelch_get_timeout(yagi_hip_agc_##K q, uint64_t *timeout) try {         \
        return bank_get(q, timeout, [](auto &o) { return o.g.timeout; });                           \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_squelch_get_status(yagi_hip_agc_##K q, uint8_t *mode) try {              \
        return bank_get_each(q, mode, [](auto &o, size_t c) { return o.hs[c].mode; });              \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_init(yagi_hip_agc_##K q, const T *x, size_t x_pitch, size_t n) try {     \
        CHECK_Q(q);                                                                                 \
        YG_TRY(AgcHost::check_init(q->C, x, x_pitch, n));                                           \
        YG_TRY(q->ws.put(q->st, x, (n - 1) * x_pitch + q->C));                                      \
        return q->init_dev(q->ws.x.as<T>(), x_pitch, n);                                            \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_init_dev(yagi_hip_agc_##K q, const T *x_dev, size_t x_pitch, size_t n) try { \
        CHECK_Q(q);                                                                                 \
        YG_TRY(AgcHost::check_init(q->C, x_dev, x_pitch, n));                                       \
        return q->init_dev(x_dev, x_pitch, n);                                                      \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_execute_block(yagi_hip_agc_##K q, const T *x, size_t x_pitch, size_t n, T *y, size_t y_pitch, \
                                         uint8_t *status, size_t status_pitch) try {                \
        CHECK_Q(q);                                                                                 \
        return q->block_host(x, x_pitch, n, y, y_pitch, status, status_pitch);                      \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_execute_block_dev(yagi_hip_agc_##K q, const T *x_dev, size_t x_pitch, size_t n, T *y_dev, \
                                             size_t y_pitch, uint8_t *status_dev, size_t status_pitch) try { \
        CHECK_Q(q);                                                                                 \
        YG_TRY(AgcHost::check_block<T>(q->C, x_dev, x_pitch, n, y_dev, y_pitch, status_dev, status_pitch)); \
        return q->block_dev(x_dev, x_pitch, n, y_dev, y_pitch, status_dev, status_pitch);           \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    int yagi_hip_agc_##K##_execute_host(size_t channels, float bandwidth, float scale, float g0, int locked, int squelch, \
                                        float threshold, uint64_t timeout, const T *x, size_t x_pitch, size_t n, T *y, \
                                        size_t y_pitch, uint8_t *status, size_t status_pitch, float *g_out, \
                                        uint8_t *mode_out) try {                                    \
        AgcHost o;                                                                                  \
        YG_TRY(o.configure(channels));                                                              \
        YG_TRY(AgcHost::check_bandwidth(bandwidth));                                                \
        YG_TRY(AgcHost::check_positive(scale, "scale"));                                            \
        YG_TRY(AgcHost::check_positive(g0, "gain"));                                                \
        YG_TRY(AgcHost::check_timeout(timeout));                                                    \
        YG_TRY(AgcHost::check_block<T>(channels, x, x_pitch, n, y, y_pitch, status, status_pitch)); \
        o.g.alpha = bandwidth, o.g.scale = scale, o.g.threshold = threshold, o.g.timeout = (unsigned)timeout; \
        o.g.squelch = squelch != 0;                                                                 \
        for (AgcChan &s : o.hs) {                                                                   \
            s.g = g0, s.locked = locked ? 1 : 0;                                                    \
            s.mode = squelch ? YAGI_AGC_SQUELCH_ENABLED : YAGI_AGC_SQUELCH_DISABLED;                \
        }                                                                                           \
        agc_host<T>(o.g, o.hs.data(), channels, x, x_pitch, n, y, y_pitch, status, status_pitch);   \
        for (size_t c = 0; c < channels; ++c) {                                                     \
            if (g_out) g_out[c] = o.hs[c].g;                                                        \
            if (mode_out) mode_out[c] = o.hs[c].mode;                                               \
        }                                                                                           \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                               \
    }

YAGI_AGC_API(crcf, cf32)
YAGI_AGC_API(rrrf, float)
#undef YAGI_AGC_API

extern "C" {

int yagi_hip_lnf(const float *x, size_t n, float *y) try {
    if (n != 0) {
        CHECK_PTR(x);
        CHECK_PTR(y);
    }
    yagi::agc_words_host(0, x, n, y);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_expf(const float *x, size_t n, float *y) try {
    if (n != 0) {
        CHECK_PTR(x);
        CHECK_PTR(y);
    }
    yagi::agc_words_host(1, x, n, y);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_log10f(const float *x, size_t n, float *y) try {
    if (n != 0) {
        CHECK_PTR(x);
        CHECK_PTR(y);
    }
    yagi::agc_words_host(2, x, n, y);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- SymTrack (src/framing/symtrack.rs is empty: the composition of yagi_hip.h) ------------------------------------------
// The state is the parts' own records and arrays plus one SymtrackChan per channel; symtrack_kernels.hip updates all of
// them in place on the device.  The parts are the host structs of SymSync, EqLms and Agc (their configure(), reset and
// mirrors) as they are; the device half is SymTrack's own.  Setters that touch per-channel state, the getters and clone work on the
// host mirror; the two copies are synchronised lazily (Mirror).  The loop settings travel to the kernel by value.
namespace yagi {

// everything that needs no device; the parts are their host structs
struct SymtrackHost {
    size_t C = 0, k = 0;
    SymsyncHost sy;
    EqlmsHost eq;
    AgcHost ag;
    ModemParams P{};
    std::vector<cf32> map;
    std::vector<uint8_t> nbr;
    int vco = 0, strategy = YAGI_SYMTRACK_EQ_CM;
    std::vector<float> osc;                               // the oscillator's device table, on the host
    float pll_alpha = 0.0f, pll_beta = 0.0f, bw = 0.0f;
    uint64_t holdoff = 200;
    std::vector<SymtrackChan> hst;

    // table = nullptr takes `scheme`
    int configure(size_t channels, int ftype, size_t k_, size_t m, float beta, int scheme, const cf32 *table, size_t M,
                  int osc_scheme, size_t npfb, size_t eq_len) {
        if (channels == 0 || channels > (size_t)YAGI_SYMTRACK_CHANNELS_MAX)
            return fail(YAGI_ERR_CONFIG, "symtrack: %zu channels are outside 1 .. YAGI_SYMTRACK_CHANNELS_MAX", channels);
        int kind = 0, bps = 0;
        if (table) {
            while (bps < 8 && ((size_t)1 << bps) < M) ++bps;
            if (M < 2 || ((size_t)1 << bps) != M) return fail(YAGI_ERR_CONFIG, "table size must be a power of 2 in 2..256");
            kind = MODEM_ARB;
        } else {
            YG_TRY(yagi_hip_modem_s::kind_of(scheme, &kind, &bps));
            if (kind == MODEM_PSK || kind == MODEM_DPSK)
                return fail(YAGI_ERR_CONFIG, "symtrack: PSK and DPSK decide through atan2f / sincosf of the device library, "
                                             "which are not fixed words; they are not built");
        }
        if (osc_scheme != YAGI_OSC_NCO && osc_scheme != YAGI_OSC_VCO)
            return fail(YAGI_ERR_CONFIG, "osc: unknown scheme %d", osc_scheme);
        std::vector<float> h;
        YG_TRY(symsync_rnyquist_taps(ftype, k_, m, beta, npfb, h));
        YG_TRY(sy.configure(channels, k_, npfb, h.data(), h.size()));
        YG_TRY(sy.start_at_rate(2));
        std::vector<cf32> hc;
        YG_TRY(eqlms_lowpass_taps(eq_len, 0.45f, hc));
        YG_TRY(eq.configure(channels, hc.data(), hc.size()));
        YG_TRY(ag.configure(channels));
        YG_TRY(modem_design(kind, bps, table, P, map, nbr));
        vco = osc_scheme == YAGI_OSC_VCO;
        const size_t lds = symtrack_lds_bytes(sy.Ls, eq_len, vco, map.size());
        if (lds > kSymtrackLdsMax)
            return fail(YAGI_ERR_CONFIG, "symtrack: 2 k m = %zu and eq_len = %zu need %zu bytes of LDS, more than 160 KiB",
                        sy.Ls, eq_len, lds);
        osc_device_table(vco, osc);
        C = channels, k = k_;
        strategy = YAGI_SYMTRACK_EQ_CM, holdoff = 200;
        hst.assign(C, SymtrackChan{});
        return set_bandwidth(0.9f);
    }
    int set_bandwidths(float a, float s, float e, float pl) {
        SymsyncLoop t = sy.p;
        YG_TRY(AgcHost::check_bandwidth(a));
        YG_TRY(symsync_set_bw(s, &t));
        float mu = 0.0f;
        YG_TRY(EqlmsHost::set_bw(e, &mu));
        if (!(e >= 0.0f)) return fail(YAGI_ERR_CONFIG, "learning rate cannot be less than zero");
        if (!(pl >= 0.0f)) return fail(YAGI_ERR_CONFIG, "Bandwidth must be positive");
        ag.g.alpha = a;
        sy.p = t;
        eq.mu = mu;
        pll_alpha = pl;
        pll_beta = std::sqrt(pl);
        bw = std::nanf("");
        return YAGI_OK;
    }
    int set_bandwidth(float bw_) {
        if (!(bw_ >= 0.0f)) return fail(YAGI_ERR_CONFIG, "symtrack: the bandwidth must be at least 0");
        YG_TRY(set_bandwidths(0.02f * bw_, 0.001f * bw_, 0.02f * bw_, 0.001f * bw_));
        bw = bw_;
        return YAGI_OK;
    }
    static int check_strategy(int strategy) {
        if (strategy < YAGI_SYMTRACK_EQ_OFF || strategy > YAGI_SYMTRACK_EQ_DD)
            return fail(YAGI_ERR_CONFIG, "symtrack: unknown equalizer strategy %d", strategy);
        return YAGI_OK;
    }
    SymtrackLoop loop() const {
        SymtrackLoop p{};
        p.ss = sy.p;
        p.agc_alpha = ag.g.alpha, p.agc_scale = ag.g.scale, p.eq_mu = eq.mu, p.pll_alpha = pll_alpha, p.pll_beta = pll_beta;
        p.h_len = (unsigned)eq.h_len, p.vco = (unsigned)vco, p.strategy = (unsigned)strategy, p.M = (unsigned)map.size();
        p.kind = P.kind, p.bps = P.bps;
        p.holdoff = holdoff;
        std::copy(P.ref, P.ref + 8, p.ref);
        return p;
    }
    SymtrackState host_state() {
        return SymtrackState{ag.hs.data(), sy.hs.data(), eq.hs.data(), hst.data(), sy.hh.data(), eq.hw.data(), eq.hh.data()};
    }
    void reset_chan(size_t c) {
        ag.reset_chan(c);
        sy.reset_chan(c);
        eq.reset_chan(c);
        hst[c] = SymtrackChan{};
    }
    static int check_block(size_t C, size_t x_pitch, size_t n, size_t y_pitch, bool have_sym, size_t sym_pitch, size_t ycap) {
        if (n >= ((size_t)1 << 31) || ycap >= ((size_t)1 << 31))
            return fail(YAGI_ERR_CONFIG, "symtrack: n and ycap must be below 2^31");
        if (x_pitch < C || y_pitch < C || x_pitch >= ((size_t)1 << 31) || y_pitch >= ((size_t)1 << 31) ||
            (have_sym && (sym_pitch < C || sym_pitch >= ((size_t)1 << 31))))
            return fail(YAGI_ERR_CONFIG, "symtrack: the pitches are in elements, at least the channel count and below 2^31");
        return YAGI_OK;
    }
};

struct SymtrackObj : SymtrackHost, BankObj<SymtrackObj> {
    using Host = SymtrackHost;
    static constexpr const char *kFamily = "symtrack";
    DevBuf taps_dev, osc_dev, map_dev, agc_dev, ss_dev, eq_dev, st_dev, sshist_dev, eqw_dev, eqhist_dev, wstatus, wsym;

    SymtrackState dev_state() {
        return SymtrackState{agc_dev.as<AgcChan>(),  ss_dev.as<SymsyncChan>(), eq_dev.as<EqlmsChan>(), st_dev.as<SymtrackChan>(),
                             sshist_dev.as<cf32>(), eqw_dev.as<cf32>(),       eqhist_dev.as<cf32>()};
    }
    int alloc() {
        YG_TRY(require_device());
        YG_TRY(fill(taps_dev, sy.taps.data(), sy.taps.size() * sizeof(float), st));
        YG_TRY(fill(osc_dev, osc.data(), osc.size() * sizeof(float), st));
        std::vector<float> mr(2 * map.size() + 8);
        for (size_t i = 0; i < map.size(); ++i) mr[2 * i] = map[i].re, mr[2 * i + 1] = map[i].im;
        std::copy(P.ref, P.ref + 8, mr.begin() + 2 * map.size());
        YG_TRY(fill(map_dev, mr.data(), mr.size() * sizeof(float), st));
        YG_TRY(agc_dev.alloc(C * sizeof(AgcChan)));
        YG_TRY(ss_dev.alloc(C * sizeof(SymsyncChan)));
        YG_TRY(eq_dev.alloc(C * sizeof(EqlmsChan)));
        YG_TRY(st_dev.alloc(C * sizeof(SymtrackChan)));
        YG_TRY(sshist_dev.alloc(sy.Ls * C * sizeof(cf32)));
        YG_TRY(eqw_dev.alloc(eq.h_len * C * sizeof(cf32)));
        YG_TRY(eqhist_dev.alloc(eq.h_len * C * sizeof(cf32)));
        YG_TRY(wstatus.alloc(3 * C * sizeof(unsigned)));
        mirror.host_written();
        return YAGI_OK;
    }
    template <class F>
    int each_array(F &&f) {
        YG_TRY(f(agc_dev, ag.hs.data(), C * sizeof(AgcChan)));
        YG_TRY(f(ss_dev, sy.hs.data(), C * sizeof(SymsyncChan)));
        YG_TRY(f(eq_dev, eq.hs.data(), C * sizeof(EqlmsChan)));
        YG_TRY(f(st_dev, hst.data(), C * sizeof(SymtrackChan)));
        YG_TRY(f(sshist_dev, sy.hh.data(), sy.Ls * C * sizeof(cf32)));
        YG_TRY(f(eqw_dev, eq.hw.data(), eq.h_len * C * sizeof(cf32)));
        return f(eqhist_dev, eq.hh.data(), eq.h_len * C * sizeof(cf32));
    }
    // the words of set_frequency / set_phase for channels [c0, c0 + count): nothing changes where one of them fails
    int set_nco(size_t c0, size_t count, const float *frequency, const float *phase) {
        std::vector<uint32_t> w(2 * count);
        for (size_t i = 0; i < count; ++i) {
            YG_TRY(osc_constrain(frequency[i], &w[2 * i]));
            YG_TRY(osc_constrain(phase[i], &w[2 * i + 1]));
        }
        return edit([&] {
            for (size_t i = 0; i < count; ++i) hst[c0 + i].d_theta = w[2 * i], hst[c0 + i].theta = w[2 * i + 1];
        });
    }
    int block_dev(const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch, uint8_t *sym, size_t sym_pitch,
                  size_t ycap, unsigned *status) {
        YG_TRY(ensure_dev());
        YG_TRY(launch_symtrack(loop(), taps_dev.as<float>(), osc_dev.p, map_dev.as<cf32>(), dev_state(), C, x, x_pitch, n, y,
                               y_pitch, sym, sym_pitch, ycap, status, st));
        mirror.dev_written();
        return YAGI_OK;
    }
};

}  // namespace yagi

struct yagi_hip_symtrack_cccf_s : SymtrackObj {};

extern "C" {

int yagi_hip_symtrack_cccf_create(size_t channels, int ftype, size_t k, size_t m, float beta, int scheme, int osc_scheme,
                                  size_t npfb, size_t eq_len, yagi_hip_symtrack_cccf *q) try {
    return bank_create(q, channels, ftype, k, m, beta, scheme, (const cf32 *)nullptr, (size_t)0, osc_scheme, npfb, eq_len);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_create_from_table(size_t channels, int ftype, size_t k, size_t m, float beta, const cf32 *table,
                                             size_t M, int osc_scheme, size_t npfb, size_t eq_len,
                                             yagi_hip_symtrack_cccf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    CHECK_PTR(table);
    return bank_create(q, channels, ftype, k, m, beta, (int)YAGI_MODEM_ARB, table, M, osc_scheme, npfb, eq_len);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_destroy(yagi_hip_symtrack_cccf q) try {
    return bank_destroy(q);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_clone(yagi_hip_symtrack_cccf q, yagi_hip_symtrack_cccf *out) try {
    return bank_clone(q, out);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_set_stream(yagi_hip_symtrack_cccf q, yagi_stream_t s) try {
    return bank_set_stream(q, s);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_reset(yagi_hip_symtrack_cccf q) try {
    CHECK_Q(q);
    return q->reset();
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_reset_channel(yagi_hip_symtrack_cccf q, size_t c) try {
    CHECK_Q(q);
    return q->reset_channel(c);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_set_bandwidth(yagi_hip_symtrack_cccf q, float bw) try {
    CHECK_Q(q);
    return q->set_bandwidth(bw);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_get_bandwidth(yagi_hip_symtrack_cccf q, float *bw) try {
    return bank_get(q, bw, [](auto &o) { return o.bw; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_set_bandwidths(yagi_hip_symtrack_cccf q, float agc, float sync, float eq, float pll) try {
    CHECK_Q(q);
    return q->set_bandwidths(agc, sync, eq, pll);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_set_eq_strategy(yagi_hip_symtrack_cccf q, int strategy) try {
    CHECK_Q(q);
    YG_TRY(SymtrackHost::check_strategy(strategy));
    q->strategy = strategy;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_set_eq_holdoff(yagi_hip_symtrack_cccf q, uint64_t nsyms) try {
    CHECK_Q(q);
    q->holdoff = nsyms;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_set_nco(yagi_hip_symtrack_cccf q, size_t c, float frequency, float phase) try {
    CHECK_Q(q);
    if (c >= q->C) return fail(YAGI_ERR_CONFIG, "symtrack: channel %zu of %zu", c, q->C);
    return q->set_nco(c, 1, &frequency, &phase);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_set_nco_all(yagi_hip_symtrack_cccf q, const float *frequency, const float *phase) try {
    CHECK_Q(q);
    CHECK_PTR(frequency);
    CHECK_PTR(phase);
    return q->set_nco(0, q->C, frequency, phase);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_get_channels(yagi_hip_symtrack_cccf q, size_t *channels) try {
    return bank_get(q, channels, [](auto &o) { return o.C; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_get_tau(yagi_hip_symtrack_cccf q, float *tau) try {
    return bank_get_each(q, tau, [](auto &o, size_t c) { return o.sy.hs[c].tau_decim; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_get_gain(yagi_hip_symtrack_cccf q, float *gain) try {
    return bank_get_each(q, gain, [](auto &o, size_t c) { return o.ag.hs[c].g; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_get_rssi(yagi_hip_symtrack_cccf q, float *rssi) try {
    return bank_get_each(q, rssi, [](auto &o, size_t c) { return agc_rssi(o.ag.hs[c].g); });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_get_nco_frequency(yagi_hip_symtrack_cccf q, float *frequency) try {
    return bank_get_each(q, frequency, [](auto &o, size_t c) { return osc_frequency(o.hst[c].d_theta); });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_get_nco_phase(yagi_hip_symtrack_cccf q, float *phase) try {
    return bank_get_each(q, phase, [](auto &o, size_t c) { return osc_phase(o.hst[c].theta); });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_get_num_syms(yagi_hip_symtrack_cccf q, uint64_t *num_syms) try {
    return bank_get_each(q, num_syms, [](auto &o, size_t c) { return (uint64_t)o.hst[c].num_syms; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_get_stalled(yagi_hip_symtrack_cccf q, uint32_t *stalled) try {
    return bank_get_each(q, stalled, [](auto &o, size_t c) { return o.hst[c].stall; });
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_get_nco_state(yagi_hip_symtrack_cccf q, uint32_t *theta, uint32_t *d_theta) try {
    CHECK_Q(q);
    CHECK_PTR(theta);
    CHECK_PTR(d_theta);
    YG_TRY(q->ensure_host());
    for (size_t c = 0; c < q->C; ++c) theta[c] = q->hst[c].theta, d_theta[c] = q->hst[c].d_theta;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_get_weights(yagi_hip_symtrack_cccf q, cf32 *w) try {
    CHECK_Q(q);
    CHECK_PTR(w);
    YG_TRY(q->ensure_host());
    q->eq.weights(w);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_execute_dev(yagi_hip_symtrack_cccf q, const cf32 *x_dev, size_t x_pitch, size_t n, cf32 *y_dev,
                                       size_t y_pitch, uint8_t *sym_dev, size_t sym_pitch, size_t ycap,
                                       uint32_t *status_dev) try {
    CHECK_Q(q);
    CHECK_PTR(status_dev);
    YG_TRY(SymtrackHost::check_block(q->C, x_pitch, n, y_pitch, sym_dev != nullptr, sym_pitch, ycap));
    if (n != 0) CHECK_PTR(x_dev);
    if (ycap != 0) CHECK_PTR(y_dev);
    return q->block_dev(x_dev, x_pitch, n, y_dev, y_pitch, sym_dev, sym_pitch, ycap, status_dev);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_execute(yagi_hip_symtrack_cccf q, const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch,
                                   uint8_t *sym, size_t sym_pitch, size_t ycap, uint32_t *ny, uint32_t *stalled) try {
    CHECK_Q(q);
    CHECK_PTR(ny);
    CHECK_PTR(stalled);
    const size_t C = q->C;
    YG_TRY(SymtrackHost::check_block(C, x_pitch, n, y_pitch, sym != nullptr, sym_pitch, ycap));
    if (n != 0) CHECK_PTR(x);
    if (ycap != 0) CHECK_PTR(y);
    const size_t nx = n ? (n - 1) * x_pitch + C : 0;
    YG_TRY(q->ws.put(q->st, x, nx));
    YG_TRY(q->ws.y.ensure(ycap * C * sizeof(cf32)));
    if (sym) YG_TRY(q->wsym.ensure(ycap * C));
    YG_TRY(q->block_dev(q->ws.x.as<cf32>(), x_pitch, n, q->ws.y.as<cf32>(), C, sym ? q->wsym.as<uint8_t>() : nullptr, C, ycap,
                        q->wstatus.as<unsigned>()));
    return q->fetch_ragged(q->wstatus, 3 * C, ny, stalled, y, y_pitch, &q->wsym, sym, sym_pitch);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symtrack_cccf_execute_host(size_t channels, int ftype, size_t k, size_t m, float beta, int scheme,
                                        const cf32 *table, size_t M, int osc_scheme, size_t npfb, size_t eq_len, float bw,
                                        int strategy, uint64_t holdoff, const float *nco_frequency, const float *nco_phase,
                                        const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch, uint8_t *sym,
                                        size_t sym_pitch, size_t ycap, uint32_t *ny, uint32_t *stalled) try {
    CHECK_PTR(ny);
    CHECK_PTR(stalled);
    SymtrackHost o;
    YG_TRY(o.configure(channels, ftype, k, m, beta, scheme, table, M, osc_scheme, npfb, eq_len));
    YG_TRY(o.set_bandwidth(bw));
    YG_TRY(SymtrackHost::check_strategy(strategy));
    o.strategy = strategy, o.holdoff = holdoff;
    for (size_t c = 0; c < channels; ++c) {
        if (nco_frequency) YG_TRY(osc_constrain(nco_frequency[c], &o.hst[c].d_theta));
        if (nco_phase) YG_TRY(osc_constrain(nco_phase[c], &o.hst[c].theta));
    }
    YG_TRY(SymtrackHost::check_block(channels, x_pitch, n, y_pitch, sym != nullptr, sym_pitch, ycap));
    if (n != 0) CHECK_PTR(x);
    if (ycap != 0) CHECK_PTR(y);
    std::vector<unsigned> status(3 * channels);
    symtrack_host(o.loop(), o.sy.taps.data(), o.osc.data(), o.map.data(), o.host_state(), channels, x, x_pitch, n, y, y_pitch,
                  sym, sym_pitch, ycap, status.data());
    for (size_t c = 0; c < channels; ++c) ny[c] = status[c], stalled[c] = status[channels + c];
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- Channel (yagi_hip.h; src/channel/mod.rs is empty) ---------------------------------------------------------------
// Every parameter is the host's: one ChannelLink per link as of the last parameter change plus `adv`, the samples
// executed since, so a block call passes adv by value and advances it at once, as Osc does with theta, and nothing is
// ever read back for them.  Only the carried window ([L - 1][C], ping-pong: channel_kernels.hip writes the next one) is
// the device's; reset, reset_channel and clone reach it through a host mirror (Mirror).
namespace yagi {

// everything that needs no device
struct ChannelHost {
    size_t C = 0, L = 0;
    int vco = 0;
    uint64_t seed = 0, adv = 0;
    ChannelShape forced{0, 0};                              // set_shape; cw = 0: the planner's
    std::vector<ChannelLink> link;                          // as of adv = 0
    std::vector<uint32_t> phi;                              // the phase word last set: where reset puts theta
    std::vector<cf32> hrev, hwin;                           // [L][C] taps, reversed; [L - 1][C] window mirror

    static int check_create(size_t channels, size_t taps, int scheme) {
        if (channels == 0 || channels > (size_t)YAGI_CHANNEL_CHANNELS_MAX)
            return fail(YAGI_ERR_CONFIG, "channel: %zu channels are outside 1 .. YAGI_CHANNEL_CHANNELS_MAX", channels);
        if (taps == 0 || taps > (size_t)YAGI_CHANNEL_TAPS_MAX)
            return fail(YAGI_ERR_CONFIG, "channel: %zu taps are outside 1 .. YAGI_CHANNEL_TAPS_MAX", taps);
        if (scheme != YAGI_OSC_NCO && scheme != YAGI_OSC_VCO) return fail(YAGI_ERR_CONFIG, "osc: unknown scheme %d", scheme);
        return YAGI_OK;
    }
    int configure(size_t channels, size_t taps, int scheme) {
        YG_TRY(check_create(channels, taps, scheme));
        C = channels, L = taps, vco = scheme == YAGI_OSC_VCO;
        link.assign(C, ChannelLink{1.0f, 0.0f, 0u, 0u, 0ull});
        phi.assign(C, 0u);
        hrev.assign(L * C, cf32{0.0f, 0.0f});
        for (size_t c = 0; c < C; ++c) hrev[(L - 1) * C + c] = cf32{1.0f, 0.0f};      // h = (1, 0, .., 0)
        hwin.assign((L - 1) * C, cf32{0.0f, 0.0f});
        return YAGI_OK;
    }
    void fold() {                                           // bring the words of every link to the present: adv = 0
        if (adv != 0)
            for (ChannelLink &k : link) {
                k.theta += (uint32_t)adv * k.d_theta;
                k.t += adv;
            }
        adv = 0;
    }
    int check_link(size_t c) const {
        if (c >= C) return fail(YAGI_ERR_CONFIG, "channel: link %zu of %zu", c, C);
        return YAGI_OK;
    }
    void reset_link(size_t c) {
        link[c].theta = phi[c];
        link[c].t = 0;
        for (size_t j = 0; j + 1 < L; ++j) hwin[j * C + c] = cf32{0.0f, 0.0f};
    }
    ChannelShape shape(size_t n) const { return forced.cw ? forced : channel_plan(C, L, n); }
    static int check_block(size_t C, bool bcast, const cf32 *x, size_t x_pitch, size_t n, const cf32 *y, size_t y_pitch) {
        if (n >= ((size_t)1 << 31)) return fail(YAGI_ERR_CONFIG, "channel: n must be below 2^31");
        if ((!bcast && x_pitch < C) || y_pitch < C)
            return fail(YAGI_ERR_CONFIG, "channel: the pitches are in elements, at least the channel count");
        if (n == 0) return YAGI_OK;
        if (!x || !y) return fail(YAGI_ERR_CONFIG, "null pointer argument");
        const size_t nx = bcast ? n : (n - 1) * x_pitch + C, ny = (n - 1) * y_pitch + C;
        return check_noalias(x, nx * sizeof(cf32), y, ny * sizeof(cf32));
    }
    void put_taps(size_t c, const cf32 *h) {               // hrev_c[j] = h_c[L - 1 - j]
        for (size_t j = 0; j < L; ++j) hrev[j * C + c] = h[L - 1 - j];
    }
    static void fill_shape(ChannelShape s, size_t taps, int vco, bool bcast, yagi_hip_channel_shape *out) {
        out->links = s.cw, out->rows = s.rows;
        out->tile_steps = channel_tile_steps(s);
        out->lds_bytes = channel_lds_bytes(s, taps, vco, bcast);
    }
};

// Not a BankObj: the links and taps go up by dirty flag, not through the mirror, the window is a ping-pong pair, and a
// full reset rewrites both copies of it without a download.
struct ChannelObj : ChannelHost {
    using Host = ChannelHost;
    hipStream_t st = nullptr;
    DevBuf tab, link_dev, taps_dev;
    PingPong<> win;
    bool link_dirty = true, taps_dirty = true;
    Mirror mirror;
    Staging ws;

    int alloc() {
        YG_TRY(require_device());
        std::vector<float> h;
        osc_device_table(vco, h);
        YG_TRY(fill(tab, h.data(), h.size() * sizeof(float), st));
        YG_TRY(link_dev.alloc(C * sizeof(ChannelLink)));
        YG_TRY(taps_dev.alloc(L * C * sizeof(cf32)));
        YG_TRY(win.alloc((L - 1) * C * sizeof(cf32)));
        link_dirty = taps_dirty = true;
        mirror.in_sync();
        mirror.host_written();
        return YAGI_OK;
    }
    int ensure_host() {
        return mirror.need_host([&] { return download(hwin.data(), win.cur(), hwin.size() * sizeof(cf32), st); });
    }
    int ensure_dev() {
        if (link_dirty) YG_TRY(upload(link_dev.p, link.data(), C * sizeof(ChannelLink), st));
        if (taps_dirty) YG_TRY(upload(taps_dev.p, hrev.data(), hrev.size() * sizeof(cf32), st));
        link_dirty = taps_dirty = false;
        return mirror.need_dev([&] { return upload(win.cur(), hwin.data(), hwin.size() * sizeof(cf32), st); });
    }
    void fold() {                                           // whoever folds goes on to change a link
        Host::fold();
        link_dirty = true;
    }
    void put_taps(size_t c, const cf32 *h) {
        Host::put_taps(c, h);
        taps_dirty = true;
    }
    int reset(size_t first, size_t count) {
        if (count == C) {                                   // both copies of the window are rewritten: no download
            mirror.in_sync();
        } else {
            YG_TRY(ensure_host());
        }
        fold();
        for (size_t c = first; c < first + count; ++c) reset_link(c);
        mirror.host_written();
        return YAGI_OK;
    }
    int block_dev(bool bcast, const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch) {
        if (n == 0) return YAGI_OK;
        if (((uintptr_t)x | (uintptr_t)y) & 7) return fail(YAGI_ERR_CONFIG, "channel: sample buffers must be 8-byte aligned");
        YG_TRY(ensure_dev());
        YG_TRY(launch_channel(shape(n), vco, bcast, tab.p, link_dev.as<ChannelLink>(), taps_dev.as<cf32>(), win.cur<cf32>(),
                              win.next<cf32>(), seed, adv, C, L, x, x_pitch, n, y, y_pitch, st));
        if (L > 1) {
            win.flip();
            mirror.dev_written();
        }
        adv += n;
        return YAGI_OK;
    }
    int block_host(bool bcast, const cf32 *x, size_t x_pitch, size_t n, cf32 *y, size_t y_pitch) {
        YG_TRY(check_block(C, bcast, x, x_pitch, n, y, y_pitch));
        if (n == 0) return YAGI_OK;
        YG_TRY(ws.put(st, x, bcast ? n : (n - 1) * x_pitch + C));
        YG_TRY(ws.y.ensure(n * C * sizeof(cf32)));
        YG_TRY(block_dev(bcast, ws.x.as<cf32>(), x_pitch, n, ws.y.as<cf32>(), C));
        return download_rows(st, ws.y, n, C, y, y_pitch);
    }
};

}  // namespace yagi

struct yagi_hip_channel_cccf_s : ChannelObj {};

extern "C" {

int yagi_hip_channel_plan(size_t channels, size_t L, size_t n, int osc_scheme, int bcast, yagi_hip_channel_shape *plan) try {
    CHECK_PTR(plan);
    YG_TRY(ChannelHost::check_create(channels, L, osc_scheme));
    if (n >= ((size_t)1 << 31)) return fail(YAGI_ERR_CONFIG, "channel: n must be below 2^31");
    ChannelHost::fill_shape(channel_plan(channels, L, n), L, osc_scheme == YAGI_OSC_VCO, bcast != 0, plan);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_create(size_t channels, size_t L, int osc_scheme, yagi_hip_channel_cccf *q) try {
    return bank_create(q, channels, L, osc_scheme);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_destroy(yagi_hip_channel_cccf q) try {
    return bank_destroy(q);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_clone(yagi_hip_channel_cccf q, yagi_hip_channel_cccf *out) try {
    return bank_clone(q, out);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_set_stream(yagi_hip_channel_cccf q, yagi_stream_t s) try {
    return bank_set_stream(q, s);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_reset(yagi_hip_channel_cccf q) try {
    CHECK_Q(q);
    return q->reset(0, q->C);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_reset_channel(yagi_hip_channel_cccf q, size_t c) try {
    CHECK_Q(q);
    YG_TRY(q->check_link(c));
    return q->reset(c, 1);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_set_awgn(yagi_hip_channel_cccf q, size_t c, float n0_db, float snr_db) try {
    CHECK_Q(q);
    YG_TRY(q->check_link(c));
    channel_awgn_words(n0_db, snr_db, &q->link[c].gamma, &q->link[c].nstd);
    q->link_dirty = true;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_set_awgn_all(yagi_hip_channel_cccf q, const float *n0_db, const float *snr_db) try {
    CHECK_Q(q);
    CHECK_PTR(n0_db);
    CHECK_PTR(snr_db);
    for (size_t c = 0; c < q->C; ++c) channel_awgn_words(n0_db[c], snr_db[c], &q->link[c].gamma, &q->link[c].nstd);
    q->link_dirty = true;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_set_gain_noise(yagi_hip_channel_cccf q, size_t c, float gamma, float nstd) try {
    CHECK_Q(q);
    YG_TRY(q->check_link(c));
    q->link[c].gamma = gamma, q->link[c].nstd = nstd;
    q->link_dirty = true;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_set_gain_noise_all(yagi_hip_channel_cccf q, const float *gamma, const float *nstd) try {
    CHECK_Q(q);
    CHECK_PTR(gamma);
    CHECK_PTR(nstd);
    for (size_t c = 0; c < q->C; ++c) q->link[c].gamma = gamma[c], q->link[c].nstd = nstd[c];
    q->link_dirty = true;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_set_carrier_offset(yagi_hip_channel_cccf q, size_t c, float dphi, float phi) try {
    CHECK_Q(q);
    YG_TRY(q->check_link(c));
    uint32_t df = 0, ph = 0;
    YG_TRY(osc_constrain(dphi, &df));                       // both words first: no half update
    YG_TRY(osc_constrain(phi, &ph));
    q->fold();
    q->link[c].d_theta = df, q->link[c].theta = ph, q->phi[c] = ph;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_set_carrier_offset_all(yagi_hip_channel_cccf q, const float *dphi, const float *phi) try {
    CHECK_Q(q);
    CHECK_PTR(dphi);
    CHECK_PTR(phi);
    std::vector<uint32_t> w(2 * q->C);
    for (size_t c = 0; c < q->C; ++c) {
        YG_TRY(osc_constrain(dphi[c], &w[2 * c]));
        YG_TRY(osc_constrain(phi[c], &w[2 * c + 1]));
    }
    q->fold();
    for (size_t c = 0; c < q->C; ++c) q->link[c].d_theta = w[2 * c], q->link[c].theta = q->phi[c] = w[2 * c + 1];
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_set_multipath(yagi_hip_channel_cccf q, size_t c, const yagi_cf32 *h) try {
    CHECK_Q(q);
    CHECK_PTR(h);
    YG_TRY(q->check_link(c));
    q->put_taps(c, h);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_set_multipath_all(yagi_hip_channel_cccf q, const yagi_cf32 *h) try {
    CHECK_Q(q);
    CHECK_PTR(h);
    for (size_t c = 0; c < q->C; ++c) q->put_taps(c, h + c * q->L);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_get_multipath(yagi_hip_channel_cccf q, yagi_cf32 *h) try {
    CHECK_Q(q);
    CHECK_PTR(h);
    for (size_t c = 0; c < q->C; ++c)
        for (size_t j = 0; j < q->L; ++j) h[c * q->L + j] = q->hrev[(q->L - 1 - j) * q->C + c];
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_set_seed(yagi_hip_channel_cccf q, uint64_t seed) try {
    CHECK_Q(q);
    q->seed = seed;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_get_seed(yagi_hip_channel_cccf q, uint64_t *seed) try {
    return bank_get(q, seed, [](auto &o) { return o.seed; });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_set_position(yagi_hip_channel_cccf q, size_t c, uint64_t t) try {
    CHECK_Q(q);
    YG_TRY(q->check_link(c));
    q->fold();
    q->link[c].t = t;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_set_position_all(yagi_hip_channel_cccf q, const uint64_t *t) try {
    CHECK_Q(q);
    CHECK_PTR(t);
    q->fold();
    for (size_t c = 0; c < q->C; ++c) q->link[c].t = t[c];
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_get_position(yagi_hip_channel_cccf q, uint64_t *t) try {
    CHECK_Q(q);
    CHECK_PTR(t);
    for (size_t c = 0; c < q->C; ++c) t[c] = q->link[c].t + q->adv;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_get_gain_noise(yagi_hip_channel_cccf q, float *gamma, float *nstd) try {
    CHECK_Q(q);
    for (size_t c = 0; c < q->C; ++c) {
        if (gamma) gamma[c] = q->link[c].gamma;
        if (nstd) nstd[c] = q->link[c].nstd;
    }
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_get_osc_state(yagi_hip_channel_cccf q, uint32_t *theta, uint32_t *d_theta) try {
    CHECK_Q(q);
    for (size_t c = 0; c < q->C; ++c) {
        if (theta) theta[c] = q->link[c].theta + (uint32_t)q->adv * q->link[c].d_theta;
        if (d_theta) d_theta[c] = q->link[c].d_theta;
    }
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_get_channels(yagi_hip_channel_cccf q, size_t *channels) try {
    return bank_get(q, channels, [](auto &o) { return o.C; });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_get_taps(yagi_hip_channel_cccf q, size_t *L) try {
    return bank_get(q, L, [](auto &o) { return o.L; });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_set_shape(yagi_hip_channel_cccf q, unsigned links, unsigned rows) try {
    CHECK_Q(q);
    if (links == 0 && rows == 0) {
        q->forced = ChannelShape{0, 0};
        return YAGI_OK;
    }
    if (!channel_shape_ok(ChannelShape{links, rows}))
        return fail(YAGI_ERR_CONFIG, "channel: the shape (%u links, %u rows) is not admissible", links, rows);
    q->forced = ChannelShape{links, rows};
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_get_shape(yagi_hip_channel_cccf q, size_t n, int bcast, yagi_hip_channel_shape *shape) try {
    CHECK_Q(q);
    CHECK_PTR(shape);
    ChannelHost::fill_shape(q->shape(n), q->L, q->vco, bcast != 0, shape);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_execute(yagi_hip_channel_cccf q, const yagi_cf32 *x, size_t x_pitch, size_t n, yagi_cf32 *y,
                                  size_t y_pitch) try {
    CHECK_Q(q);
    return q->block_host(false, x, x_pitch, n, y, y_pitch);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_execute_dev(yagi_hip_channel_cccf q, const yagi_cf32 *x_dev, size_t x_pitch, size_t n,
                                      yagi_cf32 *y_dev, size_t y_pitch) try {
    CHECK_Q(q);
    YG_TRY(ChannelHost::check_block(q->C, false, x_dev, x_pitch, n, y_dev, y_pitch));
    return q->block_dev(false, x_dev, x_pitch, n, y_dev, y_pitch);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_execute_bcast(yagi_hip_channel_cccf q, const yagi_cf32 *x, size_t n, yagi_cf32 *y,
                                        size_t y_pitch) try {
    CHECK_Q(q);
    return q->block_host(true, x, 0, n, y, y_pitch);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_execute_bcast_dev(yagi_hip_channel_cccf q, const yagi_cf32 *x_dev, size_t n, yagi_cf32 *y_dev,
                                            size_t y_pitch) try {
    CHECK_Q(q);
    YG_TRY(ChannelHost::check_block(q->C, true, x_dev, 0, n, y_dev, y_pitch));
    return q->block_dev(true, x_dev, 0, n, y_dev, y_pitch);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cccf_execute_host(size_t channels, size_t L, int osc_scheme, int bcast, uint64_t seed, const yagi_cf32 *h,
                                       const float *gamma, const float *nstd, const uint32_t *theta, const uint32_t *d_theta,
                                       const uint64_t *t, const yagi_cf32 *x, size_t x_pitch, size_t n, yagi_cf32 *y,
                                       size_t y_pitch) try {
    ChannelHost o;
    YG_TRY(o.configure(channels, L, osc_scheme));
    CHECK_PTR(h);
    CHECK_PTR(gamma);
    CHECK_PTR(nstd);
    CHECK_PTR(theta);
    CHECK_PTR(d_theta);
    CHECK_PTR(t);
    YG_TRY(ChannelHost::check_block(channels, bcast != 0, x, x_pitch, n, y, y_pitch));
    for (size_t c = 0; c < channels; ++c) {
        o.put_taps(c, h + c * L);
        o.link[c] = ChannelLink{gamma[c], nstd[c], theta[c], d_theta[c], t[c]};
    }
    std::vector<float> tab;
    osc_device_table(o.vco, tab);
    channel_host(o.vco, bcast != 0, tab.data(), o.link.data(), o.hrev.data(), seed, channels, L, x, x_pitch, n, y, y_pitch);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_awgn_words(float n0_db, float snr_db, float *gamma, float *nstd) try {
    CHECK_PTR(gamma);
    CHECK_PTR(nstd);
    channel_awgn_words(n0_db, snr_db, gamma, nstd);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_cos_sin(const uint32_t *k2, size_t n, double *c, double *s) try {
    if (n == 0) return YAGI_OK;
    CHECK_PTR(k2);
    CHECK_PTR(c);
    CHECK_PTR(s);
    channel_cos_sin_host(k2, n, c, s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_radius(const uint32_t *k1, size_t n, float *r) try {
    if (n == 0) return YAGI_OK;
    CHECK_PTR(k1);
    CHECK_PTR(r);
    for (size_t i = 0; i < n; ++i)
        if (k1[i] < 1 || k1[i] > (1u << 24)) return fail(YAGI_ERR_CONFIG, "channel: k1 is in 1 .. 2^24");
    channel_radius_host(k1, n, r);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_noise(uint64_t seed, uint64_t link, uint64_t first, size_t n, yagi_cf32 *out) try {
    if (n == 0) return YAGI_OK;
    CHECK_PTR(out);
    channel_noise_host(seed, link, first, n, out);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_channel_constrain(float phi, uint32_t *word) try {
    CHECK_PTR(word);
    return osc_constrain(phi, word);
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- ConvCode (yagi_hip.h; src/fec/mod.rs is empty) ------------------------------------------------------------------
// No call carries state: the object is the code, its puncture table on the device and the staging of the host forms, so
// there is no mirror and it is not a BankObj.
namespace yagi {

// everything that needs no device
struct ConvHost : ConvCode {
    ConvShape forced{0, 0};                                 // set_shape; fpw = 0: the planner's

    static int check_K(int K_) {
        if (K_ < 3 || K_ > 9) return fail(YAGI_ERR_CONFIG, "convcode: the constraint length %d is outside 3 .. 9", K_);
        return YAGI_OK;
    }
    int configure(int K_, const unsigned *g_, int R_, const uint8_t *puncture, int p_, int terminated_) {
        YG_TRY(check_K(K_));
        if (R_ < 2 || R_ > 4) return fail(YAGI_ERR_CONFIG, "convcode: %d generators are outside 2 .. 4", R_);
        if (!g_) return fail(YAGI_ERR_CONFIG, "null pointer argument");
        for (int r = 0; r < R_; ++r)
            if (g_[r] == 0 || g_[r] >= (1u << K_))
                return fail(YAGI_ERR_CONFIG, "convcode: generator %d (0x%x) is outside 1 .. 2^%d - 1", r, g_[r], K_);
        if (!puncture) p_ = 1;
        if (p_ < 1 || p_ > YAGI_CONVCODE_PERIOD_MAX)
            return fail(YAGI_ERR_CONFIG, "convcode: the puncture period %d is outside 1 .. YAGI_CONVCODE_PERIOD_MAX", p_);
        K = K_, R = R_, p = p_, terminated = terminated_ != 0, kp = 0;
        for (int r = 0; r < 4; ++r) g[r] = r < R ? g_[r] : 0u;
        for (int j = 0; j < YAGI_CONVCODE_PERIOD_MAX; ++j) off[j] = keep[j] = 0;
        for (int j = 0; j < p; ++j) {
            for (int r = 0; r < R; ++r) {
                const unsigned v = puncture ? puncture[(size_t)r * p + j] : 1u;
                if (v > 1) return fail(YAGI_ERR_CONFIG, "convcode: the puncture matrix holds 0 and 1 only");
                off[j] |= kp << (8 * r);
                keep[j] |= v << r;
                kp += v;
            }
            for (int r = R; r < 4; ++r) off[j] |= kp << (8 * r);
            if (keep[j] == 0) return fail(YAGI_ERR_CONFIG, "convcode: puncture column %d keeps no bit", j);
        }
        return YAGI_OK;
    }
    int check_n(size_t n) const {
        if (n == 0) return fail(YAGI_ERR_CONFIG, "convcode: a frame holds at least one bit");
        if (n > nmax())
            return fail(YAGI_ERR_CONFIG,
                        "convcode: %zu bits are more than %zu: the decisions of a frame fit YAGI_CONVCODE_DECISION_BYTES and its "
                        "steps YAGI_CONVCODE_STEPS_MAX", n, nmax());
        return YAGI_OK;
    }
    // rows of a bytes in, rows of b bytes out (and F metric words): the pitches, the pointers and the overlaps
    int check_block(size_t n, size_t F, const void *in, size_t in_pitch, size_t a, const void *out, size_t out_pitch, size_t b,
                    const uint32_t *metric) const {
        YG_TRY(check_n(n));
        if (F > (size_t)YAGI_CONVCODE_FRAMES_MAX) return fail(YAGI_ERR_CONFIG, "convcode: %zu frames are more than YAGI_CONVCODE_FRAMES_MAX", F);
        if (in_pitch < a || out_pitch < b)
            return fail(YAGI_ERR_CONFIG, "convcode: the pitches are in bytes, at least the row length (%zu in, %zu out)", a, b);
        if (F == 0) return YAGI_OK;
        if (!in || !out) return fail(YAGI_ERR_CONFIG, "null pointer argument");
        const size_t nin = (F - 1) * in_pitch + a, nout = (F - 1) * out_pitch + b;
        YG_TRY(check_noalias(in, nin, out, nout));
        if (metric) {
            if ((uintptr_t)metric & 3) return fail(YAGI_ERR_CONFIG, "convcode: the metric words are 4-byte aligned");
            YG_TRY(check_noalias(in, nin, metric, F * sizeof(uint32_t)));
            YG_TRY(check_noalias(out, nout, metric, F * sizeof(uint32_t)));
        }
        return YAGI_OK;
    }
    ConvShape shape(size_t n, size_t F) const { return forced.fpw ? forced : conv_plan(K, steps(n), F); }
    void fill_shape(ConvShape s, size_t n, yagi_hip_convcode_shape *out) const {
        out->frames_per_wave = s.fpw, out->waves = s.waves, out->states_per_lane = conv_spl(K), out->chunk_steps = conv_chunk(s);
        out->frames_per_wg = (size_t)s.fpw * s.waves;
        out->lds_bytes = conv_lds_bytes(K, s, steps(n));
    }
};

struct ConvObj : ConvHost {
    using Host = ConvHost;
    hipStream_t st = nullptr;
    DevBuf tab, wm;                                         // the puncture table; the metric words of a host call
    Staging ws;

    int alloc() {
        YG_TRY(require_device());
        uint32_t words[kConvTableWords];
        conv_table(*this, words);
        return fill(tab, words, sizeof(words), st);
    }
    int ensure_host() { return YAGI_OK; }                   // bank_clone's hook: nothing lives on the device alone
    int encode_dev(const uint8_t *msg, size_t msg_pitch, size_t n, size_t F, uint8_t *coded, size_t coded_pitch) {
        return launch_conv_encode(*this, tab.as<uint32_t>(), msg, msg_pitch, n, F, coded, coded_pitch, st);
    }
    int decode_dev(const uint8_t *soft, size_t soft_pitch, size_t n, size_t F, uint8_t *msg, size_t msg_pitch, uint32_t *metric) {
        return launch_conv_decode(*this, shape(n, F), tab.as<uint32_t>(), soft, soft_pitch, n, F, msg, msg_pitch, metric, st);
    }
};

}  // namespace yagi

struct yagi_hip_convcode_s : ConvObj {};

extern "C" {

int yagi_hip_convcode_plan(int K, int terminated, size_t n, size_t F, yagi_hip_convcode_shape *plan) try {
    CHECK_PTR(plan);
    YG_TRY(ConvHost::check_K(K));
    ConvHost o;
    o.K = K, o.terminated = terminated != 0;
    YG_TRY(o.check_n(n));
    if (F > (size_t)YAGI_CONVCODE_FRAMES_MAX) return fail(YAGI_ERR_CONFIG, "convcode: %zu frames are more than YAGI_CONVCODE_FRAMES_MAX", F);
    o.fill_shape(o.shape(n, F), n, plan);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_create(int K, const unsigned *g, int R, const uint8_t *puncture, int p, int terminated,
                             yagi_hip_convcode *q) try {
    return bank_create(q, K, g, R, puncture, p, terminated);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_destroy(yagi_hip_convcode q) try {
    return bank_destroy(q);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_clone(yagi_hip_convcode q, yagi_hip_convcode *out) try {
    return bank_clone(q, out);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_set_stream(yagi_hip_convcode q, yagi_stream_t s) try {
    return bank_set_stream(q, s);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_get_K(yagi_hip_convcode q, int *K) try {
    return bank_get(q, K, [](auto &o) { return o.K; });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_get_R(yagi_hip_convcode q, int *R) try {
    return bank_get(q, R, [](auto &o) { return o.R; });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_get_rate(yagi_hip_convcode q, size_t *kept, size_t *p) try {
    CHECK_Q(q);
    CHECK_PTR(kept);
    CHECK_PTR(p);
    *kept = q->kp, *p = (size_t)q->p;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_get_ncoded(yagi_hip_convcode q, size_t n, size_t *ncoded) try {
    CHECK_Q(q);
    CHECK_PTR(ncoded);
    YG_TRY(q->check_n(n));
    *ncoded = q->ncoded(n);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_get_nmax(yagi_hip_convcode q, size_t *nmax) try {
    return bank_get(q, nmax, [](auto &o) { return o.nmax(); });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_set_shape(yagi_hip_convcode q, unsigned frames_per_wave, unsigned waves) try {
    CHECK_Q(q);
    if (frames_per_wave == 0 && waves == 0) {
        q->forced = ConvShape{0, 0};
        return YAGI_OK;
    }
    const ConvShape s{frames_per_wave, waves};
    if (!conv_shape_ok(q->K, s))
        return fail(YAGI_ERR_CONFIG, "convcode: the shape (%u frames per wave, %u waves) is not admissible at K = %d",
                    frames_per_wave, waves, q->K);
    q->forced = s;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_get_shape(yagi_hip_convcode q, size_t n, size_t F, yagi_hip_convcode_shape *shape) try {
    CHECK_Q(q);
    CHECK_PTR(shape);
    YG_TRY(q->check_n(n));
    q->fill_shape(q->shape(n, F), n, shape);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_encode_block_dev(yagi_hip_convcode q, const uint8_t *msg_dev, size_t msg_pitch, size_t n, size_t F,
                                       uint8_t *coded_dev, size_t coded_pitch) try {
    CHECK_Q(q);
    YG_TRY(q->check_block(n, F, msg_dev, msg_pitch, (n + 7) / 8, coded_dev, coded_pitch, q->ncoded(n), nullptr));
    return q->encode_dev(msg_dev, msg_pitch, n, F, coded_dev, coded_pitch);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_decode_block_dev(yagi_hip_convcode q, const uint8_t *soft_dev, size_t soft_pitch, size_t n, size_t F,
                                       uint8_t *msg_dev, size_t msg_pitch, uint32_t *metric_dev) try {
    CHECK_Q(q);
    YG_TRY(q->check_block(n, F, soft_dev, soft_pitch, q->ncoded(n), msg_dev, msg_pitch, (n + 7) / 8, metric_dev));
    return q->decode_dev(soft_dev, soft_pitch, n, F, msg_dev, msg_pitch, metric_dev);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_encode_block(yagi_hip_convcode q, const uint8_t *msg, size_t msg_pitch, size_t n, size_t F,
                                   uint8_t *coded, size_t coded_pitch) try {
    CHECK_Q(q);
    const size_t a = (n + 7) / 8, b = q->ncoded(n);
    YG_TRY(q->check_block(n, F, msg, msg_pitch, a, coded, coded_pitch, b, nullptr));
    if (F == 0) return YAGI_OK;
    YG_TRY(q->ws.put(q->st, msg, (F - 1) * msg_pitch + a));
    YG_TRY(q->ws.y.ensure(F * b));
    YG_TRY(q->encode_dev(q->ws.x.as<uint8_t>(), msg_pitch, n, F, q->ws.y.as<uint8_t>(), b));
    return download_rows(q->st, q->ws.y, F, b, coded, coded_pitch);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_decode_block(yagi_hip_convcode q, const uint8_t *soft, size_t soft_pitch, size_t n, size_t F,
                                   uint8_t *msg, size_t msg_pitch, uint32_t *metric) try {
    CHECK_Q(q);
    const size_t a = q->ncoded(n), b = (n + 7) / 8;
    YG_TRY(q->check_block(n, F, soft, soft_pitch, a, msg, msg_pitch, b, metric));
    if (F == 0) return YAGI_OK;
    YG_TRY(q->ws.put(q->st, soft, (F - 1) * soft_pitch + a));
    YG_TRY(q->ws.y.ensure(F * b));
    if (metric) YG_TRY(q->wm.ensure(F * sizeof(uint32_t)));
    YG_TRY(q->decode_dev(q->ws.x.as<uint8_t>(), soft_pitch, n, F, q->ws.y.as<uint8_t>(), b, metric ? q->wm.as<uint32_t>() : nullptr));
    YG_TRY(download_rows(q->st, q->ws.y, F, b, msg, msg_pitch));
    return metric ? download(metric, q->wm.p, F * sizeof(uint32_t), q->st) : YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_encode_host(int K, const unsigned *g, int R, const uint8_t *puncture, int p, int terminated,
                                  const uint8_t *msg, size_t msg_pitch, size_t n, size_t F, uint8_t *coded,
                                  size_t coded_pitch) try {
    ConvHost o;
    YG_TRY(o.configure(K, g, R, puncture, p, terminated));
    YG_TRY(o.check_block(n, F, msg, msg_pitch, (n + 7) / 8, coded, coded_pitch, o.ncoded(n), nullptr));
    conv_encode_host(o, msg, msg_pitch, n, F, coded, coded_pitch);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_decode_host(int K, const unsigned *g, int R, const uint8_t *puncture, int p, int terminated,
                                  const uint8_t *soft, size_t soft_pitch, size_t n, size_t F, uint8_t *msg, size_t msg_pitch,
                                  uint32_t *metric) try {
    ConvHost o;
    YG_TRY(o.configure(K, g, R, puncture, p, terminated));
    YG_TRY(o.check_block(n, F, soft, soft_pitch, o.ncoded(n), msg, msg_pitch, (n + 7) / 8, metric));
    conv_decode_host(o, soft, soft_pitch, n, F, msg, msg_pitch, metric);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_convcode_ncoded_host(int K, int R, const uint8_t *puncture, int p, int terminated, size_t n, size_t *ncoded,
                                  size_t *nmax) try {
    ConvHost o;
    const unsigned ones[4] = {1, 1, 1, 1};                  // the count does not depend on the generators
    YG_TRY(o.configure(K, ones, R, puncture, p, terminated));
    if (nmax) *nmax = o.nmax();
    if (ncoded) {
        YG_TRY(o.check_n(n));
        *ncoded = o.ncoded(n);
    }
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- Packetizer (yagi_hip.h; src/random/scramble.rs for the mask) ------------------------------------------------------
// As ConvCode: no call carries state; the object is its description, one table on the device and the staging of the host
// forms.
namespace yagi {

// everything that needs no device
struct PktHost : Packetizer {
    ConvShape forced{0, 0};                                 // set_shape; fpw = 0: ConvCode's planner

    int configure(size_t n_, int scheme_, int K_, const unsigned *g_, int R_, const uint8_t *puncture, int p_, int terminated_,
                  size_t columns_, int scramble_) {
        ConvHost c;
        YG_TRY(c.configure(K_, g_, R_, puncture, p_, terminated_));
        code = c;
        if (!crc_params(scheme_, &crc)) return fail(YAGI_ERR_CONFIG, "packetizer: the CRC scheme %d is none of YAGI_CRC_*", scheme_);
        if (n_ == 0) return fail(YAGI_ERR_CONFIG, "packetizer: a frame holds at least one payload byte");
        if (columns_ < 1 || columns_ > (size_t)YAGI_PACKETIZER_COLUMNS_MAX)
            return fail(YAGI_ERR_CONFIG, "packetizer: %zu columns are outside 1 .. YAGI_PACKETIZER_COLUMNS_MAX", columns_);
        if (n_ > code.nmax() / 8 || 8 * (n_ + w()) > code.nmax())
            return fail(YAGI_ERR_CONFIG, "packetizer: %zu payload and %zu CRC bytes are more than the code's %zu message bits", n_, w(),
                        code.nmax());
        scheme = scheme_, n = n_, columns = columns_, scramble = scramble_ != 0;
        return YAGI_OK;
    }
    static int check_bps(unsigned bps) {
        if (bps < 1 || bps > 8) return fail(YAGI_ERR_CONFIG, "packetizer: %u bits per symbol are outside 1 .. 8", bps);
        return YAGI_OK;
    }
    // rows of a bytes in, rows of b bytes out; up to three planes of one element per frame
    int check_block(size_t F, const void *in, size_t in_pitch, size_t a, const void *out, size_t out_pitch, size_t b,
                    const uint8_t *valid, bool want_valid, const uint32_t *crcw, const uint32_t *metric) const {
        if (F > (size_t)YAGI_CONVCODE_FRAMES_MAX) return fail(YAGI_ERR_CONFIG, "packetizer: %zu frames are more than YAGI_CONVCODE_FRAMES_MAX", F);
        if (in_pitch < a || out_pitch < b)
            return fail(YAGI_ERR_CONFIG, "packetizer: the pitches are in bytes, at least the row length (%zu in, %zu out)", a, b);
        if (F == 0) return YAGI_OK;
        if (!in || !out || (want_valid && !valid)) return fail(YAGI_ERR_CONFIG, "null pointer argument");
        if (((uintptr_t)crcw | (uintptr_t)metric) & 3) return fail(YAGI_ERR_CONFIG, "packetizer: the crc and metric words are 4-byte aligned");
        const void *ptr[5] = {in, out, valid, crcw, metric};
        const size_t len[5] = {(F - 1) * in_pitch + a, (F - 1) * out_pitch + b, F, F * sizeof(uint32_t), F * sizeof(uint32_t)};
        for (int i = 0; i < 5; ++i)
            for (int j = i + 1; j < 5; ++j)
                if (ptr[i] && ptr[j]) YG_TRY(check_noalias(ptr[i], len[i], ptr[j], len[j]));
        return YAGI_OK;
    }
    size_t steps() const { return code.steps(msg_bits()); }
    ConvShape shape(size_t F) const { return forced.fpw ? forced : conv_plan(code.K, steps(), F); }
    void fill_shape(ConvShape s, yagi_hip_convcode_shape *out) const {
        out->frames_per_wave = s.fpw, out->waves = s.waves, out->states_per_lane = conv_spl(code.K), out->chunk_steps = conv_chunk(s);
        out->frames_per_wg = (size_t)s.fpw * s.waves;
        out->lds_bytes = pkt_lds_bytes(code.K, s, steps(), crc.width != 0);
    }
};

struct PktObj : PktHost {
    using Host = PktHost;
    hipStream_t st = nullptr;
    DevBuf tab, wv, wc, wm;                                 // the table; valid, crc and metric of a host call
    Staging ws;

    int alloc() {
        YG_TRY(require_device());
        std::vector<uint32_t> words(kPktTableWords);
        pkt_table(*this, words.data());
        return fill(tab, words.data(), words.size() * sizeof(uint32_t), st);
    }
    int ensure_host() { return YAGI_OK; }
    int encode_dev(const uint8_t *payload, size_t pitch, size_t F, unsigned bps, uint8_t *tx, size_t tx_pitch) {
        return launch_pkt_encode(*this, tab.as<uint32_t>(), payload, pitch, F, bps, tx, tx_pitch, st);
    }
    int decode_dev(const uint8_t *soft, size_t soft_pitch, size_t F, uint8_t *payload, size_t pitch, uint8_t *valid, uint32_t *crcw,
                   uint32_t *metric) {
        return launch_pkt_decode(*this, shape(F), tab.as<uint32_t>(), soft, soft_pitch, F, payload, pitch, valid, crcw, metric, st);
    }
};

}  // namespace yagi

struct yagi_hip_packetizer_s : PktObj {};

extern "C" {

int yagi_hip_packetizer_plan(int K, int terminated, size_t n, int crc, size_t F, yagi_hip_convcode_shape *plan) try {
    CHECK_PTR(plan);
    const unsigned ones[4] = {1, 1, 1, 1};                  // the arrangement does not depend on the generators
    PktHost o;
    YG_TRY(o.configure(n, crc, K, ones, 2, nullptr, 1, terminated, 1, 0));
    if (F > (size_t)YAGI_CONVCODE_FRAMES_MAX) return fail(YAGI_ERR_CONFIG, "packetizer: %zu frames are more than YAGI_CONVCODE_FRAMES_MAX", F);
    o.fill_shape(o.shape(F), plan);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_create(size_t n, int crc, int K, const unsigned *g, int R, const uint8_t *puncture, int p, int terminated,
                               size_t columns, int scramble, yagi_hip_packetizer *q) try {
    return bank_create(q, n, crc, K, g, R, puncture, p, terminated, columns, scramble);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_destroy(yagi_hip_packetizer q) try {
    return bank_destroy(q);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_clone(yagi_hip_packetizer q, yagi_hip_packetizer *out) try {
    return bank_clone(q, out);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_set_stream(yagi_hip_packetizer q, yagi_stream_t s) try {
    return bank_set_stream(q, s);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_get_payload_len(yagi_hip_packetizer q, size_t *n) try {
    return bank_get(q, n, [](auto &o) { return o.n; });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_get_crc_len(yagi_hip_packetizer q, size_t *w) try {
    return bank_get(q, w, [](auto &o) { return o.w(); });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_get_msg_bits(yagi_hip_packetizer q, size_t *bits) try {
    return bank_get(q, bits, [](auto &o) { return o.msg_bits(); });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_get_enc_len(yagi_hip_packetizer q, size_t *N) try {
    return bank_get(q, N, [](auto &o) { return o.N(); });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_get_nsym(yagi_hip_packetizer q, unsigned bps, size_t *nsym) try {
    CHECK_Q(q);
    CHECK_PTR(nsym);
    YG_TRY(PktHost::check_bps(bps));
    *nsym = q->nsym(bps);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_get_columns(yagi_hip_packetizer q, size_t *columns) try {
    return bank_get(q, columns, [](auto &o) { return o.columns; });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_set_shape(yagi_hip_packetizer q, unsigned frames_per_wave, unsigned waves) try {
    CHECK_Q(q);
    if (frames_per_wave == 0 && waves == 0) {
        q->forced = ConvShape{0, 0};
        return YAGI_OK;
    }
    const ConvShape s{frames_per_wave, waves};
    if (!conv_shape_ok(q->code.K, s))
        return fail(YAGI_ERR_CONFIG, "packetizer: the shape (%u frames per wave, %u waves) is not admissible at K = %d",
                    frames_per_wave, waves, q->code.K);
    q->forced = s;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_get_shape(yagi_hip_packetizer q, size_t F, yagi_hip_convcode_shape *shape) try {
    CHECK_Q(q);
    CHECK_PTR(shape);
    q->fill_shape(q->shape(F), shape);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_encode_block_dev(yagi_hip_packetizer q, const uint8_t *payload_dev, size_t payload_pitch, size_t F,
                                         unsigned bps, uint8_t *tx_dev, size_t tx_pitch) try {
    CHECK_Q(q);
    YG_TRY(PktHost::check_bps(bps));
    YG_TRY(q->check_block(F, payload_dev, payload_pitch, q->n, tx_dev, tx_pitch, q->nsym(bps), nullptr, false, nullptr, nullptr));
    return q->encode_dev(payload_dev, payload_pitch, F, bps, tx_dev, tx_pitch);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_decode_block_dev(yagi_hip_packetizer q, const uint8_t *soft_dev, size_t soft_pitch, size_t F,
                                         uint8_t *payload_dev, size_t payload_pitch, uint8_t *valid_dev, uint32_t *crc_dev,
                                         uint32_t *metric_dev) try {
    CHECK_Q(q);
    YG_TRY(q->check_block(F, soft_dev, soft_pitch, q->N(), payload_dev, payload_pitch, q->n, valid_dev, true, crc_dev, metric_dev));
    return q->decode_dev(soft_dev, soft_pitch, F, payload_dev, payload_pitch, valid_dev, crc_dev, metric_dev);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_encode_block(yagi_hip_packetizer q, const uint8_t *payload, size_t payload_pitch, size_t F, unsigned bps,
                                     uint8_t *tx, size_t tx_pitch) try {
    CHECK_Q(q);
    YG_TRY(PktHost::check_bps(bps));
    const size_t a = q->n, b = q->nsym(bps);
    YG_TRY(q->check_block(F, payload, payload_pitch, a, tx, tx_pitch, b, nullptr, false, nullptr, nullptr));
    if (F == 0) return YAGI_OK;
    YG_TRY(q->ws.put(q->st, payload, (F - 1) * payload_pitch + a));
    YG_TRY(q->ws.y.ensure(F * b));
    YG_TRY(q->encode_dev(q->ws.x.as<uint8_t>(), payload_pitch, F, bps, q->ws.y.as<uint8_t>(), b));
    return download_rows(q->st, q->ws.y, F, b, tx, tx_pitch);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_decode_block(yagi_hip_packetizer q, const uint8_t *soft, size_t soft_pitch, size_t F, uint8_t *payload,
                                     size_t payload_pitch, uint8_t *valid, uint32_t *crc, uint32_t *metric) try {
    CHECK_Q(q);
    const size_t a = q->N(), b = q->n;
    YG_TRY(q->check_block(F, soft, soft_pitch, a, payload, payload_pitch, b, valid, true, crc, metric));
    if (F == 0) return YAGI_OK;
    YG_TRY(q->ws.put(q->st, soft, (F - 1) * soft_pitch + a));
    YG_TRY(q->ws.y.ensure(F * b));
    YG_TRY(q->wv.ensure(F));
    if (crc) YG_TRY(q->wc.ensure(F * sizeof(uint32_t)));
    if (metric) YG_TRY(q->wm.ensure(F * sizeof(uint32_t)));
    YG_TRY(q->decode_dev(q->ws.x.as<uint8_t>(), soft_pitch, F, q->ws.y.as<uint8_t>(), b, q->wv.as<uint8_t>(),
                         crc ? q->wc.as<uint32_t>() : nullptr, metric ? q->wm.as<uint32_t>() : nullptr));
    YG_TRY(download_rows(q->st, q->ws.y, F, b, payload, payload_pitch));
    YG_TRY(download(valid, q->wv.p, F, q->st));
    if (crc) YG_TRY(download(crc, q->wc.p, F * sizeof(uint32_t), q->st));
    return metric ? download(metric, q->wm.p, F * sizeof(uint32_t), q->st) : YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_encode_host(size_t n, int crc, int K, const unsigned *g, int R, const uint8_t *puncture, int p,
                                    int terminated, size_t columns, int scramble, const uint8_t *payload, size_t payload_pitch,
                                    size_t F, unsigned bps, uint8_t *tx, size_t tx_pitch) try {
    PktHost o;
    YG_TRY(o.configure(n, crc, K, g, R, puncture, p, terminated, columns, scramble));
    YG_TRY(PktHost::check_bps(bps));
    YG_TRY(o.check_block(F, payload, payload_pitch, o.n, tx, tx_pitch, o.nsym(bps), nullptr, false, nullptr, nullptr));
    pkt_encode_host(o, payload, payload_pitch, F, bps, tx, tx_pitch);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_decode_host(size_t n, int crc, int K, const unsigned *g, int R, const uint8_t *puncture, int p,
                                    int terminated, size_t columns, int scramble, const uint8_t *soft, size_t soft_pitch, size_t F,
                                    uint8_t *payload, size_t payload_pitch, uint8_t *valid, uint32_t *crc_out, uint32_t *metric) try {
    PktHost o;
    YG_TRY(o.configure(n, crc, K, g, R, puncture, p, terminated, columns, scramble));
    YG_TRY(o.check_block(F, soft, soft_pitch, o.N(), payload, payload_pitch, o.n, valid, true, crc_out, metric));
    pkt_decode_host(o, soft, soft_pitch, F, payload, payload_pitch, valid, crc_out, metric);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_crc_host(int scheme, const uint8_t *data, size_t n, uint32_t *crc) try {
    CHECK_PTR(crc);
    CrcParams c;
    if (!crc_params(scheme, &c)) return fail(YAGI_ERR_CONFIG, "crc: the scheme %d is none of YAGI_CRC_*", scheme);
    if (n && !data) return fail(YAGI_ERR_CONFIG, "null pointer argument");
    *crc = crc_host(c, data, n);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_packetizer_permutation(size_t N, size_t columns, uint32_t *pi) try {
    if (columns < 1 || columns > (size_t)YAGI_PACKETIZER_COLUMNS_MAX)
        return fail(YAGI_ERR_CONFIG, "packetizer: %zu columns are outside 1 .. YAGI_PACKETIZER_COLUMNS_MAX", columns);
    if (N > ((size_t)1 << 31)) return fail(YAGI_ERR_CONFIG, "packetizer: the positions of %zu bits do not fit the words", N);
    if (N == 0) return YAGI_OK;
    CHECK_PTR(pi);
    pkt_permutation(N, columns, pi);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_scramble_data(uint8_t *x, size_t n) try {
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x);
    scramble_data_host(x, n);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_unscramble_data(uint8_t *x, size_t n) try {
    return yagi_hip_scramble_data(x, n);                    // scramble.rs :31-34
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_unscramble_data_soft(uint8_t *x, size_t n) try {
    if (n == 0) return YAGI_OK;
    CHECK_PTR(x);
    unscramble_soft_host(x, n);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- MSequence (src/sequence/msequence.rs) -------------------------------------------------------------------------
// The state is one word and lives on the host alone.  The device holds only the object's two tables of jump matrices
// (sequence_kernels.hip); a block call hands the state to the kernel by value and then advances the host word by the
// same matrices, so nothing is ever read back.
struct yagi_hip_msequence_s {
    hipStream_t st = nullptr;
    unsigned m = 0, g = 0, a = 0, n = 0, state = 0;
    std::vector<unsigned> pow, stride;                    // T^(2^b); the block kernel's lane strides per bps
    yagi::DevBuf dpow, dstride;
    yagi::Staging ws;

    int init(unsigned m_, unsigned g_, unsigned a_) {                        // new() :55-67
        if (m_ > 31 || m_ < 2) return yagi::fail(YAGI_ERR_CONFIG, "m (%u) not in range", m_);
        YG_TRY(yagi::require_device());
        m = m_;
        g = g_;
        a = a_;
        n = (1u << m) - 1u;
        state = a;
        pow.resize(yagi::kMseqPowWords);
        stride.resize(yagi::kMseqStrideWords);
        yagi::msequence_tables(g, n, pow.data(), stride.data());
        return upload_tables();
    }
    int upload_tables() {
        YG_TRY(yagi::fill(dpow, pow.data(), pow.size() * sizeof(unsigned), st));
        return yagi::fill(dstride, stride.data(), stride.size() * sizeof(unsigned), st);
    }
    unsigned advance() {                                                     // :116-122
        const unsigned b = (unsigned)__builtin_popcount(state & g) & 1u;
        state = ((state << 1) | b) & n;
        return b;
    }
    unsigned generate_symbol(unsigned bps) {                                 // :124-131
        unsigned s = 0;
        for (unsigned i = 0; i < bps; ++i) s = (s << 1) | advance();
        return s;
    }
    int block_dev(unsigned bps, size_t nb, uint8_t *y) {
        if (bps < 1 || bps > 8) return yagi::fail(YAGI_ERR_CONFIG, "bits per symbol (%u) must be in 1..8", bps);
        if (nb == 0) return YAGI_OK;
        YG_TRY(yagi::launch_msequence_gen(dpow.as<unsigned>(), dstride.as<unsigned>(), state, g, n, (int)m, (int)bps, nb, y, st));
        state = yagi::msequence_skip(pow.data(), state, (uint64_t)nb * bps);
        return YAGI_OK;
    }
    int block_host(unsigned bps, size_t nb, uint8_t *y) {
        if (bps < 1 || bps > 8) return yagi::fail(YAGI_ERR_CONFIG, "bits per symbol (%u) must be in 1..8", bps);
        if (nb == 0) return YAGI_OK;
        YG_TRY(ws.y.ensure(nb));
        YG_TRY(block_dev(bps, nb, ws.y.as<uint8_t>()));
        return yagi::download(y, ws.y.p, nb, st);
    }
};

#define MSEQ_GET(name, field)                                                                       \
    int yagi_hip_msequence_##name(yagi_hip_msequence q, unsigned *v) try {                          \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(v);                                                                               \
        *v = q->field;                                                                              \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }

extern "C" {

int yagi_hip_msequence_create(unsigned m, unsigned g, unsigned a, yagi_hip_msequence *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    auto o = std::make_unique<yagi_hip_msequence_s>();
    YG_TRY(o->init(m, g, a));
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_msequence_create_genpoly(unsigned g, yagi_hip_msequence *q) try {       // :69-77
    CHECK_PTR(q);
    *q = nullptr;
    unsigned t = 0;
    while (t < 32 && (g >> t) != 0u) ++t;                 // msb_index: the bit length
    if (t < 2) return fail(YAGI_ERR_CONFIG, "invalid generator polynomial: 0x%x", g);
    return yagi_hip_msequence_create(t, g, 1u, q);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_msequence_destroy(yagi_hip_msequence q) try {
    if (q) (void)hipStreamSynchronize(q->st);
    delete q;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_msequence_clone(yagi_hip_msequence q, yagi_hip_msequence *out) try {
    CHECK_Q(q);
    CHECK_PTR(out);
    *out = nullptr;
    auto o = std::make_unique<yagi_hip_msequence_s>();
    o->st = q->st;
    o->m = q->m;
    o->g = q->g;
    o->a = q->a;
    o->n = q->n;
    o->state = q->state;
    o->pow = q->pow;
    o->stride = q->stride;
    YG_TRY(o->upload_tables());
    *out = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_msequence_set_stream(yagi_hip_msequence q, yagi_stream_t s) try {
    CHECK_Q(q);
    if (q->st == to_stream(s)) return YAGI_OK;
    YG_HIP(hipStreamSynchronize(q->st));
    q->st = to_stream(s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_msequence_reset(yagi_hip_msequence q) try {                              // :133-135
    CHECK_Q(q);
    q->state = q->a;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_msequence_advance(yagi_hip_msequence q, unsigned *bit) try {
    CHECK_Q(q);
    CHECK_PTR(bit);
    *bit = q->advance();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_msequence_generate_symbol(yagi_hip_msequence q, unsigned bps, unsigned *sym) try {
    CHECK_Q(q);
    CHECK_PTR(sym);
    if (bps > 32) return fail(YAGI_ERR_CONFIG, "bits per symbol (%u) must be at most 32", bps);
    *sym = q->generate_symbol(bps);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_msequence_set_state(yagi_hip_msequence q, unsigned a) try {              // :143-145, not masked
    CHECK_Q(q);
    q->state = a;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
MSEQ_GET(get_state, state)
MSEQ_GET(get_genpoly, g)
MSEQ_GET(get_genpoly_length, m)
MSEQ_GET(get_length, n)
int yagi_hip_msequence_measure_period(yagi_hip_msequence q, unsigned *period) try {   // :147-158
    CHECK_Q(q);
    CHECK_PTR(period);
    const unsigned s = q->state;
    unsigned p = 0;
    for (unsigned i = 0; i <= q->n; ++i) {
        q->advance();
        ++p;
        if (q->state == s) break;
    }
    *period = p;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_msequence_skip(yagi_hip_msequence q, uint64_t k) try {
    CHECK_Q(q);
    q->state = yagi::msequence_skip(q->pow.data(), q->state, k);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_msequence_generate_bits_block(yagi_hip_msequence q, size_t n, uint8_t *bits) try {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(bits);
    return q->block_host(1, n, bits);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_msequence_generate_bits_block_dev(yagi_hip_msequence q, size_t n, uint8_t *bits_dev) try {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(bits_dev);
    return q->block_dev(1, n, bits_dev);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_msequence_generate_symbols_block(yagi_hip_msequence q, unsigned bps, size_t n, uint8_t *sym) try {
    CHECK_Q(q);
    if (n != 0) CHECK_PTR(sym);
    return q->block_host(bps, n, sym);
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_msequence_generate_symbols_block_dev(yagi_hip_msequence q, unsigned bps, size_t n, uint8_t *sym_dev) try {
    CHECK_Q(q);
    if (n != 0) CHECK_PTR(sym_dev);
    return q->block_dev(bps, n, sym_dev);
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- BSequence (src/sequence/bsequence.rs) -------------------------------------------------------------------------
// The state is the reference's word array, word 0 oldest and masked.  Scalar calls run on the host mirror; the block
// call runs sequence_kernels.hip on the device copy, whose launch writes the window it leaves into the other of two
// buffers.  The two copies are synchronised lazily (Mirror).  The kernel reads ref's words from a buffer of q's own,
// refreshed when ref (identified by uid) or its content (counted by ver) differs from what that buffer holds.
struct yagi_hip_bsequence_s {
    hipStream_t st = nullptr;
    size_t num_bits = 0, num_bits_msb = 0;
    unsigned bit_mask_msb = 0;
    std::vector<unsigned> s;                              // host mirror
    yagi::PingPong<> dev;                                 // device copy
    yagi::DevBuf dref;                                    // ref's words as the block kernel reads them
    unsigned long long uid = 0, ver = 0, ref_uid = 0, ref_ver = 0;
    yagi::Staging ws;
    yagi::Mirror mirror;

    static unsigned long long next_uid() {
        static std::atomic<unsigned long long> c{0};
        return ++c;
    }
    size_t bytes() const { return s.size() * sizeof(unsigned); }
    static int check_bits(size_t nbits) {
        if (nbits == 0) return yagi::fail(YAGI_ERR_CONFIG, "sequence length must be greater than zero");
        if (nbits > (size_t)YAGI_BSEQUENCE_NMAX)
            return yagi::fail(YAGI_ERR_CONFIG, "sequence length %zu exceeds YAGI_BSEQUENCE_NMAX = %d", nbits, YAGI_BSEQUENCE_NMAX);
        return YAGI_OK;
    }
    int init(size_t nbits) {                                                 // new() :16-30
        YG_TRY(check_bits(nbits));
        YG_TRY(yagi::require_device());
        num_bits = nbits;
        num_bits_msb = nbits % 32 == 0 ? 32 : nbits % 32;
        bit_mask_msb = num_bits_msb == 32 ? 0xffffffffu : (1u << num_bits_msb) - 1u;
        s.assign((nbits + 31) / 32, 0u);
        uid = next_uid();
        YG_TRY(dev.alloc(bytes()));
        YG_TRY(dref.alloc(bytes()));
        return reset();
    }
    int reset() {                                                            // :90-92
        std::fill(s.begin(), s.end(), 0u);
        YG_HIP(hipMemsetAsync(dev.cur(), 0, bytes(), st));
        mirror.in_sync();
        ++ver;
        return YAGI_OK;
    }
    int ensure_host() {
        return mirror.need_host([&] { return yagi::download(s.data(), dev.cur(), bytes(), st); });
    }
    int ensure_dev() {
        return mirror.need_dev([&] { return yagi::upload(dev.cur(), s.data(), bytes(), st); });
    }
    int enter_host() {
        YG_TRY(ensure_host());
        mirror.host_written();
        ++ver;
        return YAGI_OK;
    }
    void push(unsigned bit) {                                                // :115-127 (after enter_host)
        s[0] = (s[0] << 1) & bit_mask_msb;
        for (size_t i = 1; i < s.size(); ++i) {
            s[i - 1] |= s[i] >> 31;
            s[i] <<= 1;
        }
        s.back() |= bit & 1u;
    }
    void load_bytes(const uint8_t *v) {                                      // init() :95-108
        for (size_t i = 0; i < num_bits; ++i) push((v[i / 8] >> (7 - i % 8)) & 1u);
    }
    int block_dev(yagi_hip_bsequence_s *ref, const uint8_t *sym, size_t nb, unsigned bps, int32_t *rxy) {
        if (nb == 0) return YAGI_OK;
        if (ref->uid != ref_uid || ref->ver != ref_ver) {                    // ref as it stands now
            YG_TRY(ref->ensure_host());
            YG_TRY(yagi::upload(dref.p, ref->s.data(), bytes(), st));
            ref_uid = ref->uid;
            ref_ver = ref->ver;
        }
        YG_TRY(ensure_dev());
        YG_TRY(yagi::launch_bsequence_corr(dev.cur<unsigned>(), dev.next<unsigned>(), dref.as<unsigned>(), (int)s.size(),
                                           bit_mask_msb, (int)ref->num_bits_msb, sym, nb, (int)bps, rxy, st));
        dev.flip();
        mirror.dev_written();
        ++ver;
        return YAGI_OK;
    }
};

static int bseq_block_args(yagi_hip_bsequence q, yagi_hip_bsequence ref, unsigned bps) {
    CHECK_Q(q);
    CHECK_Q(ref);
    if (bps < 1 || bps > 8) return fail(YAGI_ERR_CONFIG, "bits per symbol (%u) must be in 1..8", bps);
    if (ref == q) return fail(YAGI_ERR_CONFIG, "the reference sequence must be another object than the one pushed into");
    if (ref->s.size() != q->s.size()) return fail(YAGI_ERR_CONFIG, "binary sequences must be the same length");
    return YAGI_OK;
}
// out = a (op) b word by word (:153-176)
template <class F>
static int bseq_combine(yagi_hip_bsequence a, yagi_hip_bsequence b, yagi_hip_bsequence out, F &&op) {
    CHECK_Q(a);
    CHECK_Q(b);
    CHECK_Q(out);
    if (a->s.size() != b->s.size() || a->s.size() != out->s.size())
        return fail(YAGI_ERR_CONFIG, "binary sequences must be same length");
    YG_TRY(a->ensure_host());
    YG_TRY(b->ensure_host());
    YG_TRY(out->enter_host());
    for (size_t i = 0; i < a->s.size(); ++i) out->s[i] = op(a->s[i], b->s[i]);
    return YAGI_OK;
}

extern "C" {

int yagi_hip_bsequence_create(size_t num_bits, yagi_hip_bsequence *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    auto o = std::make_unique<yagi_hip_bsequence_s>();
    YG_TRY(o->init(num_bits));
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_create_from_msequence(yagi_hip_msequence ms, yagi_hip_bsequence *q) try {    // :81-88
    CHECK_PTR(q);
    *q = nullptr;
    CHECK_Q(ms);
    auto o = std::make_unique<yagi_hip_bsequence_s>();
    YG_TRY(o->init((size_t)ms->n));
    YG_TRY(o->enter_host());
    for (unsigned i = 0; i < ms->n; ++i) o->push(ms->advance());
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_create_ccodes(yagi_hip_bsequence qa, yagi_hip_bsequence qb) try {            // :34-79
    CHECK_Q(qa);
    CHECK_Q(qb);
    if (qa->num_bits != qb->num_bits) return fail(YAGI_ERR_CONFIG, "sequence lengths must match");
    if (qa->num_bits < 8) return fail(YAGI_ERR_CONFIG, "sequence too short");
    if (qa->num_bits % 8 != 0) return fail(YAGI_ERR_CONFIG, "sequence must be multiple of 8");
    const size_t nby = qa->num_bits / 8;
    std::vector<uint8_t> a(nby, 0), b(nby, 0);
    a[nby - 1] = 0xb8;
    b[nby - 1] = 0xb7;
    for (size_t n = 1; n < nby; n *= 2) {
        const size_t i1 = nby - n, i0 = nby - 2 * n;
        for (size_t i = 0; i < n; ++i) {                  // a -> [a b], b -> [a ~b]
            a[i0 + i] = a[i1 + i];
            b[i0 + i] = a[i1 + i];
        }
        for (size_t i = 0; i < n; ++i) a[i1 + i] = b[i1 + i];
        for (size_t i = 0; i < n; ++i) b[nby - i - 1] ^= 0xff;
    }
    YG_TRY(qa->enter_host());
    YG_TRY(qb->enter_host());
    qa->load_bytes(a.data());
    qb->load_bytes(b.data());
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_destroy(yagi_hip_bsequence q) try {
    if (q) (void)hipStreamSynchronize(q->st);
    delete q;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_clone(yagi_hip_bsequence q, yagi_hip_bsequence *out) try {
    CHECK_Q(q);
    CHECK_PTR(out);
    *out = nullptr;
    YG_TRY(q->ensure_host());
    auto o = std::make_unique<yagi_hip_bsequence_s>();
    o->st = q->st;
    YG_TRY(o->init(q->num_bits));
    o->s = q->s;
    o->mirror.host_written();
    *out = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_set_stream(yagi_hip_bsequence q, yagi_stream_t s) try {
    CHECK_Q(q);
    if (q->st == to_stream(s)) return YAGI_OK;
    YG_HIP(hipStreamSynchronize(q->st));
    q->st = to_stream(s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_reset(yagi_hip_bsequence q) try {
    CHECK_Q(q);
    return q->reset();
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_init(yagi_hip_bsequence q, const uint8_t *v, size_t nbytes) try {
    CHECK_Q(q);
    CHECK_PTR(v);
    if (nbytes < (q->num_bits + 7) / 8) return fail(YAGI_ERR_CONFIG, "init needs %zu bytes", (q->num_bits + 7) / 8);
    YG_TRY(q->enter_host());
    q->load_bytes(v);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_push(yagi_hip_bsequence q, unsigned bit) try {
    CHECK_Q(q);
    YG_TRY(q->enter_host());
    q->push(bit);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_circshift(yagi_hip_bsequence q) try {                                        // :130-134
    CHECK_Q(q);
    YG_TRY(q->enter_host());
    q->push((q->s[0] >> (q->num_bits_msb - 1)) & 1u);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_correlate(yagi_hip_bsequence a, yagi_hip_bsequence b, int32_t *rxy) try {    // :137-150
    CHECK_Q(a);
    CHECK_Q(b);
    CHECK_PTR(rxy);
    if (a->s.size() != b->s.size()) return fail(YAGI_ERR_CONFIG, "binary sequences must be the same length");
    YG_TRY(a->ensure_host());
    YG_TRY(b->ensure_host());
    int32_t r = 0;
    for (size_t i = 0; i < a->s.size(); ++i) r += __builtin_popcount(~(a->s[i] ^ b->s[i]));
    *rxy = r - (32 - (int32_t)a->num_bits_msb);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_add(yagi_hip_bsequence a, yagi_hip_bsequence b, yagi_hip_bsequence out) try {
    return bseq_combine(a, b, out, [](unsigned x, unsigned y) { return x ^ y; });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_mul(yagi_hip_bsequence a, yagi_hip_bsequence b, yagi_hip_bsequence out) try {
    return bseq_combine(a, b, out, [](unsigned x, unsigned y) { return x & y; });
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_accumulate(yagi_hip_bsequence q, unsigned *count) try {                      // :179-181
    CHECK_Q(q);
    CHECK_PTR(count);
    YG_TRY(q->ensure_host());
    unsigned c = 0;
    for (unsigned w : q->s) c += (unsigned)__builtin_popcount(w);
    *count = c;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_index(yagi_hip_bsequence q, size_t i, unsigned *bit) try {                   // :188-194
    CHECK_Q(q);
    CHECK_PTR(bit);
    if (i >= q->num_bits) return fail(YAGI_ERR_CONFIG, "invalid index %zu", i);
    YG_TRY(q->ensure_host());
    *bit = (q->s[q->s.size() - 1 - i / 32] >> (i % 32)) & 1u;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_get_length(yagi_hip_bsequence q, size_t *num_bits) try {
    CHECK_Q(q);
    CHECK_PTR(num_bits);
    *num_bits = q->num_bits;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_push_correlate_block(yagi_hip_bsequence q, yagi_hip_bsequence ref, const uint8_t *sym, size_t n,
                                            unsigned bps, int32_t *rxy) try {
    YG_TRY(bseq_block_args(q, ref, bps));
    if (n == 0) return YAGI_OK;
    CHECK_PTR(sym);
    YG_TRY(q->ws.put(q->st, sym, n));
    if (rxy) YG_TRY(q->ws.y.ensure(n * sizeof(int32_t)));
    YG_TRY(q->block_dev(ref, q->ws.x.as<uint8_t>(), n, bps, rxy ? q->ws.y.as<int32_t>() : nullptr));
    if (rxy) return download(rxy, q->ws.y.p, n * sizeof(int32_t), q->st);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
int yagi_hip_bsequence_push_correlate_block_dev(yagi_hip_bsequence q, yagi_hip_bsequence ref, const uint8_t *sym_dev,
                                                size_t n, unsigned bps, int32_t *rxy_dev) try {
    YG_TRY(bseq_block_args(q, ref, bps));
    if (n == 0) return YAGI_OK;
    CHECK_PTR(sym_dev);
    if (rxy_dev) CHECK_NOALIAS(sym_dev, n, rxy_dev, n);
    return q->block_dev(ref, sym_dev, n, bps, rxy_dev);
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- Ddc / Duc (the reference's src/filter/dds.rs is an empty file: defined here as compositions) -----------------------
// Ddc = Osc::mix_block_down, then FirDecimationFilter::execute_block; Duc = FirInterpolationFilter::execute_block, then
// Osc::mix_block_up.  The objects compose the parts' own structs, so the window mirror, the staging of host slices, the
// oscillator words and their constrain routine are the shared ones.  A block call runs one fused launch
// (ddc_kernels.hip) where a fused kernel serves the shape, else the two launches of the parts through a scratch buffer
// the object owns (kernel choice 1 forces that route); the words are the same either way.
namespace yagi {

static int ddc_check_scheme(int scheme) {
    if (scheme != YAGI_OSC_NCO && scheme != YAGI_OSC_VCO) return fail(YAGI_ERR_CONFIG, "osc: unknown scheme %d", scheme);
    return YAGI_OK;
}

struct DdcCommon {
    OscObj osc;
    DevBuf scratch;            // two-launch route: the full-rate stream between the launches
    int choice = 0, last = 0;  // set_kernel / get_last_kernel
    int set_kernel(int c) {
        if (c < 0 || c > 2) return fail(YAGI_ERR_CONFIG, "unknown kernel choice %d (0 auto, 1 two launches, 2 fused)", c);
        choice = c;
        return YAGI_OK;
    }
    void copy_osc(const DdcCommon &o) {
        osc.theta = o.osc.theta;
        osc.d_theta = o.osc.d_theta;
        osc.alpha = o.osc.alpha;
        osc.beta = o.osc.beta;
        choice = o.choice;
    }
};

template <class K>
struct DdcObj : DdcCommon {
    using C = typename K::C;
    FirDecim<K> fir;

    hipStream_t &stream() { return fir.st; }
    DevWindow<cf32> &window() { return fir.w; }
    C &scale() { return fir.scale; }
    size_t rate() const { return (size_t)fir.M; }
    size_t n_in(size_t n) const { return n * (size_t)fir.M; }
    size_t n_out(size_t n) const { return n; }
    int init(int scheme, size_t M, const C *h, size_t n) {
        YG_TRY(ddc_check_scheme(scheme));
        YG_TRY(fir.init(M, h, n));
        osc.st = fir.st;
        return osc.init(scheme);
    }
    int clone_from(DdcObj &q) {
        YG_TRY(q.fir.w.ensure_dev(q.fir.st));
        fir.st = q.fir.st;
        YG_TRY(init(q.osc.vco ? YAGI_OSC_VCO : YAGI_OSC_NCO, (size_t)q.fir.M, q.fir.h.data(), q.fir.h.size()));
        fir.scale = q.fir.scale;
        copy_osc(q);
        return fir.w.clone_from(q.fir.w, q.fir.st);
    }
    // n outputs from n*M device samples
    int block_dev(const cf32 *x, size_t n, cf32 *y) {
        if (n == 0) return YAGI_OK;
        const size_t nin = n_in(n);
        if (choice != 1 && ddc_fused_serves<K>(fir.L, fir.M, n, osc.vco)) {
            YG_TRY(fir.w.ensure_dev(fir.st));
            YG_TRY((launch_ddc_block<K>(fir.w.dev(), x, fir.taps.template as<C>(), fir.L, fir.M, fir.scale, y, n, fir.st,
                                        fir.w.next(), osc.vco, osc.tab.p, osc.theta, osc.d_theta)));
            fir.w.flip();                           // the kernel's last workgroup wrote the next window, mixed
            osc.theta += (uint32_t)nin * osc.d_theta;
            last = 2;
            return YAGI_OK;
        }
        YG_TRY(scratch.ensure(nin * sizeof(cf32)));
        YG_TRY(osc.block_dev(x, nin, scratch.as<cf32>(), true));
        YG_TRY(fir.block_dev(scratch.as<cf32>(), n, y));
        last = 1;
        return YAGI_OK;
    }
    // x[M] -> y on the host mirror: mix, step, push; the output follows the FIRST of the M pushes (firdecim.rs:179-191)
    int execute(const cf32 *x, cf32 *y) {
        YG_TRY(fir.w.ensure_host(fir.st));
        for (int i = 0; i < fir.M; ++i) {
            fir.w.push(osc_mix(osc.vco, osc.theta, true, x[i]));
            osc.theta += osc.d_theta;
            if (i == 0) *y = host_fir_window_dot<cf32, C>(fir.w.host(), (size_t)fir.L, fir.h.data(), fir.scale);
        }
        return YAGI_OK;
    }
    Staging &staging() { return fir.ws; }
};

template <class K>
struct DucObj : DdcCommon {
    using C = typename K::C;
    FirInterp<K> fir;

    hipStream_t &stream() { return fir.bank.st; }
    DevWindow<cf32> &window() { return fir.bank.w; }
    C &scale() { return fir.bank.scale; }
    size_t rate() const { return (size_t)fir.interp; }
    size_t n_in(size_t n) const { return n; }
    size_t n_out(size_t n) const { return n * (size_t)fir.interp; }
    int init(int scheme, size_t I, const C *h, size_t n) {
        YG_TRY(ddc_check_scheme(scheme));
        YG_TRY(fir.init(I, h, n));
        osc.st = fir.bank.st;
        return osc.init(scheme);
    }
    int clone_from(DucObj &q) {
        FirPfb<K> &b = fir.bank, &qb = q.fir.bank;
        YG_TRY(qb.w.ensure_dev(qb.st));
        fir.interp = q.fir.interp;
        fir.hs = q.fir.hs;
        b.st = qb.st;
        b.nf = qb.nf;
        b.Ls = qb.Ls;
        b.hb = qb.hb;
        b.scale = qb.scale;
        YG_TRY(fill(b.taps, b.hb.data(), b.hb.size() * sizeof(C), b.st));
        YG_TRY(b.w.clone_from(qb.w, qb.st));
        osc.st = b.st;
        YG_TRY(osc.init(q.osc.vco ? YAGI_OSC_VCO : YAGI_OSC_NCO));
        copy_osc(q);
        return YAGI_OK;
    }
    // n inputs -> n*I device outputs
    int block_dev(const cf32 *x, size_t n, cf32 *y) {
        if (n == 0) return YAGI_OK;
        FirPfb<K> &b = fir.bank;
        const size_t nout = n_out(n);
        if (choice != 1 && duc_fused_serves<K>(b.nf, b.Ls, osc.vco)) {
            YG_TRY(b.w.ensure_dev(b.st));
            YG_TRY((launch_duc_all<K>(b.w.dev(), x, b.taps.template as<C>(), b.nf, b.Ls, b.scale, y, n, b.st, b.w.next(),
                                      osc.vco, osc.tab.p, osc.theta, osc.d_theta)));
            b.w.flip();                             // the kernel's last workgroup wrote the next window
            osc.theta += (uint32_t)nout * osc.d_theta;
            last = 2;
            return YAGI_OK;
        }
        YG_TRY(scratch.ensure(nout * sizeof(cf32)));
        YG_TRY(fir.block_dev(x, n, scratch.as<cf32>()));
        YG_TRY(osc.block_dev(scratch.as<cf32>(), nout, y, false));
        last = 1;
        return YAGI_OK;
    }
    // x -> y[I] on the host mirror: push, then every branch's sum (firinterp.rs:224-231) mixed up and stepped
    int execute(const cf32 *x, cf32 *y) {
        FirPfb<K> &b = fir.bank;
        YG_TRY(b.w.ensure_host(b.st));
        b.w.push(*x);
        for (int i = 0; i < b.nf; ++i) {
            const cf32 v = host_fir_window_dot<cf32, C>(b.w.host(), (size_t)b.Ls, b.hb.data() + (size_t)i * b.Ls, b.scale);
            y[i] = osc_mix(osc.vco, osc.theta, false, v);
            osc.theta += osc.d_theta;
        }
        return YAGI_OK;
    }
    Staging &staging() { return fir.bank.ws; }
};

template <class Q>
static int ddc_block_host(Q *q, const cf32 *x, size_t n, cf32 *y) {
    return q->staging().run(q->stream(), x, q->n_in(n), y, q->n_out(n),
                            [&](const cf32 *xd, cf32 *yd) { return q->block_dev(xd, n, yd); });
}

// the Kaiser prototypes of the parts (firdecim.rs:70-87, firinterp.rs:73-90): same checks, same messages
template <class C>
static int ddc_kaiser_taps(bool interp, size_t M, size_t m, float as_, std::vector<C> &hc) {
    if (M < 2) return fail(YAGI_ERR_CONFIG, interp ? "interp factor must be greater than 1" : "decim factor must be greater than 1");
    if (m == 0) return fail(YAGI_ERR_CONFIG, "filter delay must be greater than 0");
    if (as_ < 0.0f) return fail(YAGI_ERR_CONFIG, "stop-band attenuation must be positive");
    std::vector<float> hf;
    YG_TRY(design_kaiser(2 * M * m + 1, 0.5f / (float)M, as_, 0.0f, hf));
    hc.resize(hf.size() - (interp ? 1 : 0));               // the interpolator drops the last tap (firinterp.rs:89)
    for (size_t i = 0; i < hc.size(); ++i) hc[i] = to_c(hf[i], (C *)nullptr);
    return YAGI_OK;
}

}  // namespace yagi

// OBJ: ddc | duc; INTERP: 0 | 1; RATE: the name of the rate accessor
#define YAGI_DDC_IMPL(OBJ, TMPL, INTERP, RATE, K, KT, C)                                                            \
    struct yagi_hip_##OBJ##_##K##_s : TMPL<KT> {};                                                                  \
    extern "C" {                                                                                                    \
    int yagi_hip_##OBJ##_##K##_create(int scheme, size_t rate, const C *h, size_t h_len, yagi_hip_##OBJ##_##K *q) try { \
        CHECK_PTR(q);                                                                                               \
        *q = nullptr;                                                                                               \
        if (h_len && !h) return fail(YAGI_ERR_CONFIG, "null pointer argument");                                     \
        auto o = std::make_unique<yagi_hip_##OBJ##_##K##_s>();                                                      \
        YG_TRY(o->init(scheme, rate, h, h_len));                                                                    \
        *q = o.release();                                                                                           \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_create_kaiser(int scheme, size_t rate, size_t m, float as_,                          \
                                             yagi_hip_##OBJ##_##K *q) try {                                         \
        CHECK_PTR(q);                                                                                               \
        *q = nullptr;                                                                                               \
        YG_TRY(ddc_check_scheme(scheme));                                                                           \
        std::vector<C> hc;                                                                                          \
        YG_TRY(ddc_kaiser_taps<C>(INTERP, rate, m, as_, hc));                                                       \
        return yagi_hip_##OBJ##_##K##_create(scheme, rate, hc.data(), hc.size(), q);                                \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_destroy(yagi_hip_##OBJ##_##K q) try {                                                \
        if (q) (void)hipStreamSynchronize(q->stream());                                                             \
        delete q;                                                                                                   \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_clone(yagi_hip_##OBJ##_##K q, yagi_hip_##OBJ##_##K *out) try {                       \
        CHECK_Q(q);                                                                                                 \
        CHECK_PTR(out);                                                                                             \
        *out = nullptr;                                                                                             \
        auto o = std::make_unique<yagi_hip_##OBJ##_##K##_s>();                                                      \
        YG_TRY(o->clone_from(*q));                                                                                  \
        *out = o.release();                                                                                         \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_set_stream(yagi_hip_##OBJ##_##K q, yagi_stream_t s) try {                            \
        CHECK_Q(q);                                                                                                 \
        if (q->stream() == to_stream(s)) return YAGI_OK;                                                            \
        YG_HIP(hipStreamSynchronize(q->stream()));                                                                  \
        q->stream() = to_stream(s);                                                                                 \
        q->osc.st = to_stream(s);                                                                                   \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_reset(yagi_hip_##OBJ##_##K q) try {      /* the filter window; the oscillator stays */ \
        CHECK_Q(q);                                                                                                 \
        return q->window().reset(q->stream());                                                                      \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_set_frequency(yagi_hip_##OBJ##_##K q, float dtheta) try {                            \
        CHECK_Q(q);                                                                                                 \
        return osc_constrain(dtheta, &q->osc.d_theta);                                                              \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_adjust_frequency(yagi_hip_##OBJ##_##K q, float df) try {                             \
        CHECK_Q(q);                                                                                                 \
        uint32_t w = 0;                                                                                             \
        YG_TRY(osc_constrain(df, &w));                                                                              \
        q->osc.d_theta += w;                                                                                        \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_set_phase(yagi_hip_##OBJ##_##K q, float phi) try {                                   \
        CHECK_Q(q);                                                                                                 \
        return osc_constrain(phi, &q->osc.theta);                                                                   \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_adjust_phase(yagi_hip_##OBJ##_##K q, float dphi) try {                               \
        CHECK_Q(q);                                                                                                 \
        uint32_t w = 0;                                                                                             \
        YG_TRY(osc_constrain(dphi, &w));                                                                            \
        q->osc.theta += w;                                                                                          \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_get_frequency(yagi_hip_##OBJ##_##K q, float *f) try {                                \
        CHECK_Q(q);                                                                                                 \
        CHECK_PTR(f);                                                                                               \
        *f = osc_frequency(q->osc.d_theta);                                                                         \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_get_phase(yagi_hip_##OBJ##_##K q, float *phi) try {                                  \
        CHECK_Q(q);                                                                                                 \
        CHECK_PTR(phi);                                                                                             \
        *phi = osc_phase(q->osc.theta);                                                                             \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_get_state(yagi_hip_##OBJ##_##K q, uint32_t *theta, uint32_t *d_theta) try {          \
        CHECK_Q(q);                                                                                                 \
        CHECK_PTR(theta);                                                                                           \
        CHECK_PTR(d_theta);                                                                                         \
        *theta = q->osc.theta;                                                                                      \
        *d_theta = q->osc.d_theta;                                                                                  \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_set_state(yagi_hip_##OBJ##_##K q, uint32_t theta, uint32_t d_theta) try {            \
        CHECK_Q(q);                                                                                                 \
        q->osc.theta = theta;                                                                                       \
        q->osc.d_theta = d_theta;                                                                                   \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_set_scale(yagi_hip_##OBJ##_##K q, C scale) try {                                     \
        CHECK_Q(q);                                                                                                 \
        q->scale() = scale;                                                                                         \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_get_scale(yagi_hip_##OBJ##_##K q, C *scale) try {                                    \
        CHECK_Q(q);                                                                                                 \
        CHECK_PTR(scale);                                                                                           \
        *scale = q->scale();                                                                                        \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_##RATE(yagi_hip_##OBJ##_##K q, size_t *rate) try {                                   \
        CHECK_Q(q);                                                                                                 \
        CHECK_PTR(rate);                                                                                            \
        *rate = q->rate();                                                                                          \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_set_kernel(yagi_hip_##OBJ##_##K q, int choice) try {                                 \
        CHECK_Q(q);                                                                                                 \
        return q->set_kernel(choice);                                                                               \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_get_last_kernel(yagi_hip_##OBJ##_##K q, int *k) try {                                \
        CHECK_Q(q);                                                                                                 \
        CHECK_PTR(k);                                                                                               \
        *k = q->last;                                                                                               \
        return YAGI_OK;                                                                                             \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_execute(yagi_hip_##OBJ##_##K q, const yagi_cf32 *x, yagi_cf32 *y) try {              \
        CHECK_Q(q);                                                                                                 \
        CHECK_PTR(x);                                                                                               \
        CHECK_PTR(y);                                                                                               \
        return q->execute(x, y);                                                                                    \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_execute_block(yagi_hip_##OBJ##_##K q, const yagi_cf32 *x, size_t n,                  \
                                             yagi_cf32 *y) try {                                                    \
        CHECK_Q(q);                                                                                                 \
        if (n == 0) return YAGI_OK;                                                                                 \
        CHECK_PTR(x);                                                                                               \
        CHECK_PTR(y);                                                                                               \
        return ddc_block_host(q, x, n, y);                                                                          \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    int yagi_hip_##OBJ##_##K##_execute_block_dev(yagi_hip_##OBJ##_##K q, const yagi_cf32 *x, size_t n,              \
                                                 yagi_cf32 *y) try {                                                \
        CHECK_Q(q);                                                                                                 \
        if (n == 0) return YAGI_OK;                                                                                 \
        CHECK_PTR(x);                                                                                               \
        CHECK_PTR(y);                                                                                               \
        CHECK_NOALIAS(x, q->n_in(n), y, q->n_out(n));                                                               \
        return q->block_dev(x, n, y);                                                                               \
    } catch (...) { return ::yagi::api_exception(); }                                                               \
    }

YAGI_DDC_IMPL(ddc, DdcObj, false, get_decim_rate, crcf, CRCF, float)
YAGI_DDC_IMPL(ddc, DdcObj, false, get_decim_rate, cccf, CCCF, yagi_cf32)
YAGI_DDC_IMPL(duc, DucObj, true, get_interp_rate, crcf, CRCF, float)
YAGI_DDC_IMPL(duc, DucObj, true, get_interp_rate, cccf, CCCF, yagi_cf32)

// ---- SymStream (src/framing/symstream.rs) -----------------------------------------------------------------------------
// The reference's fields (ftype, k, m, beta, modem, gain, interp, buf, buf_index :6-17) plus the symbol source: the words
// and jump tables of an MSequence, copied at creation.  The modem and the interpolator are the library's own objects, so
// the three-launch route (DPSK, shapes the fused kernel does not serve) is their launchers one after the other and the
// window mirror is the shared one; a block call runs symstream_kernels.hip wherever that serves the object as it stands.
struct yagi_hip_symstreamcf_s {
    int ftype = YAGI_FIR_SHAPE_UNKNOWN;
    size_t k = 0, m = 0;
    float beta = 0.0f, gain = 1.0f;
    yagi_hip_modem modem = nullptr;            // owned
    FirInterp<CRCF> fir;
    int p = 0;                                 // buf_index
    unsigned sm = 0, sg = 0, smask = 0, sstate = 0;       // the source: MSequence's m, g, n and state
    std::vector<unsigned> pow, stride;         // T^(2^b); the fused kernel's lane strides per bps
    DevBuf dpow, dstride;
    int run = 0;                               // symstream_run(k, Ls): what `stride` is built for
    DevBuf dbuf;                               // k values: the reference's buf, the branches of the last pushed symbol
    DevBuf dsym, dpts, dout, flag;             // three-launch route: symbols, points, interpolator output; range flag
    Staging ws;

    ~yagi_hip_symstreamcf_s() {
        if (modem) (void)yagi_hip_modem_destroy(modem);
    }
    hipStream_t &stream() { return fir.bank.st; }
    int Ls() const { return fir.bank.Ls; }
    int alloc_dev() {
        YG_TRY(fill(dpow, pow.data(), pow.size() * sizeof(unsigned), stream()));
        YG_TRY(fill(dstride, stride.data(), stride.size() * sizeof(unsigned), stream()));
        YG_TRY(dbuf.alloc(k * sizeof(cf32)));
        YG_HIP(hipMemsetAsync(dbuf.p, 0, k * sizeof(cf32), stream()));
        return flag.alloc(sizeof(int));
    }
    int init(int ftype_, size_t k_, size_t m_, float beta_, const float *h, size_t h_len, int scheme, yagi_hip_msequence src) {
        YG_TRY(fir.init(k_, h, h_len));        // needs the device
        YG_TRY(yagi_hip_modem_create(scheme, &modem));
        modem->st = stream();
        ftype = ftype_;
        k = k_;
        m = m_;
        beta = beta_;
        sm = src->m;
        sg = src->g;
        smask = src->n;
        sstate = src->state;
        pow = src->pow;
        run = symstream_run((int)k, Ls());
        stride.resize(kSymStrideWords);
        symstream_strides(pow.data(), run, stride.data());
        return alloc_dev();
    }
    bool fused() const { return modem->P.kind != MODEM_DPSK && symstream_fused_serves((int)k, Ls(), modem->P.M); }
    int reset() {                                                            // :61-65
        YG_TRY(modem->reset());
        YG_TRY(fir.bank.w.reset(stream()));
        p = 0;
        return YAGI_OK;
    }
    int set_modem(yagi_hip_modem fresh) {      // takes ownership
        YG_HIP(hipStreamSynchronize(stream()));
        (void)yagi_hip_modem_destroy(modem);
        modem = fresh;
        modem->st = stream();
        return YAGI_OK;
    }
    // samples [0, n) of a call that starts at buf_index p; sym: the caller's symbols on the device, or null (the source)
    int block_dev(const uint8_t *sym, size_t n, cf32 *y) {
        if (n == 0) return YAGI_OK;
        FirPfb<CRCF> &b = fir.bank;
        const int bps = modem->P.bps, M = modem->P.M;
        const size_t old = p > 0 ? 1 : 0;
        const size_t nnew = ((size_t)p + n + k - 1) / k - old;
        if (fused()) {
            YG_TRY(b.w.ensure_dev(b.st));
            const int *fl = nullptr;
            if (sym) {
                YG_TRY(launch_symstream_check(M, sym, nnew, flag.as<int>(), b.st));
                if (M < 256) fl = flag.as<int>();
            }
            const SymSource src{dpow.as<unsigned>(), dstride.as<unsigned>(), sstate, sg, smask, (int)sm, bps, run};
            YG_TRY(launch_symstream(b.w.dev(), b.taps.as<float>(), (int)k, b.Ls, b.scale, modem->dmap.as<cf32>(), M, gain, sym,
                                    fl, sym ? nullptr : &src, p, n, y, b.w.next(), dbuf.as<cf32>(), b.st));
            if (fl) {
                int bad = 0;
                YG_TRY(download(&bad, flag.p, sizeof(int), b.st));
                if (bad) return fail(YAGI_ERR_RANGE, "input symbol exceeds constellation size");
            }
            if (nnew) b.w.flip();              // the kernel's last workgroup wrote the next window
        } else {
            // the branches of the symbol the previous call pushed, then the parts' launchers over the new symbols
            const size_t head = p > 0 ? std::min(n, k - (size_t)p) : 0;
            if (nnew) {
                const uint8_t *s = sym;
                if (!s) {
                    YG_TRY(dsym.ensure(nnew));
                    YG_TRY(gen_symbols(nnew));
                    s = dsym.as<uint8_t>();
                }
                YG_TRY(dpts.ensure(nnew * sizeof(cf32)));
                YG_TRY(dout.ensure(nnew * k * sizeof(cf32)));
                YG_TRY(modem->modulate_dev(s, nnew, dpts.as<cf32>()));       // a symbol >= M: YAGI_ERR_RANGE, nothing moved
                YG_TRY(launch_symstream_gain(dpts.as<cf32>(), nnew, gain, b.st));
                YG_TRY(fir.block_dev(dpts.as<cf32>(), nnew, dout.as<cf32>()));
            }
            if (head)
                YG_HIP(hipMemcpyAsync(y, dbuf.as<cf32>() + p, head * sizeof(cf32), hipMemcpyDeviceToDevice, b.st));
            if (nnew) {
                YG_HIP(hipMemcpyAsync(y + head, dout.p, (n - head) * sizeof(cf32), hipMemcpyDeviceToDevice, b.st));
                YG_HIP(hipMemcpyAsync(dbuf.p, dout.as<cf32>() + (nnew - 1) * k, k * sizeof(cf32), hipMemcpyDeviceToDevice, b.st));
            }
        }
        if (!sym) sstate = msequence_skip(pow.data(), sstate, (uint64_t)nnew * (uint64_t)bps);
        p = (int)(((size_t)p + n) % k);
        return YAGI_OK;
    }
    // the source's next nnew symbols into dsym: MSequence's own generator with the object's tables
    int gen_symbols(size_t nnew) {
        if (mstride.empty()) {                 // first use of the three-launch route
            std::vector<unsigned> pw(kMseqPowWords);
            mstride.resize(kMseqStrideWords);
            msequence_tables(sg, smask, pw.data(), mstride.data());
            YG_TRY(fill(dmstride, mstride.data(), mstride.size() * sizeof(unsigned), stream()));
        }
        return launch_msequence_gen(dpow.as<unsigned>(), dmstride.as<unsigned>(), sstate, sg, smask, (int)sm, modem->P.bps, nnew,
                                    dsym.as<uint8_t>(), stream());
    }
    std::vector<unsigned> mstride;             // MSequence's block-kernel strides (three-launch route only)
    DevBuf dmstride;
    int block_host(const uint8_t *sym, size_t nsym, size_t n, cf32 *y) {
        YG_TRY(ws.y.ensure(n * sizeof(cf32)));
        const uint8_t *sd = nullptr;
        if (sym) {
            YG_TRY(ws.put(stream(), sym, nsym));
            sd = ws.x.as<uint8_t>();
        }
        YG_TRY(block_dev(sd, n, ws.y.as<cf32>()));
        return download(y, ws.y.p, n * sizeof(cf32), stream());
    }
};

static int symstream_check_source(yagi_hip_msequence src) {
    if (!src) return fail(YAGI_ERR_CONFIG, "null handle (symbol source)");
    return YAGI_OK;
}

#define SYMSTREAM_GET(name, type, expr)                                                             \
    int yagi_hip_symstreamcf_##name(yagi_hip_symstreamcf q, type *v) try {                          \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(v);                                                                               \
        *v = (expr);                                                                                \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }

extern "C" {

int yagi_hip_symstreamcf_create_linear(int ftype, size_t k, size_t m, float beta, int scheme, yagi_hip_msequence src,
                                       yagi_hip_symstreamcf *q) try {                // new_linear :24-59
    CHECK_PTR(q);
    *q = nullptr;
    if (k < 2) return fail(YAGI_ERR_CONFIG, "samples/symbol must be at least 2");
    if (m == 0) return fail(YAGI_ERR_CONFIG, "filter delay must be greater than zero");
    if (!(beta >= 0.0f && beta <= 1.0f)) return fail(YAGI_ERR_CONFIG, "filter excess bandwidth must be in (0,1]");
    int kind = 0, bps = 0;
    YG_TRY(yagi_hip_modem_s::kind_of(scheme, &kind, &bps));
    std::vector<float> h;
    YG_TRY(firinterp_prototype_taps(ftype, k, m, beta, 0.0f, h));
    YG_TRY(symstream_check_source(src));
    auto o = std::make_unique<yagi_hip_symstreamcf_s>();
    o->fir.bank.st = src->st;
    YG_TRY(o->init(ftype, k, m, beta, h.data(), h.size(), scheme, src));
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamcf_create_taps(size_t k, const float *h, size_t h_len, int scheme, yagi_hip_msequence src,
                                     yagi_hip_symstreamcf *q) try {
    CHECK_PTR(q);
    *q = nullptr;
    if (k < 2) return fail(YAGI_ERR_CONFIG, "samples/symbol must be at least 2");
    if (h_len && !h) return fail(YAGI_ERR_CONFIG, "null pointer argument");
    if (h_len < k) return fail(YAGI_ERR_CONFIG, "filter length cannot be less than interp factor");
    int kind = 0, bps = 0;
    YG_TRY(yagi_hip_modem_s::kind_of(scheme, &kind, &bps));
    YG_TRY(symstream_check_source(src));
    auto o = std::make_unique<yagi_hip_symstreamcf_s>();
    o->fir.bank.st = src->st;
    const size_t ls = (h_len + k - 1) / k;
    YG_TRY(o->init(YAGI_FIR_SHAPE_UNKNOWN, k, (ls - 1) / 2, 0.0f, h, h_len, scheme, src));
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamcf_destroy(yagi_hip_symstreamcf q) try {
    if (q) (void)hipStreamSynchronize(q->stream());
    delete q;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamcf_clone(yagi_hip_symstreamcf q, yagi_hip_symstreamcf *out) try {
    CHECK_Q(q);
    CHECK_PTR(out);
    *out = nullptr;
    FirPfb<CRCF> &qb = q->fir.bank;
    YG_TRY(qb.w.ensure_dev(qb.st));
    auto o = std::make_unique<yagi_hip_symstreamcf_s>();
    FirPfb<CRCF> &b = o->fir.bank;
    o->ftype = q->ftype;
    o->k = q->k;
    o->m = q->m;
    o->beta = q->beta;
    o->gain = q->gain;
    o->p = q->p;
    o->sm = q->sm;
    o->sg = q->sg;
    o->smask = q->smask;
    o->sstate = q->sstate;
    o->pow = q->pow;
    o->stride = q->stride;
    o->run = q->run;
    o->fir.interp = q->fir.interp;
    o->fir.hs = q->fir.hs;
    b.st = qb.st;
    b.nf = qb.nf;
    b.Ls = qb.Ls;
    b.hb = qb.hb;
    b.scale = qb.scale;
    YG_TRY(fill(b.taps, b.hb.data(), b.hb.size() * sizeof(float), b.st));
    YG_TRY(b.w.clone_from(qb.w, qb.st));
    YG_TRY(yagi_hip_modem_clone(q->modem, &o->modem));
    YG_TRY(o->alloc_dev());
    YG_HIP(hipMemcpyAsync(o->dbuf.p, q->dbuf.p, q->k * sizeof(cf32), hipMemcpyDeviceToDevice, b.st));
    YG_HIP(hipStreamSynchronize(b.st));
    *out = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamcf_set_stream(yagi_hip_symstreamcf q, yagi_stream_t s) try {
    CHECK_Q(q);
    if (q->stream() == to_stream(s)) return YAGI_OK;
    YG_HIP(hipStreamSynchronize(q->stream()));
    q->stream() = to_stream(s);
    q->modem->st = to_stream(s);
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamcf_reset(yagi_hip_symstreamcf q) try {
    CHECK_Q(q);
    return q->reset();
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamcf_source_set_state(yagi_hip_symstreamcf q, unsigned a) try {
    CHECK_Q(q);
    q->sstate = a;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

SYMSTREAM_GET(source_get_state, unsigned, q->sstate)
SYMSTREAM_GET(get_ftype, int, q->ftype)                                              // :67-69
SYMSTREAM_GET(get_k, size_t, q->k)                                                   // :71-73
SYMSTREAM_GET(get_m, size_t, q->m)                                                   // :75-77
SYMSTREAM_GET(get_beta, float, q->beta)                                              // :79-81
SYMSTREAM_GET(get_scheme, int, q->modem->scheme)                                     // :88-90
SYMSTREAM_GET(get_gain, float, q->gain)                                              // :96-98
SYMSTREAM_GET(get_delay, size_t, q->k * q->m)                                        // :100-102
SYMSTREAM_GET(get_buf_index, size_t, (size_t)q->p)
SYMSTREAM_GET(is_fused, int, q->fused() ? 1 : 0)

int yagi_hip_symstreamcf_set_scheme(yagi_hip_symstreamcf q, int scheme) try {        // :83-86
    CHECK_Q(q);
    yagi_hip_modem fresh = nullptr;
    YG_TRY(yagi_hip_modem_create(scheme, &fresh));
    return q->set_modem(fresh);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamcf_set_modem(yagi_hip_symstreamcf q, yagi_hip_modem mod) try {
    CHECK_Q(q);
    CHECK_Q(mod);
    yagi_hip_modem fresh = nullptr;
    YG_TRY(yagi_hip_modem_clone(mod, &fresh));
    return q->set_modem(fresh);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamcf_set_gain(yagi_hip_symstreamcf q, float gain) try {          // :92-94
    CHECK_Q(q);
    q->gain = gain;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamcf_write_samples(yagi_hip_symstreamcf q, yagi_cf32 *y, size_t n) try {      // :111-121
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(y);
    return q->block_host(nullptr, 0, n, y);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamcf_write_samples_dev(yagi_hip_symstreamcf q, yagi_cf32 *y_dev, size_t n) try {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(y_dev);
    return q->block_dev(nullptr, n, y_dev);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamcf_modulate_symbols(yagi_hip_symstreamcf q, const uint8_t *sym, size_t nsym, yagi_cf32 *y) try {
    CHECK_Q(q);
    if (nsym == 0) return YAGI_OK;
    CHECK_PTR(sym);
    CHECK_PTR(y);
    if (q->p != 0) return fail(YAGI_ERR_MODE, "modulate_symbols needs a symbol boundary (buf_index is %d)", q->p);
    for (size_t i = 0; i < nsym; ++i)
        if ((int)sym[i] >= q->modem->P.M) return fail(YAGI_ERR_RANGE, "input symbol %zu exceeds constellation size", i);
    return q->block_host(sym, nsym, nsym * q->k, y);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamcf_modulate_symbols_dev(yagi_hip_symstreamcf q, const uint8_t *sym_dev, size_t nsym,
                                              yagi_cf32 *y_dev) try {
    CHECK_Q(q);
    if (nsym == 0) return YAGI_OK;
    CHECK_PTR(sym_dev);
    CHECK_PTR(y_dev);
    if (q->p != 0) return fail(YAGI_ERR_MODE, "modulate_symbols needs a symbol boundary (buf_index is %d)", q->p);
    CHECK_NOALIAS(sym_dev, nsym, y_dev, nsym * q->k);
    return q->block_dev(sym_dev, nsym * q->k, y_dev);
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"

// ---- SymStreamR (src/framing/symstreamr.rs) ---------------------------------------------------------------------------
// The reference's fields: a SymStream at k = 2, an MsResamp of rate 0.5 / bw and buf (the outputs of the last pushed
// sample that no call has taken yet).  Both parts are the library's own objects, so the composition route is their
// device forms one after the other; the fused route (symstreamr_kernels.hip) forms the SymStream's samples and the
// MsResamp's arbitrary stage in one launch on the same state, and the MsResamp's half-band chain follows unchanged.
// The schedule is host arithmetic on the Resamp's integer phase: no call reads anything back.
namespace yagi {

// MsResamp::new's split of the rate (msresamp.rs:33-51) and the Resamp's step for what remains
static void symstreamr_split(float rate, int *interp, size_t *stages, float *rate_arb, uint32_t *step) {
    *interp = rate > 1.0f ? 1 : 0;
    *stages = 0;
    float ra = rate;
    if (*interp) {
        while (ra > 2.0f) { ++*stages; ra *= 0.5f; }
    } else {
        while (ra < 0.5f) { ++*stages; ra *= 2.0f; }
    }
    *rate_arb = ra;
    *step = (uint32_t)std::round(16777216.0f / ra);
}

// inputs the arbitrary stage needs from phase p0 for q outputs, and all the outputs they give
static size_t symstreamr_need(uint32_t p0, uint32_t step, size_t q, size_t *outputs, uint32_t *next) {
    if (q == 0) {
        if (outputs) *outputs = 0;
        if (next) *next = p0;
        return 0;
    }
    const unsigned __int128 a = (unsigned __int128)p0 + (unsigned __int128)(q - 1) * step;
    const size_t need = (size_t)(a >> 24) + 1;
    const unsigned __int128 end = (unsigned __int128)need << 24;
    const size_t n = (size_t)((end - p0 + step - 1) / step);
    if (outputs) *outputs = n;
    if (next) *next = (uint32_t)((unsigned __int128)p0 + (unsigned __int128)n * step - end);
    return need;
}

static int symstreamr_check_bw(float bw) {
    if (!std::isfinite(bw) || !(bw >= 0.001f && bw <= 1.0f))
        return fail(YAGI_ERR_CONFIG, "symbol bandwidth (%g) must be in [0.001,1]", (double)bw);
    return YAGI_OK;
}

}  // namespace yagi

struct yagi_hip_symstreamrcf_s {
    yagi_hip_symstreamcf S = nullptr;          // owned, k = 2
    yagi_hip_msresamp_crcf R = nullptr;        // owned
    DevBuf left;                               // 2 * 2^stages values: outputs pushed but not taken
    size_t left_off = 0, left_len = 0;
    DevBuf ds, dy;                             // composition route: the SymStream's samples, the MsResamp's outputs
    Staging ws;

    ~yagi_hip_symstreamrcf_s() {
        if (S) (void)yagi_hip_symstreamcf_destroy(S);
        if (R) (void)yagi_hip_msresamp_crcf_destroy(R);
    }
    hipStream_t stream() { return S->stream(); }
    size_t left_cap() const { return (size_t)2 << R->num_stages; }
    bool fused() const {
        return S->fused() && symstreamr_fused_serves(R->arb->step, R->arb->bank.Ls, S->Ls(), S->modem->P.M, S->run);
    }
    int copy_dev(cf32 *dst, const cf32 *src, size_t n) {
        if (n) YG_HIP(hipMemcpyAsync(dst, src, n * sizeof(cf32), hipMemcpyDeviceToDevice, stream()));
        return YAGI_OK;
    }
    int reset() {
        YG_TRY(yagi_hip_symstreamcf_reset(S));
        YG_TRY(yagi_hip_msresamp_crcf_reset(R));
        left_off = left_len = 0;
        return YAGI_OK;
    }
    // the next n samples of the stream to y (device)
    int write_dev(cf32 *y, size_t n) {
        cf32 *lb = left.as<cf32>();
        const size_t c = std::min(n, left_len);
        YG_TRY(copy_dev(y, lb + left_off, c));
        left_off += c;
        left_len -= c;
        const size_t miss = n - c;
        if (miss == 0) return YAGI_OK;
        y += c;
        auto &A = *R->arb;
        const size_t ns = R->num_stages;
        const size_t q = (miss + R->group() - 1) >> ns;
        size_t n1 = 0;
        uint32_t next = 0;
        const size_t need = symstreamr_need(A.phase, A.step, q, &n1, &next);
        if (ns) YG_TRY(R->mid.ensure(n1 * sizeof(cf32)));
        if (!fused()) {
            // the composition: S's samples into scratch, then R's arbitrary stage -- into the stream between R's two parts
            // where half-band stages follow, else into scratch from where the two parts of the call are copied out
            YG_TRY(ds.ensure(need * sizeof(cf32)));
            YG_TRY(S->block_dev(nullptr, need, ds.as<cf32>()));
            if (ns == 0) {
                YG_TRY(dy.ensure(n1 * sizeof(cf32)));
                YG_TRY(A.block_dev(ds.as<cf32>(), need, dy.as<cf32>(), n1));
                YG_TRY(copy_dev(y, dy.as<cf32>(), miss));
                YG_TRY(copy_dev(lb, dy.as<cf32>() + miss, n1 - miss));
            } else {
                YG_TRY(A.block_dev(ds.as<cf32>(), need, R->mid.as<cf32>(), n1));
            }
        } else {
            FirPfb<CRCF> &sb = S->fir.bank, &rb = A.bank;
            YG_TRY(sb.w.ensure_dev(sb.st));
            YG_TRY(rb.w.ensure_dev(rb.st));
            const int bps = S->modem->P.bps, M = S->modem->P.M, p = S->p;
            const SymSource src{S->dpow.as<unsigned>(), S->dstride.as<unsigned>(), S->sstate, S->sg, S->smask, (int)S->sm, bps,
                                S->run};
            cf32 *ya = ns ? R->mid.as<cf32>() : y, *yb = ns ? ya : lb;
            YG_TRY(launch_symstreamr(sb.w.dev(), sb.taps.as<float>(), sb.Ls, sb.scale, S->modem->dmap.as<cf32>(), M, S->gain,
                                     src, p, rb.w.dev(), rb.taps.as<float>(), rb.Ls, A.bits, A.step, A.phase, need, n1, ya,
                                     ns ? n1 : miss, yb, sb.w.next(), rb.w.next(), S->dbuf.as<cf32>(), sb.st));
            const size_t nnew = ((size_t)p + need + 1) / 2 - (p > 0 ? 1 : 0);
            if (nnew) {
                sb.w.flip();
                S->sstate = msequence_skip(S->pow.data(), S->sstate, (uint64_t)nnew * (uint64_t)bps);
            }
            S->p = (int)(((size_t)p + need) % 2);
            rb.w.flip();
            A.phase = next;
        }
        if (ns == 0) {
            left_off = 0;
            left_len = n1 - miss;
            return YAGI_OK;
        }
        // the half-band chain: whole groups straight to y, the last ones to the leftover and their requested part copied out
        const cf32 *mid = R->mid.as<cf32>();
        const size_t gfull = miss >> ns, rem = n1 - gfull, tail = miss - (gfull << ns);
        YG_TRY(R->half->block_dev(mid, gfull, y));
        YG_TRY(R->half->block_dev(mid + gfull, rem, lb));
        YG_TRY(copy_dev(y + (gfull << ns), lb, tail));
        left_off = tail;
        left_len = (rem << ns) - tail;
        return YAGI_OK;
    }
    int write_host(cf32 *y, size_t n) {
        YG_TRY(ws.y.ensure(n * sizeof(cf32)));
        YG_TRY(write_dev(ws.y.as<cf32>(), n));
        return download(y, ws.y.p, n * sizeof(cf32), stream());
    }
};

#define SYMSTREAMR_GET(name, type, expr)                                                            \
    int yagi_hip_symstreamrcf_##name(yagi_hip_symstreamrcf q, type *v) try {                        \
        CHECK_Q(q);                                                                                 \
        CHECK_PTR(v);                                                                               \
        *v = (expr);                                                                                \
        return YAGI_OK;                                                                             \
    } catch (...) { return ::yagi::api_exception(); }

extern "C" {

int yagi_hip_symstreamrcf_create_linear(int ftype, float bw, size_t m, float beta, int scheme, yagi_hip_msequence src,
                                        yagi_hip_symstreamrcf *q) try {              // new_linear :23-53
    CHECK_PTR(q);
    *q = nullptr;
    YG_TRY(symstreamr_check_bw(bw));
    auto o = std::make_unique<yagi_hip_symstreamrcf_s>();
    YG_TRY(yagi_hip_symstreamcf_create_linear(ftype, 2, m, beta, scheme, src, &o->S));
    YG_TRY(yagi_hip_msresamp_crcf_create(0.5f / bw, 60.0f, &o->R));
    YG_TRY(yagi_hip_msresamp_crcf_set_stream(o->R, (yagi_stream_t)o->S->stream()));
    YG_TRY(o->left.alloc(o->left_cap() * sizeof(cf32)));
    *q = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamrcf_destroy(yagi_hip_symstreamrcf q) try {
    if (q && q->S) (void)hipStreamSynchronize(q->stream());
    delete q;
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamrcf_clone(yagi_hip_symstreamrcf q, yagi_hip_symstreamrcf *out) try {
    CHECK_Q(q);
    CHECK_PTR(out);
    *out = nullptr;
    auto o = std::make_unique<yagi_hip_symstreamrcf_s>();
    YG_TRY(yagi_hip_symstreamcf_clone(q->S, &o->S));
    YG_TRY(yagi_hip_msresamp_crcf_clone(q->R, &o->R));
    YG_TRY(o->left.alloc(o->left_cap() * sizeof(cf32)));
    o->left_off = q->left_off;
    o->left_len = q->left_len;
    YG_TRY(o->copy_dev(o->left.as<cf32>(), q->left.as<cf32>(), q->left_cap()));
    YG_HIP(hipStreamSynchronize(o->stream()));
    *out = o.release();
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamrcf_set_stream(yagi_hip_symstreamrcf q, yagi_stream_t s) try {
    CHECK_Q(q);
    YG_TRY(yagi_hip_symstreamcf_set_stream(q->S, s));
    return yagi_hip_msresamp_crcf_set_stream(q->R, s);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamrcf_reset(yagi_hip_symstreamrcf q) try {                        // :55-60
    CHECK_Q(q);
    return q->reset();
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamrcf_source_set_state(yagi_hip_symstreamrcf q, unsigned a) try {
    CHECK_Q(q);
    return yagi_hip_symstreamcf_source_set_state(q->S, a);
} catch (...) { return ::yagi::api_exception(); }

SYMSTREAMR_GET(source_get_state, unsigned, q->S->sstate)
SYMSTREAMR_GET(get_ftype, int, q->S->ftype)                                           // :62-64
SYMSTREAMR_GET(get_bw, float, 1.0f / (q->R->rate * (float)q->S->k))                   // :66-68
SYMSTREAMR_GET(get_m, size_t, q->S->m)                                                // :70-72
SYMSTREAMR_GET(get_beta, float, q->S->beta)                                           // :74-76
SYMSTREAMR_GET(get_scheme, int, q->S->modem->scheme)                                  // :82-84
SYMSTREAMR_GET(get_gain, float, q->S->gain)                                           // :90-92
SYMSTREAMR_GET(get_delay, float, ((float)(q->S->k * q->S->m) + q->R->delay()) * q->R->rate)   // :94-99
SYMSTREAMR_GET(get_pending, size_t, q->left_len)
SYMSTREAMR_GET(is_fused, int, q->fused() ? 1 : 0)

int yagi_hip_symstreamrcf_get_params(yagi_hip_symstreamrcf q, int *interp, size_t *num_halfband_stages,
                                     float *rate_arbitrary) try {
    CHECK_Q(q);
    return yagi_hip_msresamp_crcf_get_params(q->R, interp, num_halfband_stages, rate_arbitrary);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamrcf_set_scheme(yagi_hip_symstreamrcf q, int scheme) try {       // :78-80
    CHECK_Q(q);
    return yagi_hip_symstreamcf_set_scheme(q->S, scheme);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamrcf_set_modem(yagi_hip_symstreamrcf q, yagi_hip_modem mod) try {
    CHECK_Q(q);
    return yagi_hip_symstreamcf_set_modem(q->S, mod);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamrcf_set_gain(yagi_hip_symstreamrcf q, float gain) try {         // :86-88
    CHECK_Q(q);
    return yagi_hip_symstreamcf_set_gain(q->S, gain);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamrcf_write_samples(yagi_hip_symstreamrcf q, yagi_cf32 *y, size_t n) try {    // :118-128
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(y);
    return q->write_host(y, n);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_symstreamrcf_write_samples_dev(yagi_hip_symstreamrcf q, yagi_cf32 *y_dev, size_t n) try {
    CHECK_Q(q);
    if (n == 0) return YAGI_OK;
    CHECK_PTR(y_dev);
    if ((uintptr_t)y_dev & 7) return fail(YAGI_ERR_CONFIG, "symstreamr: sample buffers must be 8-byte aligned");
    return q->write_dev(y_dev, n);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_plan_symstreamr(float bw, size_t m, size_t n, uint32_t p0, yagi_hip_symstreamr_plan *out) try {
    CHECK_PTR(out);
    *out = yagi_hip_symstreamr_plan{};
    YG_TRY(symstreamr_check_bw(bw));
    if (m == 0 || m > ((size_t)1 << 20)) return fail(YAGI_ERR_CONFIG, "filter delay must be in [1, 2^20]");
    const float rate = 0.5f / bw;
    symstreamr_split(rate, &out->interp, &out->stages, &out->rate_arb, &out->step);
    out->rate = rate;
    const int Lr = 14, Ls = (int)(2 * m + 1), run = symstream_run(2, Ls);     // MsResamp's Resamp has m = 7
    out->tile = symstreamr_tile(out->step, Lr);
    out->max_wg_tiles = symstreamr_fused_serves(out->step, Lr, Ls, 256, run) ? symstreamr_max_tiles(out->step, Lr, Ls, run) : 0;
    out->q = (n + ((size_t)1 << out->stages) - 1) >> out->stages;
    out->need = symstreamr_need(p0, out->step, out->q, &out->outputs_arb, &out->phase_next);
    out->outputs = out->outputs_arb << out->stages;
    out->leftover = out->outputs - n;
    if (out->max_wg_tiles && out->outputs_arb) {
        out->wg_tiles = symstreamr_wg_tiles(out->step, Lr, Ls, run, out->outputs_arb);
        out->lds = symstreamr_lds_bytes(out->step, Lr, Ls, 256, out->wg_tiles);
    }
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

}  // extern "C"
