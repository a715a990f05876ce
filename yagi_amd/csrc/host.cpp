// host.cpp -- host-only pieces of libyagi_hip.so: error reporting and the design-time scalar
// maths the constructors need (Kaiser-windowed sinc taps).  Design code runs once per object
// on the CPU in the reference as well; it is not on the hot path.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace yagi {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

int fail(int status, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return status;
}

// translate the exception in flight (called from a catch (...) block) into a status + message
int api_exception() noexcept {
    const char *what = "unexpected C++ exception";
    std::string msg;
    try {
        throw;
    } catch (const std::bad_alloc &) {
        what = "out of host memory";
    } catch (const std::exception &e) {
        try { msg = std::string("unexpected C++ exception: ") + e.what(); what = msg.c_str(); } catch (...) {}
    } catch (...) {
    }
    try { g_last_error = what; } catch (...) {}
    return YAGI_ERR_INTERNAL;
}

// ---- Kaiser design, single precision like the reference -----------------------------------
// ln Gamma(z): recursion below 10, Stirling-type series above (math/gamma.rs:7-22)
static float ln_gamma(float z) {
    // below 10 step up with lnGamma(z) = lnGamma(z+1) - ln z; the subtractions are applied
    // largest argument first, which is the order the reference's recursion produces
    float logs[16];
    int nlog = 0;
    while (z < 10.0f && nlog < 16) {
        logs[nlog++] = std::log(z);
        z += 1.0f;
    }
    const float two_pi = 2.0f * 3.14159265358979323846f;
    float g = 0.5f * (std::log(two_pi) - std::log(z));
    g += z * (std::log(z + 1.0f / (12.0f * z - 0.1f / z)) - 1.0f);
    for (int i = nlog - 1; i >= 0; --i) g -= logs[i];
    return g;
}

// I0(z) through the log-domain series the reference uses (math/bessel.rs:9-67)
static float bessel_i0(float z) {
    if (z == 0.0f) return 1.0f;
    if (z < 1e-3f) return 1.0f / std::exp(ln_gamma(1.0f));
    const float lhz = std::log(0.5f * z);
    float acc = 0.0f;
    for (int k = 0; k < 64; ++k) {
        const float kf = static_cast<float>(k);
        const float lg = ln_gamma(kf + 1.0f);
        acc += std::exp(2.0f * kf * lhz - lg - lg);
    }
    return std::exp(0.0f + std::log(acc));
}

static float sinc(float x) {     // math/mod.rs:63-69
    const float pi = 3.14159265358979323846f;
    if (std::fabs(x) < 0.01f)
        return std::cos(pi * x / 2.0f) * std::cos(pi * x / 4.0f) * std::cos(pi * x / 8.0f);
    return std::sin(pi * x) / (pi * x);
}

static float kaiser_beta(float as_) {     // kaiser.rs:62-72
    const float a = std::fabs(as_);
    if (a > 50.0f) return 0.1102f * (a - 8.7f);
    if (a > 21.0f) return 0.5842f * std::pow(a - 21.0f, 0.4f) + 0.07886f * (a - 21.0f);
    return 0.0f;
}

// fir_design_kaiser (kaiser.rs:16-51) with windows::kaiser (math/windows.rs:76-90)
int design_kaiser(size_t n, float fc, float as_, float mu, std::vector<float> &h) {
    if (mu <= -0.5f || mu > 0.5f)
        return fail(YAGI_ERR_CONFIG, "fractional sample offset (%g) out of range (-0.5, 0.5)", mu);
    if (fc <= 0.0f || fc > 0.5f)
        return fail(YAGI_ERR_CONFIG, "cutoff frequency (%g) out of range (0, 0.5)", fc);
    if (n == 0) return fail(YAGI_ERR_CONFIG, "filter length must be greater than zero");
    if (as_ <= 0.0f) return fail(YAGI_ERR_CONFIG, "stop-band attenuation must be greater than zero");
    const float beta = kaiser_beta(as_);
    const float i0_beta = bessel_i0(beta);
    h.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const float t = static_cast<float>(i) - (static_cast<float>(n) - 1.0f) / 2.0f + mu;
        const float proto = sinc(2.0f * fc * t);
        const float tw = static_cast<float>(i) - static_cast<float>(n - 1) / 2.0f;
        const float r = 2.0f * tw / static_cast<float>(n - 1);
        const float win = bessel_i0(beta * std::sqrt(1.0f - r * r)) / i0_beta;
        h[i] = proto * win;
    }
    return YAGI_OK;
}

// ---- (root-)Nyquist prototypes (design/mod.rs:392-451), single precision like the reference ----------------
// estimate_req_filter_len_kaiser (design/mod.rs:228-238), [Vaidyanathan:1993]
static int filter_len_kaiser(float df, float as_, float *n) {
    if (df > 0.5f || df <= 0.0f) return fail(YAGI_ERR_CONFIG, "cutoff frequency (%g) out of range (0, 0.5)", (double)df);
    if (as_ <= 0.0f) return fail(YAGI_ERR_CONFIG, "stopband attenuation must be greater than zero");
    *n = (as_ - 7.95f) / (14.26f * df);
    return YAGI_OK;
}

// estimate_req_filter_stopband_attenuation (design/mod.rs:161-184): twenty bisections of [0.01, 200] dB on the Kaiser
// length estimate
int estimate_stopband_attenuation(float df, size_t n, float *as_) {
    float as0 = 0.01f, as1 = 200.0f, as_hat = 0.0f;
    for (int it = 0; it < 20; ++it) {
        as_hat = 0.5f * (as1 + as0);
        float n_hat = 0.0f;
        YG_TRY(filter_len_kaiser(df, as_hat, &n_hat));
        if (n_hat < static_cast<float>(n)) as0 = as_hat;
        else as1 = as_hat;
    }
    *as_ = as_hat;
    return YAGI_OK;
}

static int check_nyquist_args(size_t k, size_t m, float beta) {       // rcos.rs:18-26, rrcos.rs:16-24
    if (k < 1) return fail(YAGI_ERR_CONFIG, "k must be greater than 0");
    if (m < 1) return fail(YAGI_ERR_CONFIG, "m must be greater than 0");
    if (beta < 0.0f || beta > 1.0f) return fail(YAGI_ERR_CONFIG, "beta must be in [0,1]");
    return YAGI_OK;
}

// fir_design_rcos (rcos.rs:17-51)
static int design_rcos(size_t k, size_t m, float beta, float dt, std::vector<float> &h) {
    YG_TRY(check_nyquist_args(k, m, beta));
    const float pi = 3.14159265358979323846f;
    const float kf = static_cast<float>(k), mf = static_cast<float>(m);
    h.resize(2 * k * m + 1);
    for (size_t n = 0; n < h.size(); ++n) {
        const float z = (static_cast<float>(n) + dt) / kf - mf;
        const float t1 = std::cos(beta * pi * z);
        const float t2 = sinc(z);
        const float t3 = 1.0f - 4.0f * beta * beta * z * z;
        // where 4 beta^2 z^2 reaches 1 the quotient is 0 / 0: its limit
        h[n] = std::fabs(t3) < 1e-3f ? std::sin(pi / (2.0f * beta)) * beta * 0.5f : t1 * t2 / t3;
    }
    return YAGI_OK;
}

// fir_design_rrcos (rrcos.rs:15-63): the closed form and its two limits, at z = 0 and at 16 beta^2 z^2 = 1
static int design_rrcos(size_t k, size_t m, float beta, float dt, std::vector<float> &h) {
    YG_TRY(check_nyquist_args(k, m, beta));
    const float pi = 3.14159265358979323846f;
    const float kf = static_cast<float>(k), mf = static_cast<float>(m);
    h.resize(2 * k * m + 1);
    for (size_t n = 0; n < h.size(); ++n) {
        const float z = (static_cast<float>(n) + dt) / kf - mf;
        if (std::fabs(z) < 1e-5f) {
            h[n] = 1.0f - beta + 4.0f * beta / pi;
            continue;
        }
        float g = 1.0f - 16.0f * beta * beta * z * z;
        g *= g;
        if (std::fabs(g) < 1e-5f) {
            const float g1 = 1.0f + 2.0f / pi, g2 = std::sin(0.25f * pi / beta);
            const float g3 = 1.0f - 2.0f / pi, g4 = std::cos(0.25f * pi / beta);
            h[n] = beta / std::sqrt(2.0f) * (g1 * g2 + g3 * g4);
        } else {
            const float t1 = std::cos((1.0f + beta) * pi * z);
            const float t2 = std::sin((1.0f - beta) * pi * z);
            const float t3 = 1.0f / (4.0f * beta * z);
            const float t4 = 4.0f * beta / (pi * (1.0f - (16.0f * beta * beta * z * z)));
            h[n] = t4 * (t1 + (t2 * t3));
        }
    }
    return YAGI_OK;
}

// fir_design_arkaiser (rkaiser.rs:49-93): a Kaiser-windowed sinc whose transition band is narrowed by rho and whose
// cutoff is moved up to match, rho from the closed form rho ~ c0 + c1 ln(beta) + c2 ln^2(beta); normalised to sum h^2 = k.
// Where that form leaves (0, 1) the reference falls back on a table of fitted constants (rkaiser.rs:105-144), which is
// not part of this library: those shapes are a configuration error here.
static int design_arkaiser(size_t k, size_t m, float beta, float dt, std::vector<float> &h) {
    if (k < 2) return fail(YAGI_ERR_CONFIG, "k must be at least 2");
    if (m < 1) return fail(YAGI_ERR_CONFIG, "m must be at least 1");
    if (beta <= 0.0f || beta >= 1.0f) return fail(YAGI_ERR_CONFIG, "beta must be in (0,1)");
    if (dt < -1.0f || dt > 1.0f) return fail(YAGI_ERR_CONFIG, "dt must be in [-1,1]");
    const float mf = static_cast<float>(m);
    const float c0 = 0.762886f + 0.067663f * std::log(mf);
    const float c1 = 0.065515f;
    const float c2 = std::log(1.0f - 0.088f * std::pow(mf, -1.6f));
    const float log_beta = std::log(beta);
    const float rho_hat = c0 + c1 * log_beta + c2 * log_beta * log_beta;
    if (!(rho_hat > 0.0f && rho_hat < 1.0f))
        return fail(YAGI_ERR_CONFIG,
                    "arkaiser: the closed-form bandwidth correction rho (%g) leaves (0, 1) at m = %zu, beta = %g; "
                    "the reference's fitted fallback table is not part of this library",
                    (double)rho_hat, m, (double)beta);
    const size_t n = 2 * k * m + 1;
    const float kf = static_cast<float>(k);
    const float del = beta * rho_hat / kf;
    float as_ = 0.0f;
    YG_TRY(estimate_stopband_attenuation(del, n, &as_));
    const float fc = 0.5f * (1.0f + beta * (1.0f - rho_hat)) / kf;
    YG_TRY(design_kaiser(n, fc, as_, dt, h));
    float e2 = 0.0f;
    for (float v : h) e2 += v * v;
    const float s = std::sqrt(kf / e2);
    for (float &v : h) v *= s;
    return YAGI_OK;
}

// fir_design_prototype (design/mod.rs:392-451) for the shapes built here; ftype is numbered as FirFilterShape
// (design/mod.rs:41-77).  The stop-band estimate comes first, as there, so beta = 0 fails in it for every shape.
int design_prototype(int ftype, size_t k, size_t m, float beta, float dt, std::vector<float> &h) {
    static const char *const names[] = {"kaiser", "pm", "rcos", "fexp", "fsech", "farcsech", "arkaiser", "rkaiser",
                                        "rrcos", "hm3", "gmsktx", "gmskrx", "rfexp", "rfsech", "rfarcsech"};
    if (ftype < 0 || ftype >= (int)(sizeof names / sizeof *names)) return fail(YAGI_ERR_CONFIG, "unknown filter shape %d", ftype);
    if (ftype != YAGI_FIR_SHAPE_KAISER && ftype != YAGI_FIR_SHAPE_RCOS && ftype != YAGI_FIR_SHAPE_RRCOS &&
        ftype != YAGI_FIR_SHAPE_ARKAISER)
        return fail(YAGI_ERR_CONFIG, "filter shape %s is not built (its design code is not part of this library)", names[ftype]);
    if (k < 1) return fail(YAGI_ERR_CONFIG, "k must be greater than 0");
    if (m < 1) return fail(YAGI_ERR_CONFIG, "m must be greater than 0");
    if (k > ((size_t)1 << 20) || m > ((size_t)1 << 20) || k * m > ((size_t)1 << 24))
        return fail(YAGI_ERR_CONFIG, "prototype too long (k = %zu, m = %zu)", k, m);
    const size_t h_len = 2 * k * m + 1;
    const float fc = 0.5f / static_cast<float>(k);
    const float df = beta / static_cast<float>(k);
    float as_ = 0.0f;
    YG_TRY(estimate_stopband_attenuation(df, h_len, &as_));
    switch (ftype) {
    case YAGI_FIR_SHAPE_KAISER: return design_kaiser(h_len, fc, as_, dt, h);
    case YAGI_FIR_SHAPE_RCOS: return design_rcos(k, m, beta, dt, h);
    case YAGI_FIR_SHAPE_RRCOS: return design_rrcos(k, m, beta, dt, h);
    default: return design_arkaiser(k, m, beta, dt, h);
    }
}

// fir_design_notch (design/mod.rs:336-378): 1 - (Kaiser-windowed tone at f0, normalised to unit gain at f0)
int design_notch(size_t m, float f0, float as_, std::vector<float> &h) {
    if (m < 1 || m > 1000) return fail(YAGI_ERR_CONFIG, "filter semi-length (%zu) out of range [1,1000]", m);
    if (f0 < -0.5f || f0 > 0.5f) return fail(YAGI_ERR_CONFIG, "notch frequency (%g) out of range [-0.5,0.5]", (double)f0);
    if (as_ <= 0.0f) return fail(YAGI_ERR_CONFIG, "stop-band attenuation must be greater than zero");
    const size_t n = 2 * m + 1;
    const float beta = kaiser_beta(as_);
    const float i0_beta = bessel_i0(beta);
    h.assign(n, 0.0f);
    float scale = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        const float p = -std::cos(2.0f * 3.14159265358979323846f * f0 * (static_cast<float>(i) - static_cast<float>(m)));
        const float tw = static_cast<float>(i) - static_cast<float>(n - 1) / 2.0f;
        const float r = 2.0f * tw / static_cast<float>(n - 1);
        const float w = bessel_i0(beta * std::sqrt(1.0f - r * r)) / i0_beta;
        h[i] = p * w;
        scale += h[i] * p;
    }
    for (size_t i = 0; i < n; ++i) h[i] /= scale;
    h[m] += 1.0f;
    return YAGI_OK;
}

// ---- taper windows for Spgram (math/windows.rs:76-205), single precision like the reference -------
// type: 1 Hamming, 2 Hann, 3 BlackmanHarris, 4 BlackmanHarris7, 5 Kaiser, 6 FlatTop, 7 Triangular,
//       8 RcosTaper, 9 Kbd (the reference's WindowType discriminants)
static float kaiser_window(size_t i, size_t wlen, float beta) {
    const float t = static_cast<float>(i) - static_cast<float>(wlen - 1) / 2.0f;
    const float r = 2.0f * t / static_cast<float>(wlen - 1);
    return bessel_i0(beta * std::sqrt(1.0f - r * r)) / bessel_i0(beta);
}

int window_value(int type, size_t i, size_t wlen, float arg, float *out) {
    const float pi = 3.14159265358979323846f;
    const float t = 2.0f * pi * static_cast<float>(i) / static_cast<float>(wlen - 1);
    switch (type) {
        case 1: *out = 0.53836f - 0.46164f * std::cos((2.0f * pi * static_cast<float>(i)) / static_cast<float>(wlen - 1)); return YAGI_OK;
        case 2: *out = 0.5f - 0.5f * std::cos((2.0f * pi * static_cast<float>(i)) / static_cast<float>(wlen - 1)); return YAGI_OK;
        case 3: *out = 0.35875f - 0.48829f * std::cos(t) + 0.14128f * std::cos(2.0f * t) - 0.01168f * std::cos(3.0f * t); return YAGI_OK;
        case 4:
            *out = 0.27105f - 0.43329f * std::cos(t) + 0.21812f * std::cos(2.0f * t) - 0.06592f * std::cos(3.0f * t) +
                   0.01081f * std::cos(4.0f * t) - 0.00077f * std::cos(5.0f * t) + 0.00001f * std::cos(6.0f * t);
            return YAGI_OK;
        case 5:
            if (arg < 0.0f) return fail(YAGI_ERR_VALUE, "Kaiser window: beta must be greater than or equal to zero");
            *out = kaiser_window(i, wlen, arg);
            return YAGI_OK;
        case 6: *out = 1.000f - 1.930f * std::cos(t) + 1.290f * std::cos(2.0f * t) - 0.388f * std::cos(3.0f * t) + 0.028f * std::cos(4.0f * t); return YAGI_OK;
        case 7: {
            const size_t n = static_cast<size_t>(arg);
            if (n + 1 != wlen && n != wlen && n != wlen + 1)
                return fail(YAGI_ERR_VALUE, "Triangular window: sub-length must be in wlen+{-1,0,1}");
            if (n == 0) return fail(YAGI_ERR_VALUE, "Triangular window: sub-length must be greater than zero");
            const float v0 = static_cast<float>(i) - static_cast<float>(wlen - 1) / 2.0f;
            *out = 1.0f - std::fabs(v0 / (static_cast<float>(n) / 2.0f));
            return YAGI_OK;
        }
        case 8: {
            const size_t tp = static_cast<size_t>(arg);
            if (tp > wlen / 2) return fail(YAGI_ERR_VALUE, "Raised-cosine taper window: taper length cannot exceed half window length");
            size_t ii = i;
            if (ii > wlen - tp - 1) ii = wlen - ii - 1;
            *out = (ii < tp) ? 0.5f - 0.5f * std::cos(pi * (static_cast<float>(ii) + 0.5f) / static_cast<float>(tp)) : 1.0f;
            return YAGI_OK;
        }
        case 9: {
            if (wlen % 2 != 0) return fail(YAGI_ERR_VALUE, "KBD window: window length must be even");
            const size_t m = wlen / 2;
            const size_t ii = (i >= m) ? wlen - i - 1 : i;
            float w0 = 0.0f, w1 = 0.0f;
            for (size_t j = 0; j <= m; ++j) {
                const float wv = kaiser_window(j, m + 1, arg);
                w1 += wv;
                if (j <= ii) w0 += wv;
            }
            *out = std::sqrt(w0 / w1);
            return YAGI_OK;
        }
        default: return fail(YAGI_ERR_CONFIG, "unknown window type");
    }
}

// ---------------------------------------------------------------------------------------------
// Per-sample arithmetic of the FIR objects on the host mirror of their window (capi.hip DevWindow): what
// FirFilter::execute (firfilt.rs:241-246), FirPfbFilter::execute (firpfb.rs:277-286) and
// FirDecimationFilter::execute (firdecim.rs:179-191) compute, in the reference's order: products unfused, every
// sum left to right from zero (dotprod/mod.rs:19-73: `iter().zip().map(|(a, b)| a * b).sum()`), the scale applied to
// the finished sum.  This is product code (tens of nanoseconds per call), not the test oracle.
// ---------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
namespace {
inline float h_mul(float a, float b) { return a * b; }
inline cf32 h_mul(cf32 a, float b) { return cf32{a.re * b, a.im * b}; }
inline cf32 h_mul(cf32 a, cf32 b) { return cf32{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
inline float h_add(float a, float b) { return a + b; }
inline cf32 h_add(cf32 a, cf32 b) { return cf32{a.re + b.re, a.im + b.im}; }
}  // namespace

// FirFilter: the state is a VecDeque with the NEWEST sample first (push = rotate_right(1) + w[0] = x, :220-223), summed
// against h[0..L) as two slices (dotprod/mod.rs:75-121): the ring wraps `split = L - head` samples from its start.
// w = the window oldest first (w[L-1] = newest), head = the VecDeque's physical head.
template <class T, class C>
T host_fir_ring_dot(const T *w, size_t L, size_t head, const C *h, C scale) {
    const size_t split = L - head;
    T l{}, r{};
    const T *newest = w + (L - 1);
    for (size_t k = 0; k < split; ++k) l = h_add(l, h_mul(newest[-(ptrdiff_t)k], h[k]));
    for (size_t k = split; k < L; ++k) r = h_add(r, h_mul(newest[-(ptrdiff_t)k], h[k]));
    return h_mul(h_add(l, r), scale);
}
// Window-based objects: the contiguous window oldest first against the taps reversed (firdecim.rs:47, firpfb.rs:45-52);
// h = the taps in natural order (h[0] meets the newest sample)
template <class T, class C>
T host_fir_window_dot(const T *w, size_t L, const C *h, C scale) {
    T s{};
    for (size_t k = 0; k < L; ++k) s = h_add(s, h_mul(w[k], h[L - 1 - k]));
    return h_mul(s, scale);
}
template float host_fir_ring_dot<float, float>(const float *, size_t, size_t, const float *, float);
template cf32 host_fir_ring_dot<cf32, float>(const cf32 *, size_t, size_t, const float *, float);
template cf32 host_fir_ring_dot<cf32, cf32>(const cf32 *, size_t, size_t, const cf32 *, cf32);
template float host_fir_window_dot<float, float>(const float *, size_t, const float *, float);
template cf32 host_fir_window_dot<cf32, float>(const cf32 *, size_t, const float *, float);
template cf32 host_fir_window_dot<cf32, cf32>(const cf32 *, size_t, const cf32 *, cf32);


// IirFilter per-sample steps on the host mirror of the state (capi.hip IirObj), in the reference's order.
// Transfer function (iirfilt.rs:359-374): s = the VecDeque's logical v[0 .. n-1) (newest first), *head = its physical
// head; rotate_right(1) moves the head back one slot and as_slices() then splits the dot products at n - head
// (dotprod/mod.rs:75-121: each slice summed left to right from zero, then l + r).  Returns the unscaled output.
template <class T, class C>
T host_iir_tf_step(T *s, size_t S, size_t *head, const C *a, const C *b, T x) {
    const size_t n = S + 1;
    *head = (*head == 0) ? n - 1 : *head - 1;
    const size_t split = (*head == 0) ? n : n - *head;
    T l{}, r{};
    l = h_add(l, h_mul(T{}, a[0]));                     // v[0] = 0 during the feedback sum
    for (size_t i = 1; i < n; ++i) {
        const T q = h_mul(s[i - 1], a[i]);
        if (i < split) l = h_add(l, q); else r = h_add(r, q);
    }
    const T v0 = h_add(l, r);
    T w;
    if constexpr (sizeof(T) == sizeof(float)) w = x - v0;
    else w = T{x.re - v0.re, x.im - v0.im};
    l = h_add(T{}, h_mul(w, b[0]));
    r = T{};
    for (size_t i = 1; i < n; ++i) {
        const T q = h_mul(s[i - 1], b[i]);
        if (i < split) l = h_add(l, q); else r = h_add(r, q);
    }
    for (size_t i = S; i > 1; --i) s[i - 1] = s[i - 2];
    if (S) s[0] = w;
    return h_add(l, r);
}
// Second-order sections (iirfiltsos.rs:103-117): s[2k], s[2k+1] = v[0], v[1] of section k; b, a = [nsec][3]
template <class T, class C>
T host_iir_sos_step(T *s, size_t nsec, const C *b, const C *a, T x) {
    T u = x;
    for (size_t k = 0; k < nsec; ++k) {
        const T v2 = s[2 * k + 1], v1 = s[2 * k];
        const T p1 = h_mul(v1, a[3 * k + 1]), p2 = h_mul(v2, a[3 * k + 2]);
        T v0;
        if constexpr (sizeof(T) == sizeof(float)) v0 = (u - p1) - p2;
        else v0 = T{(u.re - p1.re) - p2.re, (u.im - p1.im) - p2.im};
        u = h_add(h_add(h_mul(v0, b[3 * k]), h_mul(v1, b[3 * k + 1])), h_mul(v2, b[3 * k + 2]));
        s[2 * k] = v0;
        s[2 * k + 1] = v1;
    }
    return u;
}
template <class T, class C> T host_iir_scale(T y, C scale) { return h_mul(y, scale); }
template float host_iir_tf_step<float, float>(float *, size_t, size_t *, const float *, const float *, float);
template cf32 host_iir_tf_step<cf32, float>(cf32 *, size_t, size_t *, const float *, const float *, cf32);
template cf32 host_iir_tf_step<cf32, cf32>(cf32 *, size_t, size_t *, const cf32 *, const cf32 *, cf32);
template float host_iir_sos_step<float, float>(float *, size_t, const float *, const float *, float);
template cf32 host_iir_sos_step<cf32, float>(cf32 *, size_t, const float *, const float *, cf32);
template cf32 host_iir_sos_step<cf32, cf32>(cf32 *, size_t, const cf32 *, const cf32 *, cf32);
template float host_iir_scale<float, float>(float, float);
template cf32 host_iir_scale<cf32, float>(cf32, float);
template cf32 host_iir_scale<cf32, cf32>(cf32, cf32);

// ---- IIR design helpers, f32 like the reference --------------------------------------------------------------------
namespace {
struct c32 { float re, im; };
inline c32 cadd(c32 a, c32 b) { return c32{a.re + b.re, a.im + b.im}; }
inline c32 cmul(c32 a, c32 b) { return c32{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
inline c32 cneg(c32 a) { return c32{-a.re, -a.im}; }
inline c32 cconj(c32 a) { return c32{a.re, -a.im}; }
inline c32 polar(float r, float th) { return c32{r * std::cos(th), r * std::sin(th)}; }
inline c32 cdiv(c32 a, c32 b) {     // num-complex Div
    const float d = b.re * b.re + b.im * b.im;
    return c32{(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}

// find_conjugate_pairs + cleanup (design/mod.rs:77-193)
int cplxpair(const c32 *z, size_t n, float tol, c32 *p) {
    std::vector<bool> paired(n, false);
    size_t num_pairs = 0, k = 0;
    for (size_t i = 0; i < n; ++i) {
        if (paired[i] || std::fabs(z[i].im) < tol) continue;
        for (size_t j = i + 1; j < n; ++j) {
            if (paired[j] || std::fabs(z[j].im) < tol) continue;
            if (std::fabs(z[i].im + z[j].im) < tol && std::fabs(z[i].re - z[j].re) < tol) {
                p[k] = z[i];
                p[k + 1] = z[j];
                paired[i] = paired[j] = true;
                ++num_pairs;
                k += 2;
                break;
            }
        }
    }
    if (k > n) return fail(YAGI_ERR_RANGE, "invalid derived order");
    for (size_t i = 0; i < n; ++i) {
        if (paired[i]) continue;
        if (std::fabs(z[i].im) < tol) {
            p[k++] = z[i];
            paired[i] = true;
        }
    }
    for (size_t i = 0; i < num_pairs; ++i) {
        p[2 * i] = (p[2 * i + 1].im < 0.0f) ? p[2 * i + 1] : cconj(p[2 * i + 1]);
        p[2 * i + 1] = cconj(p[2 * i]);
    }
    for (size_t i = 0; i < num_pairs; ++i)
        for (size_t j = num_pairs - 1; j > i; --j)
            if (p[2 * (j - 1)].re > p[2 * j].re) {
                std::swap(p[2 * (j - 1)], p[2 * j]);
                std::swap(p[2 * (j - 1) + 1], p[2 * j + 1]);
            }
    for (size_t i = 2 * num_pairs; i < n; ++i)
        for (size_t j = n - 1; j > i; --j)
            if (p[j - 1].re > p[j].re) std::swap(p[j - 1], p[j]);
    return YAGI_OK;
}

// iir_design_d2sos (design/mod.rs:415-502)
int d2sos(const c32 *zd, const c32 *pd, size_t n, c32 k, float *b, float *a) {
    const float tol = 1e-6f;
    std::vector<c32> zp(n), pp(n);
    if (cplxpair(zd, n, tol, zp.data()) != YAGI_OK) return fail(YAGI_ERR_INTERNAL, "could not associate complex pairs (zeros)");
    if (cplxpair(pd, n, tol, pp.data()) != YAGI_OK) return fail(YAGI_ERR_INTERNAL, "could not associate complex pairs (poles)");
    const size_t r = n % 2, L = (n - r) / 2;
    for (size_t i = 0; i < L; ++i) {
        const c32 p0 = cneg(pp[2 * i]), p1 = cneg(pp[2 * i + 1]);
        const c32 z0 = cneg(zp[2 * i]), z1 = cneg(zp[2 * i + 1]);
        a[3 * i] = 1.0f;
        a[3 * i + 1] = cadd(p0, p1).re;
        a[3 * i + 2] = cmul(p0, p1).re;
        b[3 * i] = 1.0f;
        b[3 * i + 1] = cadd(z0, z1).re;
        b[3 * i + 2] = cmul(z0, z1).re;
    }
    if (r == 1) {
        const c32 p0 = cneg(pp[n - 1]), z0 = cneg(zp[n - 1]);
        a[3 * L] = 1.0f; a[3 * L + 1] = p0.re; a[3 * L + 2] = 0.0f;
        b[3 * L] = 1.0f; b[3 * L + 1] = z0.re; b[3 * L + 2] = 0.0f;
    }
    const float kr = k.re;
    const float sgn = kr < 0.0f ? -1.0f : 1.0f;
    const float g = std::pow(kr * sgn, 1.0f / (float)(L + r));
    for (size_t i = 0; i < L + r; ++i) { b[3 * i] *= g; b[3 * i + 1] *= g; b[3 * i + 2] *= g; }
    b[0] *= sgn; b[1] *= sgn; b[2] *= sgn;
    return YAGI_OK;
}
}  // namespace

// new_integrator (iirfilt.rs:204-246) / new_differentiator (:248-288): [Pintelon:1990] digital z/p/k -> 4 sections
int design_iir_pintelon(bool differentiator, float *b, float *a) {
    const float d = 3.14159265358979323846f / 180.0f;
    c32 z[8], p[8], k;
    if (!differentiator) {
        const float zr[8] = {1.175839f * -1.0f, 3.371020f, 3.371020f, 4.549710f, 4.549710f, 5.223966f, 5.223966f, 5.443743f};
        const float zt[8] = {0, -125.1125f, 125.1125f, -80.96404f, 80.96404f, -40.09347f, 40.09347f, 0};
        const float pr[8] = {0.5805235f * -1.0f, 0.2332021f, 0.2332021f, 0.1814755f, 0.1814755f, 0.1641457f, 0.1641457f, 1.0f};
        const float pt[8] = {0, -114.0968f, 114.0968f, -66.33969f, 66.33969f, -21.89539f, 21.89539f, 0};
        for (int i = 0; i < 8; ++i) {
            const bool real = (i == 0 || i == 7);
            const c32 u = polar(1.0f, d * zt[i]), v = polar(1.0f, d * pt[i]);
            z[i] = real ? c32{zr[i], 0.0f} : c32{zr[i] * u.re, zr[i] * u.im};
            p[i] = real ? c32{pr[i], 0.0f} : c32{pr[i] * v.re, pr[i] * v.im};
        }
        k = c32{(float)(-1.89213380759321e-05 / 0.9695401191711425781), 0.0f};
    } else {
        const float zr[8] = {1.702575f * -1.0f, 5.877385f, 5.877385f, 4.197421f, 4.197421f, 5.350284f, 5.350284f, 1.0f};
        const float zt[8] = {0, -221.4063f, 221.4063f, -144.5972f, 144.5972f, -66.88802f, 66.88802f, 0};
        const float pr[8] = {0.8476936f * -1.0f, 0.2990781f, 0.2990781f, 0.2232427f, 0.2232427f, 0.1958670f, 0.1958670f, 0.1886088f};
        const float pt[8] = {0, -125.5188f, 125.5188f, -81.52326f, 81.52326f, -40.51510f, 40.51510f, 0};
        for (int i = 0; i < 8; ++i) {
            const bool real = (i == 0 || i == 7);
            const c32 u = polar(1.0f, d * zt[i]), v = polar(1.0f, d * pt[i]);
            z[i] = real ? c32{zr[i], 0.0f} : c32{zr[i] * u.re, zr[i] * u.im};
            p[i] = real ? c32{pr[i], 0.0f} : c32{pr[i] * v.re, pr[i] * v.im};
        }
        k = c32{(float)(2.09049284907492e-05 / 1.033477783203125000), 0.0f};
    }
    return d2sos(z, p, 8, k, b, a);
}

// iir_design (design/mod.rs:567-717), low-pass band and second-order-section format only: the analog prototype of
// butter.rs:16-48 or cheby2.rs:18-83 (which widens to f64 itself), the prewarp (:207), iir_design_bilinear_a2d
// (:236-271) and iir_design_d2sos.  b, a hold 3 (L + r) coefficients, L = order / 2, r = order % 2.
int design_iir_lowpass_sos(int shape, size_t order, float fc, float ap, float as_, float *b, float *a) {
    if (fc <= 0.0f || fc >= 0.5f) return fail(YAGI_ERR_CONFIG, "cutoff frequency out of range");
    if (ap <= 0.0f) return fail(YAGI_ERR_CONFIG, "pass-band ripple out of range");
    if (as_ <= 0.0f) return fail(YAGI_ERR_CONFIG, "stop-band ripple out of range");
    if (order == 0) return fail(YAGI_ERR_CONFIG, "filter order must be > 0");
    const size_t n = order, r = n % 2, L = (n - r) / 2;
    const c32 one{1.0f, 0.0f};
    auto inv = [](c32 z) {                                   // num-complex inv()
        const float d = z.re * z.re + z.im * z.im;
        return c32{z.re / d, -z.im / d};
    };
    std::vector<c32> pa, za;
    if (shape == YAGI_IIRDES_BUTTER) {
        const float pi = 3.14159265358979323846f;
        for (size_t i = 0; i < L; ++i) {
            const float theta = (2.0f * ((float)i + 1.0f) + (float)n - 1.0f) * pi / (2.0f * (float)n);
            pa.push_back(polar(1.0f, theta));
            pa.push_back(polar(1.0f, -theta));
        }
        if (r) pa.push_back(c32{-1.0f, 0.0f});
    } else if (shape == YAGI_IIRDES_CHEBY2) {
        const double pi = 3.14159265358979323846;
        const float es = std::pow(10.0f, -as_ / 20.0f);
        const double ew = (double)es, t0 = std::sqrt(1.0 + 1.0 / (ew * ew));
        const double tp = std::pow(t0 + 1.0 / ew, 1.0 / (double)n), tm = std::pow(t0 - 1.0 / ew, 1.0 / (double)n);
        const double bb = 0.5 * (tp + tm), aa = 0.5 * (tp - tm);
        for (size_t i = 0; i < L; ++i) {
            const double theta = (double)(2 * (i + 1) + n - 1) * pi / (double)(2 * n);
            pa.push_back(inv(c32{(float)(aa * std::cos(theta)), (float)(-bb * std::sin(theta))}));
            pa.push_back(inv(c32{(float)(aa * std::cos(theta)), (float)(bb * std::sin(theta))}));
        }
        if (r) pa.push_back(inv(c32{(float)-aa, 0.0f}));
        for (size_t i = 0; i < L; ++i) {
            const double theta = 0.5 * pi * (double)(2 * (i + 1) - 1) / (double)n;
            za.push_back(cneg(inv(c32{0.0f, (float)std::cos(theta)})));
            za.push_back(inv(c32{0.0f, (float)std::cos(theta)}));
        }
    } else if (shape == YAGI_IIRDES_CHEBY1 || shape == YAGI_IIRDES_ELLIP || shape == YAGI_IIRDES_BESSEL) {
        return fail(YAGI_ERR_CONFIG, "iir design: the Chebyshev-I, elliptic and Bessel prototypes are not built");
    } else {
        return fail(YAGI_ERR_CONFIG, "iir design: unknown filter shape %d", shape);
    }
    const float m = std::tan(3.14159265358979323846f * fc);
    std::vector<c32> zd(n), pd(n);
    c32 kd = one;                                            // k0 = 1 for both shapes
    auto scl = [](c32 z, float v) { return c32{z.re * v, z.im * v}; };
    auto csub = [](c32 x, c32 y) { return c32{x.re - y.re, x.im - y.im}; };
    for (size_t i = 0; i < n; ++i) {
        zd[i] = (i < za.size()) ? cdiv(cadd(one, scl(za[i], m)), csub(one, scl(za[i], m))) : c32{-1.0f, 0.0f};
        pd[i] = cdiv(cadd(one, scl(pa[i], m)), csub(one, scl(pa[i], m)));
        kd = cmul(kd, cdiv(csub(one, pd[i]), csub(one, zd[i])));
    }
    return d2sos(zd.data(), pd.data(), n, kd, b, a);
}

// iir_design_pll_active_lag (design/pll.rs:16-39)
int design_pll_active_lag(float w, float zeta, float k, float *b, float *a) {
    if (w <= 0.0f) return fail(YAGI_ERR_CONFIG, "bandwidth must be greater than 0");
    if (zeta <= 0.0f) return fail(YAGI_ERR_CONFIG, "damping factor must be greater than 0");
    if (k <= 0.0f) return fail(YAGI_ERR_CONFIG, "gain must be greater than 0");
    const float wn = w, t1 = k / (wn * wn), t2 = 2.0f * zeta / wn - 1.0f / k;
    b[0] = 2.0f * k * (1.0f + t2 / 2.0f);
    b[1] = 2.0f * k * 2.0f;
    b[2] = 2.0f * k * (1.0f - t2 / 2.0f);
    a[0] = 1.0f + t1 / 2.0f;
    a[1] = -t1;
    a[2] = -1.0f + t1 / 2.0f;
    return YAGI_OK;
}

// iir_group_delay (design/mod.rs:771-818)
int iir_group_delay(const float *b, size_t nb, const float *a, size_t na, float fc, float *out) {
    if (nb == 0) return fail(YAGI_ERR_CONFIG, "iir_group_delay(), numerator length must be greater than zero");
    if (na == 0) return fail(YAGI_ERR_CONFIG, "iir_group_delay(), denominator length must be greater than zero");
    if (fc < -0.5f || fc > 0.5f) return fail(YAGI_ERR_CONFIG, "iir_group_delay(), _fc must be in [-0.5,0.5]");
    const size_t nc = na + nb - 1;
    std::vector<float> c(nc, 0.0f);
    for (size_t i = 0; i < na; ++i)
        for (size_t j = 0; j < nb; ++j) c[i + j] += a[na - i - 1] * b[j];
    c32 t0{0.0f, 0.0f}, t1{0.0f, 0.0f};
    for (size_t i = 0; i < nc; ++i) {
        const c32 e = polar(1.0f, 2.0f * 3.14159265358979323846f * fc * (float)i);
        const c32 c0{c[i] * e.re, c[i] * e.im};
        t0 = cadd(t0, c32{c0.re * (float)i, c0.im * (float)i});
        t1 = cadd(t1, c0);
    }
    if (std::hypot(t1.re, t1.im) < 1e-5f) { *out = 0.0f; return YAGI_OK; }
    *out = cdiv(t0, t1).re - (float)(na - 1);
    return YAGI_OK;
}

// ---- Osc (src/nco/osc.rs, nco.rs, vco.rs) ---------------------------------------------------------------------------
// Both lookup tables, built once in the reference's order with libm sinf, and the per-sample operations on the u32
// phase.  Every f32 expression is spelled as the reference writes it, one rounding per operation (the x86-64 host
// target has no FMA, so -ffp-contract cannot fuse anything here).
namespace {
constexpr float kOscPi = 3.14159265358979323846f;      // std::f32::consts::PI
constexpr float kOscTwoPi = 2.0f * kOscPi;             // exact

struct OscTables {
    float nco[1024];                                   // nco.rs:19-28
    float vco_v[1024], vco_s[1024];                    // vco.rs:34-77 (value, skew)
    OscTables() {
        for (int i = 0; i < 1024; ++i) nco[i] = sinf(2.0f * kOscPi * (float)i / 1024.0f);
        auto fp_sin = [](uint32_t th) { return sinf((float)th * kOscPi / 2147483648.0f); };   // vco.rs:79-81
        uint32_t th = 0;
        const uint32_t dth = 0xFFFFFFFFu / 1024u;      // u32::MAX / 1024 = 2^22 - 1
        for (int i = 0; i < 256; ++i) {
            const float value = fp_sin(th);
            const float next = fp_sin(th + dth);
            const float skew = (next - value) / (float)dth;
            vco_v[i] = value;
            vco_s[i] = skew;
            vco_v[i + 512] = -value;
            vco_s[i + 512] = -skew;
            th += dth;
        }
        vco_v[256] = 1.0f;
        vco_s[256] = -vco_s[255];
        vco_v[768] = -vco_v[256];
        vco_s[768] = vco_s[255];
        for (int i = 1; i < 256; ++i) {                // mirror [0, pi/2] onto [pi/2, pi] and [3pi/2, 2pi]
            const int k = i + 256;
            const float value = vco_v[256 - i];
            const float skew = vco_s[256 - i - 1];
            vco_v[k] = value;
            vco_s[k] = -skew;
            vco_v[k + 512] = -value;
            vco_s[k + 512] = skew;
        }
    }
};
const OscTables &osc_tables() {
    static const OscTables t;                          // thread-safe, built once
    return t;
}
}  // namespace

// the device images: NCO float2 {sin[i], sin[(i + 256) & 1023]}; VCO float4 {v[i], s[i], v[i'], s[i']}, i' = (i + 256) & 1023
void osc_device_table(int vco, std::vector<float> &out) {
    const OscTables &t = osc_tables();
    out.clear();
    for (int i = 0; i < 1024; ++i) {
        const int j = (i + 256) & 1023;
        if (!vco) {
            out.push_back(t.nco[i]);
            out.push_back(t.nco[j]);
        } else {
            out.push_back(t.vco_v[i]);
            out.push_back(t.vco_s[i]);
            out.push_back(t.vco_v[j]);
            out.push_back(t.vco_s[j]);
        }
    }
}

// constrain (osc.rs:191-201).  Rust's `as u32` saturates (NaN -> 0); the while loops are kept, so 99.0 or -pi land on
// the reference's word.  Where the reference never returns (an infinity, or a magnitude at which adding 2 pi no
// longer changes the f32) this is a config error.
int osc_constrain(float theta, uint32_t *out) {
    while (theta >= kOscTwoPi) {
        const float t = theta - kOscTwoPi;
        if (t == theta) return fail(YAGI_ERR_CONFIG, "osc: phase/frequency %g cannot be reduced modulo 2 pi in f32", theta);
        theta = t;
    }
    while (theta < 0.0f) {
        const float t = theta + kOscTwoPi;
        if (t == theta) return fail(YAGI_ERR_CONFIG, "osc: phase/frequency %g cannot be reduced modulo 2 pi in f32", theta);
        theta = t;
    }
    const float v = (theta / kOscTwoPi) * 4294967296.0f;   // u32::MAX as f32 == 2^32
    if (!(v > 0.0f)) *out = 0u;                             // NaN, zero, negative zero
    else if (v >= 4294967296.0f) *out = 0xFFFFFFFFu;
    else *out = (uint32_t)v;
    return YAGI_OK;
}

// get_phase / get_frequency (osc.rs:91-103)
float osc_phase(uint32_t theta) { return 2.0f * kOscPi * (float)theta / 4294967296.0f; }
float osc_frequency(uint32_t d_theta) {
    const float d = 2.0f * kOscPi * (float)d_theta / 4294967296.0f;
    return d > kOscPi ? d - 2.0f * kOscPi : d;
}

// sin_cos (nco.rs:41-51, vco.rs:99-112)
void osc_sin_cos(int vco, uint32_t theta, float *s, float *c) {
    const OscTables &t = osc_tables();
    if (!vco) {
        const uint32_t i = ((theta + (1u << 21)) >> 22) & 1023u;
        *s = t.nco[i];
        *c = t.nco[(i + 256) & 1023u];
    } else {
        const uint32_t i = theta >> 22, j = (i + 256) & 1023u;
        const float acc = (float)(theta & 0x3FFFFFu);       // == the low 22 bits of theta + 2^30
        const float ps = acc * t.vco_s[i], pc = acc * t.vco_s[j];
        *s = t.vco_v[i] + ps;
        *c = t.vco_v[j] + pc;
    }
}

// mix_up / mix_down (osc.rs:155-176): x * (cos + i sin), x * conj(cos + i sin), num_complex's Mul
cf32 osc_mix(int vco, uint32_t theta, bool down, cf32 x) {
    float s, c;
    osc_sin_cos(vco, theta, &s, &c);
    if (down) s = -s;
    const float rr = x.re * c, ii = x.im * s, ri = x.re * s, ir = x.im * c;
    return cf32{rr - ii, ri + ir};
}

// ---- FirHilbertFilter (src/filter/fir/firhilb.rs) -------------------------------------------------------------------
// new() :38-64: the Kaiser half-band filter of 4m + 1 taps times Complex32::from_polar(1, pi/2 t).im (libm sinf, f32),
// then every other tap, reversed: hq[j] = h[h_len - i - 1], i = 1, 3, ..
int firhilb_design(size_t m, float as_, std::vector<float> &hq) {
    if (m < 2) return fail(YAGI_ERR_CONFIG, "filter semi-length (m) must be at least 2");
    const size_t h_len = 4 * m + 1;
    std::vector<float> h;
    YG_TRY(design_kaiser(h_len, 0.25f, std::fabs(as_), 0.0f, h));
    for (size_t i = 0; i < h_len; ++i) {
        const float t = (float)i - (float)(h_len - 1) / 2.0f;
        const float im = 1.0f * sinf(0.5f * kOscPi * t);
        h[i] = h[i] * im;
    }
    hq.clear();
    for (size_t i = 1; i < h_len; i += 2) hq.push_back(h[h_len - i - 1]);
    return YAGI_OK;
}
// hq.dotprod(window.read()): products and adds unfused, left to right from the oldest sample, from +0.0
float firhilb_dot(const float *hq, const float *w, size_t L) {
    float s = 0.0f;
    for (size_t k = 0; k < L; ++k) s = s + hq[k] * w[k];
    return s;
}
}  // namespace yagi

extern "C" {

const char *yagi_hip_last_error(void) { return yagi::g_last_error.c_str(); }
const char *yagi_hip_version(void) { return "yagi_hip 0.1.0 (gfx950)"; }

int yagi_hip_fir_design_kaiser(size_t n, float fc, float as_, float mu, float *h) {
    std::vector<float> v;
    YG_TRY(yagi::design_kaiser(n, fc, as_, mu, v));
    if (!h) return yagi::fail(YAGI_ERR_CONFIG, "null output pointer");
    std::memcpy(h, v.data(), n * sizeof(float));
    return YAGI_OK;
}

int yagi_hip_estimate_req_filter_stopband_attenuation(float df, size_t n, float *as_) try {
    if (!as_) return yagi::fail(YAGI_ERR_CONFIG, "null output pointer");
    return yagi::estimate_stopband_attenuation(df, n, as_);
} catch (...) { return ::yagi::api_exception(); }

int yagi_hip_fir_design_prototype(int ftype, size_t k, size_t m, float beta, float dt, float *h) try {
    std::vector<float> v;
    YG_TRY(yagi::design_prototype(ftype, k, m, beta, dt, v));
    if (!h) return yagi::fail(YAGI_ERR_CONFIG, "null output pointer");
    std::memcpy(h, v.data(), v.size() * sizeof(float));
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }

// extension: the 2m taps of FirHilbertFilter::new (firhilb.rs:43-64); no device needed
int yagi_hip_firhilb_design(size_t m, float as_, float *hq) try {
    std::vector<float> v;
    YG_TRY(yagi::firhilb_design(m, as_, v));
    if (!hq) return yagi::fail(YAGI_ERR_CONFIG, "null output pointer");
    std::memcpy(hq, v.data(), v.size() * sizeof(float));
    return YAGI_OK;
} catch (...) { return ::yagi::api_exception(); }
}
