// objstate.hpp -- host-side building blocks shared by the stateful objects of capi.hip (the only file that includes
// this): synchronous copies, table upload, ping-pong device state, the staging of host-pointer block calls and the bookkeeping of a host mirror.
#pragma once

#include <algorithm>

#include "common.hpp"

// nothing here is part of the library's interface
#pragma GCC visibility push(hidden)

namespace yagi {

inline int upload(void *dst, const void *src, size_t bytes, hipStream_t st) {
    if (bytes == 0) return YAGI_OK;
    YG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
    YG_HIP(hipStreamSynchronize(st));
    return YAGI_OK;
}
inline int download(void *dst, const void *src, size_t bytes, hipStream_t st) {
    if (bytes == 0) return YAGI_OK;
    YG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    YG_HIP(hipStreamSynchronize(st));
    return YAGI_OK;
}

// a table: exactly `bytes` on the device, filled from the host
inline int fill(DevBuf &b, const void *src, size_t bytes, hipStream_t st) {
    YG_TRY(b.alloc(bytes));
    return upload(b.p, src, bytes, st);
}

// Device state that a kernel rewrites as a whole: it reads cur() and writes next(), the host then flip()s.
template <int N = 2>
struct PingPong {
    DevBuf buf[N];
    int at = 0;
    int alloc(size_t bytes) {
        for (auto &b : buf) YG_TRY(b.alloc(bytes));
        return YAGI_OK;
    }
    template <class T = void> T *cur() const { return static_cast<T *>(buf[at].p); }
    template <class T = void> T *next() const { return static_cast<T *>(buf[(at + 1) % N].p); }
    void flip() { at = (at + 1) % N; }
};

// Host-pointer block calls: two grow-only device buffers per object; run() uploads nx elements of x, hands both device
// pointers to the object's device form and downloads ny elements of y.  Every copy is synchronous.
struct Staging {
    DevBuf x, y;
    template <class T>
    int put(hipStream_t st, const T *xh, size_t nx) {      // input only
        YG_TRY(x.ensure(nx * sizeof(T)));
        return upload(x.p, xh, nx * sizeof(T), st);
    }
    // y_room: elements to reserve for y where that is more than ny
    template <class T, class F>
    int run(hipStream_t st, const T *xh, size_t nx, T *yh, size_t ny, F &&block_dev, size_t y_room = 0) {
        YG_TRY(x.ensure(nx * sizeof(T)));
        YG_TRY(y.ensure(std::max(ny, y_room) * sizeof(T)));
        YG_TRY(upload(x.p, xh, nx * sizeof(T), st));
        YG_TRY(block_dev(x.as<T>(), y.as<T>()));
        return download(yh, y.p, ny * sizeof(T), st);
    }
};

// Which of an object's two copies of its state (host mirror, device buffer) is current.  Whoever writes one side says
// so, which makes the other stale; need_host() / need_dev() run the copy only then.
class Mirror {
    bool host_valid = true, dev_valid = true;

public:
    void host_written() { dev_valid = false; }                    // the host copy was current (need_host) and changed
    void dev_written() { host_valid = false; }                    // the device copy was current (need_dev) and changed
    void in_sync() { host_valid = dev_valid = true; }             // after both sides were reset
    bool dev_current() const { return dev_valid; }
    template <class F>
    int need_host(F &&download_fn) {
        if (host_valid) return YAGI_OK;
        YG_TRY(download_fn());
        host_valid = true;
        return YAGI_OK;
    }
    template <class F>
    int need_dev(F &&upload_fn) {
        if (dev_valid) return YAGI_OK;
        YG_TRY(upload_fn());
        dev_valid = true;
        return YAGI_OK;
    }
};

// rows x C elements, compact on the device, to the caller's rows of pitch y_pitch
template <class T>
int download_rows(hipStream_t st, const DevBuf &src, size_t rows, size_t C, T *y, size_t y_pitch) {
    std::vector<T> t(rows * C);
    YG_TRY(download(t.data(), src.p, rows * C * sizeof(T), st));
    for (size_t j = 0; j < rows; ++j) std::copy(t.begin() + j * C, t.begin() + (j + 1) * C, y + j * y_pitch);
    return YAGI_OK;
}

// What the objects that hold a bank of independent channels share.  Such an object D is two halves: a plain copyable
// host struct D::Host (configuration, the host mirror of the per-channel state, everything that needs no device: C,
// reset_chan(c)), from which it derives, and this device half.  D supplies kFamily (the name its messages start with),
// alloc() and each_array(f), its one list of mirrored arrays: f(DevBuf &, void *host, size_t bytes) for each.
template <class D>
struct BankObj {
    hipStream_t st = nullptr;
    Mirror mirror;
    Staging ws;                                           // host block forms: x as given, y compact [rows][C]

    D &self() { return *static_cast<D *>(this); }
    int ensure_host() {
        return mirror.need_host(
            [&] { return self().each_array([&](DevBuf &d, void *h, size_t b) { return download(h, d.p, b, st); }); });
    }
    int ensure_dev() {
        return mirror.need_dev(
            [&] { return self().each_array([&](DevBuf &d, void *h, size_t b) { return upload(d.p, h, b, st); }); });
    }
    template <class F>
    int edit(F &&f) {                                       // f() changes the host mirror
        YG_TRY(ensure_host());
        f();
        mirror.host_written();
        return YAGI_OK;
    }
    int reset() {
        return edit([&] {
            for (size_t c = 0; c < self().C; ++c) self().reset_chan(c);
        });
    }
    int reset_channel(size_t c) {
        if (c >= self().C) return fail(YAGI_ERR_CONFIG, "%s: channel %zu of %zu", D::kFamily, c, self().C);
        return edit([&] { self().reset_chan(c); });
    }
    // The tail of a host call whose channels write different numbers of rows: `status` holds ny[C], stalled[C] (and
    // more, `words` in all); row j of ws.y, and of the byte plane symsrc where sym is given, goes out for j < ny[c].
    int fetch_ragged(const DevBuf &status, size_t words, uint32_t *ny, uint32_t *stalled, cf32 *y, size_t y_pitch,
                     const DevBuf *symsrc = nullptr, uint8_t *sym = nullptr, size_t sym_pitch = 0) {
        const size_t C = self().C;
        std::vector<unsigned> s(words);
        YG_TRY(download(s.data(), status.p, words * sizeof(unsigned), st));
        size_t rows = 0;
        for (size_t c = 0; c < C; ++c) {
            ny[c] = s[c];
            stalled[c] = s[C + c];
            rows = std::max(rows, (size_t)s[c]);
        }
        std::vector<cf32> t(rows * C);
        YG_TRY(download(t.data(), ws.y.p, rows * C * sizeof(cf32), st));
        std::vector<uint8_t> tb(sym ? rows * C : 0);
        if (sym) YG_TRY(download(tb.data(), symsrc->p, rows * C, st));
        for (size_t j = 0; j < rows; ++j)
            for (size_t c = 0; c < C; ++c)
                if (j < ny[c]) {
                    y[j * y_pitch + c] = t[j * C + c];
                    if (sym) sym[j * sym_pitch + c] = tb[j * C + c];
                }
        return YAGI_OK;
    }
};

// The bodies of the entry points every bank object has.  S is the handle's struct: it has st, configure(args...),
// alloc(), ensure_host() and names its host struct S::Host.
template <class S, class... A>
int bank_create(S **q, A... args) {
    if (!q) return fail(YAGI_ERR_CONFIG, "null pointer argument");
    *q = nullptr;
    auto o = std::make_unique<S>();
    YG_TRY(o->configure(args...));
    YG_TRY(o->alloc());
    *q = o.release();
    return YAGI_OK;
}
template <class S>
int bank_destroy(S *q) {
    if (q) (void)hipStreamSynchronize(q->st);
    delete q;
    return YAGI_OK;
}
// on the source's stream: the host struct whole, then fresh device buffers and staging
template <class S>
int bank_clone(S *q, S **out) {
    if (!q) return fail(YAGI_ERR_CONFIG, "null handle");
    if (!out) return fail(YAGI_ERR_CONFIG, "null pointer argument");
    *out = nullptr;
    YG_TRY(q->ensure_host());
    auto o = std::make_unique<S>();
    static_cast<typename S::Host &>(*o) = static_cast<const typename S::Host &>(*q);
    o->st = q->st;
    YG_TRY(o->alloc());
    *out = o.release();
    return YAGI_OK;
}
template <class S>
int bank_set_stream(S *q, yagi_stream_t s) {
    if (!q) return fail(YAGI_ERR_CONFIG, "null handle");
    if (q->st == to_stream(s)) return YAGI_OK;
    YG_HIP(hipStreamSynchronize(q->st));
    q->st = to_stream(s);
    return YAGI_OK;
}
// *out = f(object): a setting
template <class S, class T, class F>
int bank_get(S *q, T *out, F &&f) {
    if (!q) return fail(YAGI_ERR_CONFIG, "null handle");
    if (!out) return fail(YAGI_ERR_CONFIG, "null pointer argument");
    *out = f(*q);
    return YAGI_OK;
}
// out[c] = f(object, c) for every channel, on the host mirror
template <class S, class T, class F>
int bank_get_each(S *q, T *out, F &&f) {
    if (!q) return fail(YAGI_ERR_CONFIG, "null handle");
    if (!out) return fail(YAGI_ERR_CONFIG, "null pointer argument");
    YG_TRY(q->ensure_host());
    for (size_t c = 0; c < q->C; ++c) out[c] = f(*q, c);
    return YAGI_OK;
}

}  // namespace yagi

#pragma GCC visibility pop
