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

}  // namespace yagi

#pragma GCC visibility pop
