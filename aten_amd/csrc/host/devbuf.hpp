// Owned GPU handles of the host side: device buffers, events and streams.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

namespace atn {

#define ATN_HIP(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) { return fail(ATN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { swap(o); return *this; }
    ~DevBuf() { release(); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; n = 0; } }
    hipError_t resize(size_t count)
    {
        if (count <= n && p) return hipSuccess;
        release();
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T) + 256);     // slack: the walk's pair fetch reads 32 B past a record
        if (e == hipSuccess) n = count;
        return e;
    }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); }
    hipError_t upload(const std::vector<T>& v, hipStream_t s)
    {
        hipError_t e = resize(v.size() ? v.size() : 1);
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
    }
};

// An event or a stream that its holder owns.  It is created in place through `&x.h`, where and how the holder decides (HIP hands out
// hardware queues in creation order: context.hpp), and destroyed with the holder.  Move-only; reads as the raw handle.
template <class H, hipError_t (*Destroy)(H)>
struct DevHandle {
    H h = nullptr;
    DevHandle() = default;
    DevHandle(DevHandle&& o) noexcept : h(o.h) { o.h = nullptr; }
    DevHandle& operator=(DevHandle&& o) noexcept { swap(o); return *this; }
    ~DevHandle() { if (h) (void)Destroy(h); }
    void swap(DevHandle& o) { std::swap(h, o.h); }
    operator H() const { return h; }
};
using DevEvent = DevHandle<hipEvent_t, hipEventDestroy>;
using DevStream = DevHandle<hipStream_t, hipStreamDestroy>;

} // namespace atn
