// owned.h — what the HIP runtime hands out, owned by type: device memory, page-locked host memory, streams and events live in
// std::unique_ptr with a stateless deleter, so whatever holds one frees it when it goes and nothing keeps a list of frees.
// Host code only.
//
// A deleter ignores the runtime's verdict.  The paths that report a failed free (the grow-only buffer below, a re-upload of the
// weights, a rebuild of the slot streams) release() the handle and call the HIP function themselves.
// The creation helpers return the runtime's error and assign only on success: an owner is either empty or holds a live handle.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

namespace davo {

struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
struct PinnedFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };

template <class T> using DevMem = std::unique_ptr<T, DevFree>;            // hipMalloc
template <class T> using PinnedMem = std::unique_ptr<T, PinnedFree>;      // hipHostMalloc
using StreamOwner = std::unique_ptr<ihipStream_t, StreamDestroy>;         // hipStream_t is ihipStream_t*
using EventOwner = std::unique_ptr<ihipEvent_t, EventDestroy>;            // hipEvent_t is ihipEvent_t*

template <class T> inline constexpr size_t elem_bytes = sizeof(T);
template <> inline constexpr size_t elem_bytes<void> = 1;                 // DevMem<void>: n counts bytes

// n elements of device memory
template <class T> hipError_t dev_alloc(DevMem<T>* out, size_t n) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, n * elem_bytes<T>);
    if (e == hipSuccess) out->reset(static_cast<T*>(p));
    return e;
}

// free what *m holds, then n elements anew (contents are not kept).  A failed free is reported; *m is then empty.
template <class T> hipError_t dev_realloc(DevMem<T>* m, size_t n) {
    if (*m) {
        const hipError_t e = hipFree(m->release());
        if (e != hipSuccess) return e;
    }
    return dev_alloc(m, n);
}

// n elements of page-locked host memory (flags: hipHostMallocDefault, hipHostMallocMapped | ...)
template <class T> hipError_t pinned_alloc(PinnedMem<T>* out, size_t n, unsigned flags) {
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, n * elem_bytes<T>, flags);
    if (e == hipSuccess) out->reset(static_cast<T*>(p));
    return e;
}

// a non-blocking stream; with a mask (`words' 32-bit words) one confined to those compute units
inline hipError_t stream_create(StreamOwner* out, unsigned words = 0, const uint32_t* cu_mask = nullptr) {
    hipStream_t s = nullptr;
    const hipError_t e = cu_mask ? hipExtStreamCreateWithCUMask(&s, words, cu_mask) : hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) out->reset(s);
    return e;
}

inline hipError_t event_create(EventOwner* out, unsigned flags = hipEventDefault) {
    hipEvent_t ev = nullptr;
    const hipError_t e = hipEventCreateWithFlags(&ev, flags);
    if (e == hipSuccess) out->reset(ev);
    return e;
}

// A device buffer that only grows: reserve(bytes) leaves at least that much behind get(), freeing the smaller block first (nothing
// may still read it) and not keeping its contents.  It stays where it is: the deleted copy operations - the only special members
// this header spells out - take the moves with them.
class GrowBuf {
public:
    GrowBuf() = default;
    GrowBuf(const GrowBuf&) = delete;
    GrowBuf& operator=(const GrowBuf&) = delete;
    void* get() const { return mem_.get(); }
    size_t bytes() const { return cap_; }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap_) return hipSuccess;
        cap_ = 0;
        const hipError_t e = dev_realloc(&mem_, bytes);
        if (e == hipSuccess) cap_ = bytes;
        return e;
    }

private:
    DevMem<void> mem_;
    size_t cap_ = 0;
};

// a host table on the device; empty if it could not be put there (hipGetLastError() says why)
template <class T> DevMem<T> upload_table(const std::vector<T>& host) {
    DevMem<T> d;
    if (dev_alloc(&d, host.size()) != hipSuccess ||
        hipMemcpy(d.get(), host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
        d.reset();
    return d;
}

}  // namespace davo
