// gf_hip_own.hpp — who owns device memory, page-locked memory, streams and events, and the one way a failed HIP call becomes an error code.
// Every handle of the library (gf_ba, gf_tracker, gf_featsweep, PreintBatch, gf_comm) holds its resources as members of these types: a handle is released by
// deleting it, members go in reverse order of their declaration, and an error path that returns early frees what was built so far.
// The types only own.  WHEN memory is obtained stays with the create functions, as explicit statements in a deliberate order: an allocation's place in the
// process's sequence decides which recycled memory it gets ("Handles and ownership").
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>

#include "../../include/groundfusion_hip.h"

namespace gf {
int set_err(int code, const char* fmt, ...);   // gf_tracker.hip
}

#define HIPCHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return gf::set_err((e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? GF_ERR_NO_DEVICE : GF_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

namespace gf {

inline int require_device() {
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { (void)hipGetLastError(); return set_err(GF_ERR_NO_DEVICE, "no HIP device available (%s); the HIP path has no CPU fallback", hipGetErrorString(e)); }
    return GF_OK;
}

inline void pinned_free(void* p) { if (p) (void)hipHostFree(p); }

// Device memory.  Two ways to get it, for the two policies of the library:
//   alloc(count)  exactly `count` elements (at least one is allocated), zero-filled, the fill finished on the null stream before the call returns: hipMalloc hands
//                 back whatever the previous owner left, and the handles' streams are non-blocking -- nothing of theirs may meet the fill
//   fit(count)    capacity of at least `count` elements, grown when it is too small (the content is lost), never filled: staging that every use overwrites
// A failed call leaves the buffer empty.  n: the elements asked for (alloc) or the capacity (fit).
template <class T> struct DevBuf {
    T* p = nullptr; size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
    ~DevBuf() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t count) {
        reset();
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        hipError_t e = hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) { p = nullptr; return e; }
        e = hipMemset(p, 0, bytes);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) { reset(); return e; }
        n = count;
        return hipSuccess;
    }
    hipError_t fit(size_t count) {
        if (count <= n) return hipSuccess;
        reset();
        const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        n = count;
        return hipSuccess;
    }
};

// Page-locked host memory, with the same two ways.  hd: the same memory as kernels address it (page-locked memory is mapped into the device's address space), or null.
template <class T> struct PinBuf {
    T* p = nullptr; size_t n = 0; T* hd = nullptr;
    PinBuf() = default;
    PinBuf(PinBuf&& o) noexcept : p(o.p), n(o.n), hd(o.hd) { o.p = o.hd = nullptr; o.n = 0; }
    PinBuf& operator=(PinBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; n = o.n; hd = o.hd; o.p = o.hd = nullptr; o.n = 0; } return *this; }
    ~PinBuf() { reset(); }
    void reset() { pinned_free(p); p = hd = nullptr; n = 0; }
    hipError_t alloc(size_t count) {   // page-locked memory is recycled inside the process like device memory: zeros, explicitly
        reset();
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        if (const hipError_t e = get(bytes)) return e;
        memset(p, 0, bytes);
        n = count;
        return hipSuccess;
    }
    hipError_t fit(size_t count) {
        if (count <= n) return hipSuccess;
        reset();
        if (const hipError_t e = get(count * sizeof(T))) return e;
        n = count;
        return hipSuccess;
    }
  private:
    hipError_t get(size_t bytes) {
        const hipError_t e = hipHostMalloc((void**)&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return e; }
        void* q = nullptr;
        hd = hipHostGetDevicePointer(&q, p, 0) == hipSuccess ? static_cast<T*>(q) : nullptr;
        (void)hipGetLastError();
        return hipSuccess;
    }
};

// A stream / an event that is destroyed with its owner.  Created by the owner with the hipStreamCreate* / hipEventCreate* call it wants, on the raw handle;
// converts to the raw handle, so launches and records read as with one.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};

}  // namespace gf
