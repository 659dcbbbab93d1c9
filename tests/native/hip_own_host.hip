// The owning buffer types of gf_hip_own.hpp on their own (tests/test_hip_own_host.py).  `hip_own_host nodevice` on a machine without a GPU: every way of getting
// memory fails and leaves the object empty, and moving or destroying failed and empty objects does nothing.  `hip_own_host device`: the two ways of getting memory
// (alloc: exact and zeroed, fit: grow-only), moves, and alloc(0).  Prints "<check>: ok" per check; the exit status is the number of failed checks.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../ground-fusion_amd/csrc/gf_hip_own.hpp"

namespace gf {
int set_err(int code, const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); return code; }
}

static int failed = 0;
static void check(bool ok, const char* what) { printf("%s: %s\n", what, ok ? "ok" : "FAILED"); if (!ok) failed++; }

template <class B> static bool empty(const B& b) { return b.p == nullptr && b.n == 0; }

static void without_device() {
    gf::DevBuf<int> d; gf::PinBuf<int> p;
    for (int pass = 0; pass < 2; pass++) {   // a second call behaves as the first
        check(d.alloc(1000) != hipSuccess && empty(d), "device alloc fails and leaves the buffer empty");
        check(d.fit(1000) != hipSuccess && empty(d), "device fit fails and leaves the buffer empty");
        check(p.alloc(1000) != hipSuccess && empty(p) && p.hd == nullptr, "pinned alloc fails and leaves the buffer empty");
        check(p.fit(1000) != hipSuccess && empty(p) && p.hd == nullptr, "pinned fit fails and leaves the buffer empty");
    }
    gf::DevBuf<int> d2(std::move(d)); gf::PinBuf<int> p2(std::move(p));
    check(empty(d) && empty(d2) && empty(p) && empty(p2), "move construction of failed objects");
    gf::DevBuf<int> d3; gf::PinBuf<int> p3;
    d3 = std::move(d2); p3 = std::move(p2);
    check(empty(d2) && empty(d3) && empty(p2) && empty(p3), "move assignment of empty objects");
    { gf::DevBuf<double> a; gf::PinBuf<double> b; gf::Stream s; gf::Event e; check(s.s == nullptr && e.e == nullptr && hipStream_t(s) == nullptr && hipEvent_t(e) == nullptr, "empty stream and event"); }
    check(true, "destructors of empty objects");
    check(gf::require_device() == GF_ERR_NO_DEVICE, "require_device refuses");
}

static void with_device() {
    check(gf::require_device() == GF_OK, "require_device");
    {
        gf::DevBuf<int> d;
        check(d.alloc(1000) == hipSuccess && d.p && d.n == 1000, "device alloc(1000)");
        std::vector<int> back(1000, -1);
        check(hipMemcpy(back.data(), d.p, 4000, hipMemcpyDeviceToHost) == hipSuccess && back == std::vector<int>(1000, 0), "device alloc reads back as zeros");
        int* const was = d.p;
        gf::DevBuf<int> e(std::move(d));
        check(empty(d) && e.p == was && e.n == 1000, "device move construction: source empty, target holds the pointer");
        gf::DevBuf<int> f;
        f = std::move(e);
        check(empty(e) && f.p == was && f.n == 1000, "device move assignment: source empty, target holds the pointer");
    }
    {
        gf::PinBuf<int> p;
        check(p.alloc(1000) == hipSuccess && p.p && p.n == 1000, "pinned alloc(1000)");
        check(p.hd != nullptr, "pinned alloc maps the memory into the device's address space");
        bool zero = true;
        for (int i = 0; i < 1000; i++) zero = zero && p.p[i] == 0;
        check(zero, "pinned alloc is zeros");
        int* const was = p.p; int* const was_hd = p.hd;
        gf::PinBuf<int> q(std::move(p));
        check(empty(p) && p.hd == nullptr && q.p == was && q.hd == was_hd && q.n == 1000, "pinned move construction: source empty, target holds the pointer");
    }
    {
        gf::DevBuf<int> d; gf::PinBuf<int> p;
        check(d.fit(10) == hipSuccess && d.p && d.n == 10 && p.fit(10) == hipSuccess && p.p && p.n == 10, "fit(10)");
        check(d.fit(1000) == hipSuccess && d.p && d.n == 1000 && p.fit(1000) == hipSuccess && p.p && p.n == 1000, "fit(1000) grows");
        int* const dw = d.p; int* const pw = p.p;
        check(hipMemset(d.p, 0, 4000) == hipSuccess && hipDeviceSynchronize() == hipSuccess, "the grown buffer holds 1000 elements");
        for (int i = 0; i < 1000; i++) p.p[i] = i;
        check(d.fit(100) == hipSuccess && d.p == dw && d.n == 1000 && p.fit(100) == hipSuccess && p.p == pw && p.n == 1000, "fit(100) afterwards keeps pointer and capacity");
        check(d.fit(1000) == hipSuccess && d.p == dw && p.fit(1000) == hipSuccess && p.p == pw, "fit(1000) again does not allocate");
    }
    {
        gf::DevBuf<int> d; gf::PinBuf<int> p;
        check(d.alloc(0) == hipSuccess && d.n == 0 && p.alloc(0) == hipSuccess && p.n == 0, "alloc(0) succeeds");
        check(d.fit(0) == hipSuccess && p.fit(0) == hipSuccess, "fit(0) succeeds");
    }
    {
        gf::Stream s; gf::Event e;
        check(hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking) == hipSuccess && hipEventCreate(&e.e) == hipSuccess, "stream and event");
        check(hipEventRecord(e, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess, "stream and event convert to the raw handles");
    }
    check(hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess, "no error left behind");
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "nodevice")) without_device();
    else if (argc == 2 && !strcmp(argv[1], "device")) with_device();
    else { fprintf(stderr, "usage: hip_own_host nodevice | device\n"); return 99; }
    return failed;
}
