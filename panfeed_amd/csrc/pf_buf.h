// pf_buf.h -- internal: the error helpers and the owners of what the library's three translation units with device code
// (pf_api.hip, pf_rowfilter.hip, pf_deflate.hip) take from the HIP runtime: device memory (DevBuf), pinned host memory
// (PinBuf), ordinary host memory page-locked where it lies (RegBuf), events (HipEvent), streams (HipStream; TimedStream with
// the two events that time it).  Not part of the C ABI (include/panfeed_hip.h).  A buffer frees itself when its owner goes,
// an event is destroyed and a stream synchronised, then destroyed, with theirs -- nowhere else is one of them created,
// registered or let go; what is freed early on purpose says so where it happens.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/panfeed_hip.h"

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>

extern "C" void pf_set_error_(const char* msg);   // pf_api.hip: the text pf_last_error returns on this thread

// test hook (pf_debug_limit_alloc): single device allocations above the limit are refused as if the device were out of
// memory; the largest request and the exact-size retries that succeeded are counted (one set per process)
inline std::atomic<uint64_t> g_alloc_limit{0}, g_alloc_max_request{0}, g_alloc_exact_retries{0};

namespace {

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    pf_set_error_(buf);
    return code;
}

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(e_ == hipErrorOutOfMemory ? PF_ERR_OOM : PF_ERR_HIP, "%s failed: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                             \
    } while (0)
#define PFCHK(expr)             \
    do {                        \
        int r_ = (expr);        \
        if (r_ != PF_OK) return r_; \
    } while (0)

hipError_t dev_malloc(void** p, size_t bytes) {
    const uint64_t lim = g_alloc_limit.load(std::memory_order_relaxed);
    if (lim && bytes > lim) { *p = nullptr; return hipErrorOutOfMemory; }
    return hipMalloc(p, bytes);
}

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool view = false;     // points into another DevBuf (staged uploads): never freed, never grown
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept
        : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)), view(std::exchange(o.view, false)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); view = std::exchange(o.view, false);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    int ensure(size_t bytes, bool exact = false) {
        if (view) { p = nullptr; cap = 0; view = false; }
        if (bytes <= cap) return PF_OK;
        const bool regrow = p != nullptr;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        uint64_t seen = g_alloc_max_request.load(std::memory_order_relaxed);
        while (bytes > seen && !g_alloc_max_request.compare_exchange_weak(seen, bytes)) {}
        // (a buffer that has to be re-made gets a quarter of slack: hipFree + hipMalloc of a multi-gigabyte buffer was seen to
        // take 0.25 s in the middle of a submit when a batch's key-partition queues came out a little larger than the batch
        // before's; a first allocation -- the scratch slices are 123 GB in bench.py -- gets a sixteenth).  The slack is a
        // convenience, never a requirement: when it does not fit, the exact size is asked for before giving up.
        // (exact: a buffer whose size a caller's memory budget bounds gets none)
        size_t want = exact ? bytes : bytes + (regrow ? bytes / 4 : bytes / 16) + 256;
        hipError_t e = dev_malloc(&p, want);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            want = bytes;
            e = dev_malloc(&p, want);
            if (e == hipSuccess) g_alloc_exact_retries.fetch_add(1, std::memory_order_relaxed);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return fail(PF_ERR_OOM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        }
        cap = want;
        return PF_OK;
    }
    void release() { if (p && !view) (void)hipFree(p); p = nullptr; cap = 0; view = false; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Pinned (page-locked) host memory: the source or destination of an asynchronous copy.  A block that is too small is
// re-made with a quarter of slack, or at exactly `bytes` for a caller that sizes it itself.
struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    PinBuf& operator=(PinBuf&& o) noexcept {
        if (this != &o) { release(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); }
        return *this;
    }
    ~PinBuf() { release(); }
    int ensure(size_t bytes, bool exact = false) {
        if (bytes <= cap) return PF_OK;
        release();
        const size_t want = exact ? bytes : bytes + bytes / 4;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return fail(PF_ERR_OOM, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e)); }
        cap = want;
        return PF_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Ordinary host memory, 4096-aligned and page-locked where it lies (hipHostRegister) -- or a view into another RegBuf's
// block, which is never freed.  A block that is too small is re-made at exactly `bytes`; a failure leaves nothing behind,
// and no sticky HIP error either.
struct RegBuf {
    char* p = nullptr; size_t cap = 0; bool view = false;
    RegBuf() = default; RegBuf(const RegBuf&) = delete; RegBuf& operator=(const RegBuf&) = delete;
    RegBuf(RegBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)), view(std::exchange(o.view, false)) {}
    RegBuf& operator=(RegBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(view, o.view); return *this; }
    ~RegBuf() { release(); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return PF_OK;
        release();
        void* q = nullptr;
        if (posix_memalign(&q, 4096, bytes) != 0 || !q) return fail(PF_ERR_OOM, "posix_memalign(%zu) failed", bytes);
        if (hipHostRegister(q, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); free(q); return fail(PF_ERR_OOM, "hipHostRegister(%zu) failed", bytes); }
        p = static_cast<char*>(q); cap = bytes;
        return PF_OK;
    }
    void release() { if (p && !view) { (void)hipHostUnregister(p); free(p); } p = nullptr; cap = 0; view = false; }
};

// An event: made on first use with the flags its site asks for, destroyed with its owner; passed to HIP as it is.
struct HipEvent {
    hipEvent_t e = nullptr;
    HipEvent() = default; HipEvent(const HipEvent&) = delete; HipEvent& operator=(const HipEvent&) = delete;
    HipEvent(HipEvent&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
    HipEvent& operator=(HipEvent&& o) noexcept { std::swap(e, o.e); return *this; }
    ~HipEvent() { if (e) (void)hipEventDestroy(e); }
    int ensure(unsigned flags = hipEventDefault) {
        if (e || (flags == hipEventDefault ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, flags)) == hipSuccess) return PF_OK;
        e = nullptr;
        return fail(PF_ERR_HIP, "hipEventCreate failed");
    }
    operator hipEvent_t() const { return e; }
};

// A stream: synchronised, then destroyed, with its owner; passed to HIP as it is.
struct HipStream {
    hipStream_t s = nullptr;
    HipStream() = default; HipStream(const HipStream&) = delete; HipStream& operator=(const HipStream&) = delete;
    HipStream(HipStream&& o) noexcept : s(std::exchange(o.s, nullptr)) {}
    HipStream& operator=(HipStream&& o) noexcept { std::swap(s, o.s); return *this; }
    ~HipStream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    int create() {
        const hipError_t r = hipStreamCreate(&s);
        if (r != hipSuccess) { s = nullptr; return fail(PF_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(r)); }
        return PF_OK;
    }
    operator hipStream_t() const { return s; }
};

// A stream and the two events that bracket what is timed on it.  Its owner declares it last, so that it goes first: the
// stream is synchronised and destroyed before the buffers its work may still use are freed.
struct TimedStream {
    HipEvent e0, e1;
    HipStream stream;                                 // (its own last member likewise: it goes before the events recorded on it)
    int create() { PFCHK(stream.create()); PFCHK(e0.ensure()); PFCHK(e1.ensure()); return PF_OK; }
    template <class F> int timed(F&& work) {          // e0 and e1 recorded around what `work` puts on the stream
        HIPCHK(hipEventRecord(e0, stream)); PFCHK(work()); HIPCHK(hipEventRecord(e1, stream));
        return PF_OK;
    }
    // once the caller has synchronised with the stream: the time between the two events, added to *ms
    void add_elapsed(float* ms) const { float t = 0; if (hipEventElapsedTime(&t, e0, e1) == hipSuccess) *ms += t; }
};

}  // namespace
