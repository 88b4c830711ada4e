// nvx_companion.h -- what the host sides of the companion libraries (the scan, the resampler, the down-converter bank)
// have in common: the thread's error text, HIP_TRY, the device and span checks, HIP-event timing.  Internal, and all of
// it static: every library compiles its own copy and they share no state.  The main library has nvx_handle.h instead.
#ifndef NVX_COMPANION_H
#define NVX_COMPANION_H

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "navtex_amd.h"

// the calling thread's last error: what the library's own nvx_*_last_error returns
static inline char *nvx_error_text(void)
{
    static thread_local char text[512] = "";
    return text;
}

static inline void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static inline void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(nvx_error_text(), 512, fmt, ap);
    va_end(ap);
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? NVX_ERR_NODEV : NVX_ERR_HIP; \
        }                                                                                  \
    } while (0)

// `noun` names the library in the sentence: "the scan", "the resampler", "the down-converter bank"
static inline int select_device(int device, const char *noun)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        set_error("no HIP device available (%s); %s has no CPU path", e == hipSuccess ? "device count 0" : hipGetErrorString(e), noun);
        return NVX_ERR_NODEV;
    }
    if (device < 0 || device >= n) { set_error("device %d out of range (0..%d)", device, n - 1); return NVX_ERR_ARG; }
    HIP_TRY(hipSetDevice(device));
    return NVX_OK;
}

// [p, p + bytes) of `operand` against the allocation the runtime knows p to lie in; no verdict (NVX_OK) for a pointer it
// does not know
static inline int check_device_span(const void *p, size_t bytes, const char *what, const char *operand)
{
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return NVX_OK; }
    const size_t off = (size_t)((const char *)p - (const char *)base);
    if (off > size || bytes > size - off) {
        set_error("%s: %s: %zu bytes from %p leave the allocation they lie in (%zu bytes from %p): the launch would fault", what, operand, bytes, p, size,
                  (void *)base);
        return NVX_ERR_ARG;
    }
    return NVX_OK;
}

// (a * b + c) * d without wrapping; false on overflow
static inline bool span_bytes(size_t a, size_t b, size_t c, size_t d, size_t *out)
{
    size_t t;
    return !__builtin_mul_overflow(a, b, &t) && !__builtin_add_overflow(t, c, &t) && !__builtin_mul_overflow(t, d, out);
}

// HIP-event time of a library's launches while enabled: a pair of events around each, taken from a pool and returned to it
// once read.  The caller serialises access (the lock of the handle or state the timer belongs to).
struct nvx_event_timer {
    typedef std::pair<hipEvent_t, hipEvent_t> events;
    bool enabled = false;
    std::vector<events> pool, pending;
    double sum_ms = 0.0; uint64_t count = 0;

    // in front of the launch, on its stream; ev stays null while timing is off
    int begin(hipStream_t s, events &ev)
    {
        ev = events{ nullptr, nullptr };
        if (!enabled) return NVX_OK;
        if (pool.empty()) { HIP_TRY(hipEventCreate(&ev.first)); HIP_TRY(hipEventCreate(&ev.second)); }
        else { ev = pool.back(); pool.pop_back(); }
        HIP_TRY(hipEventRecord(ev.first, s));
        return NVX_OK;
    }
    int end(hipStream_t s, const events &ev)
    {
        if (!ev.first) return NVX_OK;
        HIP_TRY(hipEventRecord(ev.second, s));
        pending.push_back(ev);
        return NVX_OK;
    }
    // waits for the launches still in flight
    int collect(double *sum, uint64_t *n, int reset)
    {
        for (auto &p : pending) {
            HIP_TRY(hipEventSynchronize(p.second));
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
            sum_ms += ms; count++;
            pool.push_back(p);
        }
        pending.clear();
        if (sum) *sum = sum_ms;
        if (n) *n = count;
        if (reset) { sum_ms = 0.0; count = 0; }
        return NVX_OK;
    }
    void destroy()
    {
        for (auto &p : pending) pool.push_back(p);
        for (auto &p : pool) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
        pool.clear(); pending.clear();
    }
};

#endif
