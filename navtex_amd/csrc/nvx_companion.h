// nvx_companion.h -- what the host sides of the companion libraries have in common.  For all of them: the thread's error
// text, HIP_TRY, the device and span checks, HIP-event timing.  For those that carry rows of streams from call to call (the
// blanker, the IQ corrector, the real-input converter, the noise canceller, the tone notch, the row aligner, the multi-tap noise canceller, the diversity combiner, and the rate changers: the resampler,
// the down-converter bank, the narrowband interpolator, the channel tap, the zoom bank), below those: the position and row checks, the state rows
// read and written alternately, a push's staging buffers.  Internal, and all of it static: every library compiles its own
// copy and they share no state.  The main library has nvx_handle.h instead.
#ifndef NVX_COMPANION_H
#define NVX_COMPANION_H

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>
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

// the bodies of a library's *_timing and *_time_stats; mu is the lock of what the timer belongs to
static inline int timing_enable(std::mutex &mu, nvx_event_timer &t, int enable)
{
    std::lock_guard<std::mutex> lk(mu);
    t.enabled = enable != 0;
    return NVX_OK;
}

static inline int timing_collect(std::mutex &mu, nvx_event_timer &t, double *sum_ms, uint64_t *n, int reset)
{
    std::lock_guard<std::mutex> lk(mu);
    return t.collect(sum_ms, n, reset);
}

// ----------------------------------------------------------------------------------------------------- rows at positions
static inline bool position_ok(const char *what, uint64_t position)
{
    if (position >> 62) set_error("%s: the position passes 2^62", what);
    return !(position >> 62);
}

// row i of n, or -1 (all of them) where `lowest` says so; `noun` is what the library calls a row: "stream", "pair", "input"
static inline bool row_ok(const char *what, const char *noun, int i, int lowest, int n)
{
    if (i < lowest || i >= n) set_error("%s: %s %d of %d", what, noun, i, n);
    return i >= lowest && i < n;
}

// row i stands where row 0 does
static inline bool stands_with_first(const char *what, const char *noun, const std::vector<uint64_t> &at, size_t i)
{
    if (at[i] != at[0])
        set_error("%s: %s %zu stands at %llu, %s 0 at %llu: all %ss of a call stand at the same position", what, noun, i, (unsigned long long)at[i], noun,
                  (unsigned long long)at[0], noun);
    return at[i] == at[0];
}

static inline bool all_stand_together(const char *what, const char *noun, const std::vector<uint64_t> &at)
{
    for (size_t i = 1; i < at.size(); i++)
        if (!stands_with_first(what, noun, at, i)) return false;
    return true;
}

// The spans of a resident call with one input: n_in samples of bps bytes read of each of n_rows streams at pitch_in, n_out
// words (`as_many` as samples, for the sentence) written of each from out_first on at pitch_out.  in_bytes and out_bytes
// reach from the operand's first byte to the last row's last sample read and last word written.
static inline int resident_spans(const char *what, int n_rows, size_t bps, size_t n_in, size_t pitch_in, size_t n_out, const char *as_many,
                                 size_t pitch_out, size_t out_first, size_t *in_bytes, size_t *out_bytes)
{
    const size_t rows = (size_t)n_rows;
    size_t out_end;
    if (__builtin_add_overflow(out_first, n_out, &out_end) || !span_bytes(rows - 1, pitch_in, n_in, bps, in_bytes) ||
        !span_bytes(rows - 1, pitch_out, out_end, 4, out_bytes)) {
        set_error("%s: the span of %zu samples of %d streams at pitch %zu, or of %s words from %zu at pitch %zu, overflows", what, n_in, n_rows, pitch_in,
                  as_many, out_first, pitch_out);
        return NVX_ERR_ARG;
    }
    if (rows > 1 && (n_in > pitch_in || ((pitch_in * bps) & 15) || out_end > pitch_out)) {
        set_error("%s: %zu samples per stream at pitch %zu, words up to %zu at pitch %zu (a row must hold them, and input rows are 16-byte aligned)",
                  what, n_in, pitch_in, out_end, pitch_out);
        return NVX_ERR_ARG;
    }
    return NVX_OK;
}

// The state rows of a plan, [rows][words] of W twice over: a launch reads a row in one and writes it in the other, and
// `parity` says which of the two row i's next launch reads.  The caller holds the plan's lock.
template <typename W> struct nvx_state_rows {
    W *d[2] = { nullptr, nullptr };
    size_t words = 0;
    std::vector<uint8_t> parity;

    size_t bytes(size_t rows) const { return rows * words * sizeof(W); }
    hipError_t allocate(int rows, size_t row_words)
    {
        words = row_words; parity.assign(rows, 0);
        const hipError_t e = hipMalloc((void **)&d[0], bytes(rows));
        return e != hipSuccess ? e : hipMalloc((void **)&d[1], bytes(rows));
    }
    void release() { (void)hipFree(d[0]); (void)hipFree(d[1]); }
    W *row(int i) const { return d[parity[i]] + (size_t)i * words; }
    // what a launch over the rows from `first` on, which stand at parity p, reads and writes
    W *in(int first, int p) const { return d[p] + (size_t)first * words; }
    W *out(int first, int p) const { return d[p ^ 1] + (size_t)first * words; }
    void flip(int first, int n, int p) { for (int i = first; i < first + n; i++) parity[i] = (uint8_t)(p ^ 1); }
    // where the run of rows from i on that lie side by side (at one parity) ends, `end` at the latest
    int run_end(int i, int end) const { int j = i; while (j < end && parity[j] == parity[i]) j++; return j; }
    // Rows pushed one by one are brought to row 0's parity, on s, for a launch over all of them; a row that `skip` marks
    // holds nothing worth the copy.
    int align(const uint8_t *skip, hipStream_t s)
    {
        const int p = parity[0];
        for (size_t i = 1; i < parity.size(); i++)
            if (parity[i] != p) {
                if (!skip || !skip[i]) HIP_TRY(hipMemcpyAsync(d[p] + i * words, d[p ^ 1] + i * words, bytes(1), hipMemcpyDeviceToDevice, s));
                parity[i] = (uint8_t)p;
            }
        return NVX_OK;
    }
};

// A push's input and output on the device; they grow to the largest push.  A failed allocation leaves nothing behind in the
// runtime's last error: the library's next launch reports its own.
struct nvx_push_staging {
    void *d_in = nullptr; uint32_t *d_out = nullptr;
    size_t in_cap = 0, out_cap = 0;     // bytes, words

    static int grow(const char *what, void **p, size_t *cap, size_t units, size_t unit_bytes)
    {
        if (units <= *cap) return NVX_OK;
        (void)hipFree(*p); *p = nullptr; *cap = 0;
        if (hipMalloc(p, units * unit_bytes) != hipSuccess) { (void)hipGetLastError(); set_error("%s: hipMalloc of %zu bytes failed", what, units * unit_bytes); return NVX_ERR_NOMEM; }
        *cap = units;
        return NVX_OK;
    }
    int reserve(const char *what, size_t in_bytes, size_t out_words)
    {
        const int rc = grow(what, &d_in, &in_cap, in_bytes, 1);
        return rc != NVX_OK ? rc : grow(what, (void **)&d_out, &out_cap, out_words, 4);
    }
    void release() { (void)hipFree(d_in); (void)hipFree(d_out); }
};

#endif
