// nvx_real_host.cpp -- the real-input converter's entry points (include/navtex_amd_real.h): the config checks, the plan with
// its carried positions, state rows and held samples, the checks of a call, and a push's staging.  The launch arithmetic is
// nvx_real_plan.h's.  The library stands alone: it shares no state with any other.
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "nvx_companion.h"
#include "nvx_real_plan.h"

extern "C" const char *nvx_real_last_error(void) { return nvx_error_text(); }

static const uint32_t MAGIC = 0x4e524c31u;      // "NRL1"
static const int BPS[4] = { 2, 1, 1, 4 };       // bytes per input sample, by format
static const char *const NOUN = "the real-input converter";

struct nvx_real_converter {
    uint32_t magic = MAGIC;
    std::mutex mu;
    int device = 0, n_streams = 0, format = 0, invert = 0;
    nvx_state_rows<uint32_t> state;                         // [n_streams][NVX_REAL_STATE_WORDS]
    std::vector<uint64_t> consumed;                         // samples the kernel has taken: even
    std::vector<uint8_t> held;                              // 1: a push left an odd sample, in `sample`
    std::vector<uint32_t> sample;                           // its bytes
    nvx_event_timer timer;
    nvx_push_staging push;
    struct { int chunks, tiles_per_chunk, form; } last = {};
    int64_t kernel_launches = 0;
};

static bool valid(const nvx_real_converter *c, const char *what)
{
    if (!c || c->magic != MAGIC) { set_error("%s: not a real-input converter", what); return false; }
    return true;
}

extern "C" void nvx_real_config_default(nvx_real_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0; cfg->format = NVX_REAL_S16; cfg->n_streams = 1; cfg->invert = 0;
}

extern "C" int nvx_real_taps(int16_t *taps, int cap, int *K, int *S)
{
    if (taps && cap < NVX_REAL_NTAPS) { set_error("nvx_real_taps: room for %d taps, there are %d", cap, NVX_REAL_NTAPS); return NVX_ERR_ARG; }
    if (taps) memcpy(taps, NVX_REAL_TAPS, sizeof NVX_REAL_TAPS);
    if (K) *K = NVX_REAL_K;
    if (S) *S = NVX_REAL_S;
    return NVX_REAL_NTAPS;
}

// --------------------------------------------------------------------------------------------------------------- plans
static void release(nvx_real_converter *c)
{
    c->state.release(); c->push.release();
    c->timer.destroy();
    c->magic = 0;
    delete c;
}

extern "C" int nvx_real_create(const nvx_real_config *cfg, nvx_real_converter **out)
{
    const char *what = "nvx_real_create";
    if (!cfg || !out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    *out = nullptr;
    if (cfg->struct_size != sizeof *cfg) { set_error("%s: struct_size %u, this library's nvx_real_config has %zu bytes", what, cfg->struct_size, sizeof *cfg); return NVX_ERR_ARG; }
    if (cfg->n_streams < 1 || cfg->n_streams > 65535) { set_error("%s: n_streams %d (1 .. 65535)", what, cfg->n_streams); return NVX_ERR_ARG; }
    if (cfg->format < NVX_REAL_S16 || cfg->format > NVX_REAL_F32) { set_error("%s: format %d (NVX_REAL_S16 .. NVX_REAL_F32)", what, cfg->format); return NVX_ERR_ARG; }
    if (cfg->device < 0) { set_error("%s: device %d", what, cfg->device); return NVX_ERR_ARG; }
    if (cfg->invert != 0 && cfg->invert != 1) { set_error("%s: invert %d (0 or 1)", what, cfg->invert); return NVX_ERR_ARG; }
    nvx_real_converter *c = new (std::nothrow) nvx_real_converter;
    if (!c) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    int rc = select_device(cfg->device, NOUN);
    if (rc != NVX_OK) { release(c); return rc; }
    c->device = cfg->device; c->n_streams = cfg->n_streams; c->format = cfg->format; c->invert = cfg->invert;
    c->consumed.assign(cfg->n_streams, 0); c->held.assign(cfg->n_streams, 0); c->sample.assign(cfg->n_streams, 0);
    hipError_t e = c->state.allocate(cfg->n_streams, NVX_REAL_STATE_WORDS);
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_NOMEM; }
    const size_t state_bytes = c->state.bytes(cfg->n_streams);
    e = hipMemset(c->state.d[0], 0, state_bytes);
    if (e == hipSuccess) e = hipMemset(c->state.d[1], 0, state_bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: clearing the state failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_HIP; }
    *out = c;
    return NVX_OK;
}

extern "C" void nvx_real_destroy(nvx_real_converter *c)
{
    if (!c || c->magic != MAGIC) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    release(c);
}

extern "C" int nvx_real_plan(nvx_real_converter *c, int *format, int *n_streams, int *invert)
{
    if (!valid(c, "nvx_real_plan")) return NVX_ERR_ARG;
    if (format) *format = c->format;
    if (n_streams) *n_streams = c->n_streams;
    if (invert) *invert = c->invert;
    return NVX_OK;
}

// `stream` (-1: all) stands at sample `position` with silence in front of it and no sample held
static int restart(nvx_real_converter *c, const char *what, int stream, uint64_t position)
{
    if (!row_ok(what, "stream", stream, -1, c->n_streams)) return NVX_ERR_ARG;
    if ((position >> 62) || (position & 1)) { set_error("%s: position %llu (even, below 2^62)", what, (unsigned long long)position); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const int first = stream < 0 ? 0 : stream, n = stream < 0 ? c->n_streams : 1;
    for (int i = first, j; i < first + n; i = j) {          // runs of streams whose rows lie side by side
        j = c->state.run_end(i, first + n);
        HIP_TRY(hipMemset(c->state.row(i), 0, c->state.bytes(j - i)));
    }
    HIP_TRY(hipDeviceSynchronize());
    for (int i = first; i < first + n; i++) { c->consumed[i] = position; c->held[i] = 0; }
    return NVX_OK;
}

extern "C" int nvx_real_reset(nvx_real_converter *c, int stream)
{
    return valid(c, "nvx_real_reset") ? restart(c, "nvx_real_reset", stream, 0) : NVX_ERR_ARG;
}

extern "C" int nvx_real_debug_set_position(nvx_real_converter *c, int stream, uint64_t position)
{
    return valid(c, "nvx_real_debug_set_position") ? restart(c, "nvx_real_debug_set_position", stream, position) : NVX_ERR_ARG;
}

extern "C" int nvx_real_position(nvx_real_converter *c, int stream, uint64_t *consumed, uint64_t *produced)
{
    const char *what = "nvx_real_position";
    if (!valid(c, what) || !row_ok(what, "stream", stream, 0, c->n_streams)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (consumed) *consumed = c->consumed[stream] + c->held[stream];
    if (produced) *produced = c->consumed[stream] / 2;
    return NVX_OK;
}

extern "C" int nvx_real_timing(nvx_real_converter *c, int enable)
{
    return valid(c, "nvx_real_timing") ? timing_enable(c->mu, c->timer, enable) : NVX_ERR_ARG;
}

extern "C" int nvx_real_time_stats(nvx_real_converter *c, double *sum_ms, uint64_t *calls, int reset)
{
    return valid(c, "nvx_real_time_stats") ? timing_collect(c->mu, c->timer, sum_ms, calls, reset) : NVX_ERR_ARG;
}

extern "C" int64_t nvx_real_debug_last_launch(nvx_real_converter *c, int *chunks, int *tiles_per_chunk, int *form)
{
    if (!valid(c, "nvx_real_debug_last_launch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->kernel_launches) {
        if (chunks) *chunks = c->last.chunks;
        if (tiles_per_chunk) *tiles_per_chunk = c->last.tiles_per_chunk;
        if (form) *form = c->last.form;
    }
    return c->kernel_launches;
}

// ------------------------------------------------------------------------------------------------------------ launches
// One call over streams [first, first + n) of the plan, which stand at `consumed` and read state row `parity`; the caller
// holds the plan's lock and has checked every span.  n_in is even and not zero.
static int launch(nvx_real_converter *c, int first, int n, uint64_t consumed, int parity, const void *d_in, size_t pitch_in, size_t n_in,
                  uint32_t *d_out, size_t pitch_out, size_t out_first, hipStream_t s)
{
    nvx_real_args a;
    const int chunks = nvx_real_fill_args(consumed, d_in, pitch_in, n_in, d_out, pitch_out, out_first, n, c->state.in(first, parity),
                                          c->state.out(first, parity), c->invert, nvx_stream_wanted(n, NVX_REAL_TARGET_WORKGROUPS), &a);
    nvx_event_timer::events ev;
    int rc;
    if ((rc = c->timer.begin(s, ev)) != NVX_OK) return rc;
    HIP_TRY(nvx_real_launch(&a, c->format, n, chunks, s));
    c->last = { chunks, a.tiles_per_chunk, chunks > 1 ? 2 : 1 };
    c->kernel_launches += 1;
    if ((rc = c->timer.end(s, ev)) != NVX_OK) return rc;
    for (int i = first; i < first + n; i++) c->consumed[i] = consumed + n_in;
    c->state.flip(first, n, parity);
    return NVX_OK;
}

extern "C" int nvx_real_resident(nvx_real_converter *c, const void *d_in, size_t pitch_in, size_t n_in, void *d_out, size_t pitch_out,
                                 size_t out_first, void *hip_stream)
{
    const char *what = "nvx_real_resident";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!d_in || !d_out || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 3) || n_in > NVX_REAL_MAX_IN || (n_in & 1)) {
        set_error("%s: bad argument (null pointer, input not 16-byte aligned, output not 4-byte aligned, an odd number of samples, or more than 2^31)", what);
        return NVX_ERR_ARG;
    }
    for (int i = 0; i < c->n_streams; i++) {
        if (c->held[i]) {
            set_error("%s: stream %d holds the odd sample of a push: push one more sample, or reset it", what, i);
            return NVX_ERR_STATE;
        }
        if (!stands_with_first(what, "stream", c->consumed, i)) return NVX_ERR_STATE;
    }
    const uint64_t consumed = c->consumed[0];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    size_t in_bytes, out_bytes;
    int rc = resident_spans(what, c->n_streams, (size_t)BPS[c->format], n_in, pitch_in, n_in / 2, "half as many", pitch_out, out_first, &in_bytes, &out_bytes);
    if (rc != NVX_OK || n_in == 0) return rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_in, in_bytes, what, "input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out, out_bytes, what, "output")) != NVX_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    if ((rc = c->state.align(nullptr, s)) != NVX_OK) return rc;
    return launch(c, 0, c->n_streams, consumed, c->state.parity[0], d_in, pitch_in, n_in, (uint32_t *)d_out, pitch_out, out_first, s);
}

extern "C" int nvx_real_push(nvx_real_converter *c, int stream, const void *in, size_t n_in, int16_t *out_iq, size_t cap_samples, size_t *n_out)
{
    const char *what = "nvx_real_push";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (stream < 0 || stream >= c->n_streams || !in || !out_iq || !n_out || n_in > NVX_REAL_MAX_IN) {
        set_error("%s: bad argument (stream %d of %d, null pointer, or more than 2^31 samples)", what, stream, c->n_streams);
        return NVX_ERR_ARG;
    }
    const size_t bps = (size_t)BPS[c->format], have = n_in + c->held[stream], use = have & ~(size_t)1, words = use / 2;
    if (words > cap_samples) { set_error("%s: %zu outputs, room for %zu", what, words, cap_samples); return NVX_ERR_ARG; }
    const uint64_t consumed = c->consumed[stream];
    if (!position_ok(what, consumed + have)) return NVX_ERR_ARG;
    *n_out = 0;
    if (use) {
        int rc;
        if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
        const size_t in_bytes = use * bps;
        if ((rc = c->push.reserve(what, in_bytes, words)) != NVX_OK) return rc;
        // the held sample goes in front
        const size_t front = c->held[stream] ? bps : 0;
        if (front) HIP_TRY(hipMemcpy(c->push.d_in, &c->sample[stream], bps, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy((char *)c->push.d_in + front, in, in_bytes - front, hipMemcpyHostToDevice));
        if ((rc = launch(c, stream, 1, consumed, c->state.parity[stream], c->push.d_in, use, use, c->push.d_out, words, 0, nullptr)) != NVX_OK) return rc;
        HIP_TRY(hipMemcpy(out_iq, c->push.d_out, words * 4, hipMemcpyDeviceToHost));    // waits for the null stream
        *n_out = words;
    }
    if (have & 1) {                                         // the last sample waits for its partner
        uint32_t v = 0;
        if (n_in) memcpy(&v, (const char *)in + (n_in - 1) * bps, bps); else v = c->sample[stream];
        c->sample[stream] = v; c->held[stream] = 1;
    } else c->held[stream] = 0;
    return NVX_OK;
}
