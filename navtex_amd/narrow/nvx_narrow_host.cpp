// nvx_narrow_host.cpp -- the narrowband interpolator's entry points (include/navtex_amd_narrow.h): the design without a
// device, the config checks, the plan with its tap table and carried positions, and the checks of a call.  The state rows,
// a push's staging, the row and position checks and the timing bodies are nvx_companion.h's, the launch arithmetic
// nvx_narrow_plan.h's.  The library stands alone: it shares no state with any other.
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "nvx_companion.h"
#include "nvx_narrow_plan.h"

extern "C" const char *nvx_nb_last_error(void) { return nvx_error_text(); }

static const uint32_t MAGIC = 0x4e4e4231u;      // "NNB1"
static const int BPS[2][4] = { { 4, 2, 2, 8 }, { 2, 1, 1, 4 } };      // bytes per input sample, by kind and format
static const char *const NOUN = "the narrowband interpolator";

struct nvx_nb_interpolator {
    uint32_t magic = MAGIC;
    std::mutex mu;
    int device = 0, n_streams = 0, format = 0, kind = 0;
    nvx_nb_args shape = {};                                 // L, M, T and what follows from them
    uint32_t *d_table = nullptr;
    nvx_state_rows<uint32_t> state;                         // [n_streams][NVX_NB_STATE_WORDS]
    std::vector<uint64_t> consumed;
    nvx_event_timer timer;
    nvx_push_staging push;
    struct { int chunks, tiles_per_chunk, form; size_t lds_bytes; } last = {};
    int64_t kernel_launches = 0;

    size_t bps() const { return (size_t)BPS[kind][format]; }
};

static bool valid(const nvx_nb_interpolator *c, const char *what)
{
    if (!c || c->magic != MAGIC) { set_error("%s: not a narrowband interpolator", what); return false; }
    return true;
}

// ------------------------------------------------------------------------------------------------------ without a device
extern "C" int nvx_nb_design(uint32_t rate_num, uint32_t rate_den, int *L, int *M, int *T, int16_t *taps, int cap)
{
    int l, m, t;
    const char *why = "";
    if (nvx_nb_plan_numbers(rate_num, rate_den, &l, &m, &t, &why) != NVX_OK) {
        set_error("nvx_nb_design: %u / %u S/s: %s", rate_num, rate_den, why);
        return NVX_ERR_ARG;
    }
    if (cap < 0) { set_error("nvx_nb_design: cap %d", cap); return NVX_ERR_ARG; }
    if (L) *L = l;
    if (M) *M = m;
    if (T) *T = t;
    if (taps && cap >= l * t) {
        const int rc = nvx_nb_plan_taps(l, t, taps, &why);
        if (rc != NVX_OK) { set_error("nvx_nb_design: %u / %u S/s: %s", rate_num, rate_den, why); return rc; }
    }
    return l * t;
}

extern "C" void nvx_nb_config_default(nvx_nb_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0; cfg->n_streams = 1; cfg->rate_num = 12000; cfg->rate_den = 1; cfg->format = NVX_NB_S16; cfg->kind = NVX_NB_IQ;
}

// --------------------------------------------------------------------------------------------------------------- plans
static void release(nvx_nb_interpolator *c)
{
    (void)hipFree(c->d_table);
    c->state.release(); c->push.release();
    c->timer.destroy();
    c->magic = 0;
    delete c;
}

extern "C" int nvx_nb_create(const nvx_nb_config *cfg, nvx_nb_interpolator **out)
{
    const char *what = "nvx_nb_create";
    if (!cfg || !out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    *out = nullptr;
    if (cfg->struct_size != sizeof *cfg) { set_error("%s: struct_size %u, this library's nvx_nb_config has %zu bytes", what, cfg->struct_size, sizeof *cfg); return NVX_ERR_ARG; }
    if (cfg->n_streams < 1 || cfg->n_streams > 65535) { set_error("%s: n_streams %d (1 .. 65535)", what, cfg->n_streams); return NVX_ERR_ARG; }
    if (cfg->format < NVX_NB_S16 || cfg->format > NVX_NB_F32) { set_error("%s: format %d (NVX_NB_S16 .. NVX_NB_F32)", what, cfg->format); return NVX_ERR_ARG; }
    if (cfg->kind != NVX_NB_IQ && cfg->kind != NVX_NB_REAL) { set_error("%s: kind %d (NVX_NB_IQ or NVX_NB_REAL)", what, cfg->kind); return NVX_ERR_ARG; }
    if (cfg->device < 0) { set_error("%s: device %d", what, cfg->device); return NVX_ERR_ARG; }
    int L, M, T;
    const char *why = "";
    if (nvx_nb_plan_numbers(cfg->rate_num, cfg->rate_den, &L, &M, &T, &why) != NVX_OK) {
        set_error("%s: %u / %u S/s: %s", what, cfg->rate_num, cfg->rate_den, why);
        return NVX_ERR_ARG;
    }
    std::vector<int16_t> taps((size_t)L * T);
    int rc = nvx_nb_plan_taps(L, T, taps.data(), &why);
    if (rc != NVX_OK) { set_error("%s: %u / %u S/s: %s", what, cfg->rate_num, cfg->rate_den, why); return rc; }
    nvx_nb_interpolator *c = new (std::nothrow) nvx_nb_interpolator;
    if (!c) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    rc = select_device(cfg->device, NOUN);
    if (rc != NVX_OK) { release(c); return rc; }
    c->device = cfg->device; c->n_streams = cfg->n_streams; c->format = cfg->format; c->kind = cfg->kind;
    nvx_nb_fill_shape(L, M, T, &c->shape);
    c->consumed.assign(cfg->n_streams, 0);
    // the table as the kernel reads it: rows of Tp int16, zeros in front of the phase's taps reversed
    const int Tp = 8 * c->shape.tq, row = 8 * c->shape.row_quads;
    std::vector<int16_t> table((size_t)L * row, 0);
    for (int r = 0; r < L; r++)
        for (int t = 0; t < T; t++) table[(size_t)r * row + (Tp - 1 - t)] = taps[(size_t)r * T + t];
    const size_t table_bytes = table.size() * sizeof(int16_t);
    hipError_t e = hipMalloc((void **)&c->d_table, table_bytes);
    if (e == hipSuccess) e = c->state.allocate(cfg->n_streams, NVX_NB_STATE_WORDS);
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_NOMEM; }
    e = hipMemcpy(c->d_table, table.data(), table_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(c->state.d[0], 0, c->state.bytes(cfg->n_streams));
    if (e == hipSuccess) e = hipMemset(c->state.d[1], 0, c->state.bytes(cfg->n_streams));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: filling the table and the state failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_HIP; }
    nvx_nb_prepare();
    *out = c;
    return NVX_OK;
}

extern "C" void nvx_nb_destroy(nvx_nb_interpolator *c)
{
    if (!c || c->magic != MAGIC) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    release(c);
}

extern "C" int nvx_nb_plan(nvx_nb_interpolator *c, int *L, int *M, int *T, int *n_streams, int *format, int *kind)
{
    if (!valid(c, "nvx_nb_plan")) return NVX_ERR_ARG;
    if (L) *L = c->shape.L;
    if (M) *M = c->shape.M;
    if (T) *T = c->shape.T;
    if (n_streams) *n_streams = c->n_streams;
    if (format) *format = c->format;
    if (kind) *kind = c->kind;
    return NVX_OK;
}

// `stream` (-1: all) stands at input sample `position` with silence in front of it
static int restart(nvx_nb_interpolator *c, const char *what, int stream, uint64_t position)
{
    if (!row_ok(what, "stream", stream, -1, c->n_streams)) return NVX_ERR_ARG;
    if (position >> 62) { set_error("%s: position %llu (below 2^62)", what, (unsigned long long)position); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const int first = stream < 0 ? 0 : stream, n = stream < 0 ? c->n_streams : 1;
    HIP_TRY(hipMemset(c->state.in(first, 0), 0, c->state.bytes(n)));
    HIP_TRY(hipMemset(c->state.in(first, 1), 0, c->state.bytes(n)));
    HIP_TRY(hipDeviceSynchronize());
    for (int i = first; i < first + n; i++) c->consumed[i] = position;
    return NVX_OK;
}

extern "C" int nvx_nb_reset(nvx_nb_interpolator *c, int stream)
{
    return valid(c, "nvx_nb_reset") ? restart(c, "nvx_nb_reset", stream, 0) : NVX_ERR_ARG;
}

extern "C" int nvx_nb_debug_set_position(nvx_nb_interpolator *c, int stream, uint64_t position)
{
    return valid(c, "nvx_nb_debug_set_position") ? restart(c, "nvx_nb_debug_set_position", stream, position) : NVX_ERR_ARG;
}

extern "C" int nvx_nb_position(nvx_nb_interpolator *c, int stream, uint64_t *consumed, uint64_t *produced)
{
    const char *what = "nvx_nb_position";
    if (!valid(c, what) || !row_ok(what, "stream", stream, 0, c->n_streams)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (consumed) *consumed = c->consumed[stream];
    if (produced) *produced = nvx_nb_outputs_after(c->consumed[stream], c->shape.L, c->shape.M);
    return NVX_OK;
}

extern "C" int nvx_nb_timing(nvx_nb_interpolator *c, int enable)
{
    return valid(c, "nvx_nb_timing") ? timing_enable(c->mu, c->timer, enable) : NVX_ERR_ARG;
}

extern "C" int nvx_nb_time_stats(nvx_nb_interpolator *c, double *sum_ms, uint64_t *calls, int reset)
{
    return valid(c, "nvx_nb_time_stats") ? timing_collect(c->mu, c->timer, sum_ms, calls, reset) : NVX_ERR_ARG;
}

extern "C" int64_t nvx_nb_debug_last_launch(nvx_nb_interpolator *c, int *chunks, int *tiles_per_chunk, int *form, int *windows, int *parts,
                                            size_t *lds_bytes)
{
    if (!valid(c, "nvx_nb_debug_last_launch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->kernel_launches) {
        if (chunks) *chunks = c->last.chunks;
        if (tiles_per_chunk) *tiles_per_chunk = c->last.tiles_per_chunk;
        if (form) *form = c->last.form;
        if (windows) *windows = c->shape.windows;
        if (parts) *parts = 1 << c->shape.pshift;
        if (lds_bytes) *lds_bytes = c->last.lds_bytes;
    }
    return c->kernel_launches;
}

// ------------------------------------------------------------------------------------------------------------ launches
// The outputs of a call of n_in samples on a stream at `consumed`; false where the position passes 2^62 or they reach 2^31.
static bool call_outputs(const nvx_nb_interpolator *c, const char *what, uint64_t consumed, size_t n_in, size_t *outs)
{
    if (n_in > NVX_NB_MAX_IN) { set_error("%s: %zu samples (at most 2^30 per call)", what, n_in); return false; }
    if (!position_ok(what, consumed + n_in)) return false;
    const uint64_t n = (uint64_t)(nvx_nb_outputs_after_wide(consumed + n_in, c->shape.L, c->shape.M) - nvx_nb_outputs_after_wide(consumed, c->shape.L, c->shape.M));
    if (n >> 31) { set_error("%s: %zu samples give %llu outputs: a call's outputs stay below 2^31", what, n_in, (unsigned long long)n); return false; }
    *outs = (size_t)n;
    return true;
}

// One call over streams [first, first + n) of the plan, which stand at `consumed` and read state row `parity`; the caller
// holds the plan's lock and has checked every span.  n_in is not zero.
static int launch(nvx_nb_interpolator *c, int first, int n, uint64_t consumed, int parity, const void *d_in, size_t pitch_in, size_t n_in,
                  uint32_t *d_out, size_t pitch_out, size_t out_first, hipStream_t s)
{
    nvx_nb_args a = c->shape;
    const int chunks = nvx_nb_fill_args(consumed, d_in, pitch_in, n_in, d_out, pitch_out, out_first, c->state.in(first, parity),
                                        c->state.out(first, parity), c->d_table, nvx_stream_wanted(n, NVX_NB_TARGET_WORKGROUPS), &a);
    nvx_event_timer::events ev;
    int rc;
    if ((rc = c->timer.begin(s, ev)) != NVX_OK) return rc;
    HIP_TRY(nvx_nb_launch(&a, c->format, c->kind, n, chunks, s));
    c->last = { chunks, a.tiles_per_chunk, chunks > 1 ? 2 : 1, nvx_nb_lds_bytes(&a) };
    c->kernel_launches += 1;
    if ((rc = c->timer.end(s, ev)) != NVX_OK) return rc;
    for (int i = first; i < first + n; i++) c->consumed[i] = consumed + n_in;
    c->state.flip(first, n, parity);
    return NVX_OK;
}

extern "C" int nvx_nb_resident(nvx_nb_interpolator *c, const void *d_in, size_t pitch_in, size_t n_in, void *d_out, size_t pitch_out,
                               size_t out_first, size_t *n_out, void *hip_stream)
{
    const char *what = "nvx_nb_resident";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!d_in || !d_out || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 3)) {
        set_error("%s: bad argument (null pointer, input not 16-byte aligned, or output not 4-byte aligned)", what);
        return NVX_ERR_ARG;
    }
    if (!all_stand_together(what, "stream", c->consumed)) return NVX_ERR_STATE;
    const uint64_t consumed = c->consumed[0];
    size_t outs;
    if (!call_outputs(c, what, consumed, n_in, &outs)) return NVX_ERR_ARG;
    // every row's last sample read and last word written, in samples of its row (out_end) and in bytes of the whole operand
    const size_t rows = (size_t)c->n_streams;
    size_t out_end, in_bytes, out_bytes;
    if (__builtin_add_overflow(out_first, outs, &out_end) || !span_bytes(rows - 1, pitch_in, n_in, c->bps(), &in_bytes) ||
        !span_bytes(rows - 1, pitch_out, out_end, 4, &out_bytes)) {
        set_error("%s: the span of %zu samples of %d streams at pitch %zu, or of %zu outputs from %zu at pitch %zu, overflows", what, n_in,
                  c->n_streams, pitch_in, outs, out_first, pitch_out);
        return NVX_ERR_ARG;
    }
    if (rows > 1 && (n_in > pitch_in || ((pitch_in * c->bps()) & 15) || out_end > pitch_out)) {
        set_error("%s: %zu samples per stream at pitch %zu, words up to %zu at pitch %zu (a row must hold them, and input rows are 16-byte aligned)",
                  what, n_in, pitch_in, out_end, pitch_out);
        return NVX_ERR_ARG;
    }
    if (n_out) *n_out = outs;
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_in, in_bytes, what, "input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out, out_bytes, what, "output")) != NVX_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    // the state rows of streams pushed one by one are brought to stream 0's parity
    if ((rc = c->state.align(nullptr, s)) != NVX_OK) return rc;
    return launch(c, 0, c->n_streams, consumed, c->state.parity[0], d_in, pitch_in, n_in, (uint32_t *)d_out, pitch_out, out_first, s);
}

extern "C" int nvx_nb_push(nvx_nb_interpolator *c, int stream, const void *in, size_t n_in, int16_t *out_iq, size_t cap_samples, size_t *n_out)
{
    const char *what = "nvx_nb_push";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (stream < 0 || stream >= c->n_streams || !in || !out_iq) {
        set_error("%s: bad argument (stream %d of %d, or null pointer)", what, stream, c->n_streams);
        return NVX_ERR_ARG;
    }
    const uint64_t consumed = c->consumed[stream];
    size_t outs;
    if (!call_outputs(c, what, consumed, n_in, &outs)) return NVX_ERR_ARG;
    if (outs > cap_samples) { set_error("%s: %zu samples give %zu outputs, the buffer holds %zu: nothing consumed", what, n_in, outs, cap_samples); return NVX_ERR_ARG; }
    if (n_out) *n_out = outs;
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    const size_t in_bytes = n_in * c->bps();
    if ((rc = c->push.reserve(what, in_bytes, outs)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(c->push.d_in, in, in_bytes, hipMemcpyHostToDevice));
    if ((rc = launch(c, stream, 1, consumed, c->state.parity[stream], c->push.d_in, n_in, n_in, c->push.d_out, outs, 0, nullptr)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(out_iq, c->push.d_out, outs * 4, hipMemcpyDeviceToHost));     // waits for the null stream
    return NVX_OK;
}
