// nvx_blank_host.cpp -- the blanker's entry points (include/navtex_amd_blank.h): the config checks, the plan with its
// carried positions, state rows and counters, the checks of a call, the choice of kernel form, a push's staging.  The launch
// arithmetic is nvx_blank_plan.h's.  The library stands alone: it shares no state with any other.
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "nvx_companion.h"
#include "nvx_blank_plan.h"

extern "C" const char *nvx_blank_last_error(void) { return nvx_error_text(); }

static const uint32_t MAGIC = 0x4e424c31u;      // "NBL1"
static const int BPS[4] = { 4, 2, 2, 8 };       // bytes per input sample, by format
static const char *const NOUN = "the blanker";

struct nvx_blanker {
    uint32_t magic = MAGIC;
    std::mutex mu;
    int device = 0, n_streams = 0, format = 0;
    uint32_t thr_q8 = 0, hold = 0, floor = 0;
    nvx_state_rows<uint32_t> state;                         // [n_streams][NVX_BLANK_STATE_WORDS]
    unsigned long long *d_counters = nullptr;               // [n_streams][2]
    std::vector<uint64_t> consumed, samples;                // samples: since the last nvx_blank_stats(reset)
    std::vector<uint8_t> fresh;                             // reset since its last launch: that row is zeroed first
    nvx_event_timer timer;
    nvx_push_staging push;
    struct { int chunks, blocks_per_chunk, preroll_blocks, form; } last = {};
    int64_t kernel_launches = 0;
};

static bool valid(const nvx_blanker *b, const char *what)
{
    if (!b || b->magic != MAGIC) { set_error("%s: not a blanker", what); return false; }
    return true;
}

extern "C" void nvx_blank_config_default(nvx_blank_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0; cfg->format = NVX_BLANK_CS16; cfg->n_streams = 1;
    cfg->thr_q8 = NVX_BLANK_THR_DEFAULT; cfg->hold = NVX_BLANK_HOLD_DEFAULT; cfg->floor = NVX_BLANK_FLOOR_DEFAULT;
}

// --------------------------------------------------------------------------------------------------------------- plans
static void release(nvx_blanker *b)
{
    b->state.release(); (void)hipFree(b->d_counters); b->push.release();
    b->timer.destroy();
    b->magic = 0;
    delete b;
}

extern "C" int nvx_blank_create(const nvx_blank_config *cfg, nvx_blanker **out)
{
    const char *what = "nvx_blank_create";
    if (!cfg || !out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    *out = nullptr;
    if (cfg->struct_size != sizeof *cfg) { set_error("%s: struct_size %u, this library's nvx_blank_config has %zu bytes", what, cfg->struct_size, sizeof *cfg); return NVX_ERR_ARG; }
    if (cfg->n_streams < 1 || cfg->n_streams > 65535) { set_error("%s: n_streams %d (1 .. 65535)", what, cfg->n_streams); return NVX_ERR_ARG; }
    if (cfg->format < NVX_BLANK_CS16 || cfg->format > NVX_BLANK_CF32) { set_error("%s: format %d (NVX_BLANK_CS16 .. NVX_BLANK_CF32)", what, cfg->format); return NVX_ERR_ARG; }
    if (cfg->device < 0) { set_error("%s: device %d", what, cfg->device); return NVX_ERR_ARG; }
    if (cfg->thr_q8 != 0 && (cfg->thr_q8 < NVX_BLANK_THR_MIN || cfg->thr_q8 > NVX_BLANK_THR_MAX)) {
        set_error("%s: thr_q8 %u (0: bypass, or %d .. %d)", what, cfg->thr_q8, NVX_BLANK_THR_MIN, NVX_BLANK_THR_MAX);
        return NVX_ERR_ARG;
    }
    if (cfg->hold > NVX_BLANK_HOLD_MAX) { set_error("%s: hold %u (0 .. %d)", what, cfg->hold, NVX_BLANK_HOLD_MAX); return NVX_ERR_ARG; }
    if (cfg->floor > NVX_BLANK_FLOOR_MAX) { set_error("%s: floor %u (0 .. %d)", what, cfg->floor, NVX_BLANK_FLOOR_MAX); return NVX_ERR_ARG; }
    nvx_blanker *b = new (std::nothrow) nvx_blanker;
    if (!b) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    int rc = select_device(cfg->device, NOUN);
    if (rc != NVX_OK) { release(b); return rc; }
    b->device = cfg->device; b->n_streams = cfg->n_streams; b->format = cfg->format;
    b->thr_q8 = cfg->thr_q8; b->hold = cfg->hold; b->floor = cfg->floor;
    b->consumed.assign(cfg->n_streams, 0); b->samples.assign(cfg->n_streams, 0); b->fresh.assign(cfg->n_streams, 0);
    const size_t counter_bytes = (size_t)cfg->n_streams * 2 * sizeof(unsigned long long);
    hipError_t e = b->state.allocate(cfg->n_streams, NVX_BLANK_STATE_WORDS);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_counters, counter_bytes);
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); release(b); return NVX_ERR_NOMEM; }
    const size_t state_bytes = b->state.bytes(cfg->n_streams);
    e = hipMemset(b->state.d[0], 0, state_bytes);
    if (e == hipSuccess) e = hipMemset(b->state.d[1], 0, state_bytes);
    if (e == hipSuccess) e = hipMemset(b->d_counters, 0, counter_bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: clearing the state failed: %s", what, hipGetErrorString(e)); release(b); return NVX_ERR_HIP; }
    *out = b;
    return NVX_OK;
}

extern "C" void nvx_blank_destroy(nvx_blanker *b)
{
    if (!b || b->magic != MAGIC) return;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();
    release(b);
}

extern "C" int nvx_blank_plan(nvx_blanker *b, int *format, int *n_streams, uint32_t *thr_q8, uint32_t *hold, uint32_t *floor)
{
    if (!valid(b, "nvx_blank_plan")) return NVX_ERR_ARG;
    if (format) *format = b->format;
    if (n_streams) *n_streams = b->n_streams;
    if (thr_q8) *thr_q8 = b->thr_q8;
    if (hold) *hold = b->hold;
    if (floor) *floor = b->floor;
    return NVX_OK;
}

// `stream` (-1: all) stands at `position` with nothing in front of it
static int restart(nvx_blanker *b, const char *what, int stream, uint64_t position)
{
    if (!row_ok(what, "stream", stream, -1, b->n_streams)) return NVX_ERR_ARG;
    if (!position_ok(what, position)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    for (int i = stream < 0 ? 0 : stream; i < (stream < 0 ? b->n_streams : stream + 1); i++) { b->consumed[i] = position; b->fresh[i] = 1; }
    return NVX_OK;
}

extern "C" int nvx_blank_reset(nvx_blanker *b, int stream)
{
    return valid(b, "nvx_blank_reset") ? restart(b, "nvx_blank_reset", stream, 0) : NVX_ERR_ARG;
}

extern "C" int nvx_blank_debug_set_position(nvx_blanker *b, int stream, uint64_t position)
{
    return valid(b, "nvx_blank_debug_set_position") ? restart(b, "nvx_blank_debug_set_position", stream, position) : NVX_ERR_ARG;
}

extern "C" int nvx_blank_position(nvx_blanker *b, int stream, uint64_t *consumed)
{
    const char *what = "nvx_blank_position";
    if (!valid(b, what)) return NVX_ERR_ARG;
    if (!row_ok(what, "stream", stream, 0, b->n_streams)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    if (consumed) *consumed = b->consumed[stream];
    return NVX_OK;
}

extern "C" int nvx_blank_stats(nvx_blanker *b, int stream, uint64_t *samples, uint64_t *detections, uint64_t *blanked, int reset)
{
    const char *what = "nvx_blank_stats";
    if (!valid(b, what)) return NVX_ERR_ARG;
    if (!row_ok(what, "stream", stream, 0, b->n_streams)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    int rc;
    if ((rc = select_device(b->device, NOUN)) != NVX_OK) return rc;
    unsigned long long c[2] = { 0, 0 };
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(c, b->d_counters + 2 * (size_t)stream, sizeof c, hipMemcpyDeviceToHost));
    if (samples) *samples = b->samples[stream];
    if (detections) *detections = c[0];
    if (blanked) *blanked = c[1];
    if (reset) {
        HIP_TRY(hipMemset(b->d_counters + 2 * (size_t)stream, 0, sizeof c));
        HIP_TRY(hipDeviceSynchronize());
        b->samples[stream] = 0;
    }
    return NVX_OK;
}

extern "C" int nvx_blank_timing(nvx_blanker *b, int enable)
{
    return valid(b, "nvx_blank_timing") ? timing_enable(b->mu, b->timer, enable) : NVX_ERR_ARG;
}

extern "C" int nvx_blank_time_stats(nvx_blanker *b, double *sum_ms, uint64_t *launches, int reset)
{
    return valid(b, "nvx_blank_time_stats") ? timing_collect(b->mu, b->timer, sum_ms, launches, reset) : NVX_ERR_ARG;
}

extern "C" int64_t nvx_blank_debug_last_launch(nvx_blanker *b, int *chunks, int *blocks_per_chunk, int *preroll_blocks, int *form)
{
    if (!valid(b, "nvx_blank_debug_last_launch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    if (b->kernel_launches) {
        if (chunks) *chunks = b->last.chunks;
        if (blocks_per_chunk) *blocks_per_chunk = b->last.blocks_per_chunk;
        if (preroll_blocks) *preroll_blocks = b->last.preroll_blocks;
        if (form) *form = b->last.form;
    }
    return b->kernel_launches;
}

// ------------------------------------------------------------------------------------------------------------ launches
// One launch over streams [first, first + n) of the plan, which stand at `consumed` and read state row `parity`; the caller
// holds the plan's lock and has checked every span.
static int launch(nvx_blanker *b, int first, int n, uint64_t consumed, int parity, const void *d_in, size_t pitch_in, size_t n_in,
                  uint32_t *d_out, size_t pitch_out, size_t out_first, hipStream_t s)
{
    // the state rows the launch reads: those of streams reset since their last launch are zeroed first, run by run
    for (int i = first; i < first + n;) {
        if (!b->fresh[i]) { i++; continue; }
        int j = i;
        while (j < first + n && b->fresh[j]) b->fresh[j++] = 0;
        HIP_TRY(hipMemsetAsync(b->state.in(i, parity), 0, b->state.bytes(j - i), s));
        i = j;
    }
    nvx_blank_args a;
    const int chunks = nvx_blank_fill_args(consumed, d_in, pitch_in, n_in, d_out, pitch_out, out_first, n, b->state.in(first, parity),
                                           b->state.out(first, parity), b->d_counters + 2 * (size_t)first, b->thr_q8, b->hold, b->floor,
                                           nvx_stream_wanted(n, NVX_BLANK_TARGET_WORKGROUPS), &a);
    nvx_event_timer::events ev;
    int rc;
    if ((rc = b->timer.begin(s, ev)) != NVX_OK) return rc;
    HIP_TRY(nvx_blank_launch(&a, b->format, n, chunks, s));
    b->last = { chunks, a.tiles_per_chunk * NVX_BLANK_WAVES, chunks > 1 ? NVX_BLANK_PREROLL_TILES * NVX_BLANK_WAVES : 0, chunks > 1 ? 2 : 1 };
    b->kernel_launches++;
    if ((rc = b->timer.end(s, ev)) != NVX_OK) return rc;
    for (int i = first; i < first + n; i++) { b->consumed[i] = consumed + n_in; b->samples[i] += n_in; }
    b->state.flip(first, n, parity);
    return NVX_OK;
}

extern "C" int nvx_blank_resident(nvx_blanker *b, const void *d_in, size_t pitch_in, size_t n_in, void *d_out, size_t pitch_out,
                                  size_t out_first, void *hip_stream)
{
    const char *what = "nvx_blank_resident";
    if (!valid(b, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    if (!d_in || !d_out || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 3) || n_in > NVX_BLANK_MAX_IN) {
        set_error("%s: bad argument (null pointer, input not 16-byte aligned, output not 4-byte aligned, or more than 2^30 samples)", what);
        return NVX_ERR_ARG;
    }
    if (!all_stand_together(what, "stream", b->consumed)) return NVX_ERR_STATE;
    const uint64_t consumed = b->consumed[0];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    size_t in_bytes, out_bytes;
    int rc = resident_spans(what, b->n_streams, (size_t)BPS[b->format], n_in, pitch_in, n_in, "as many", pitch_out, out_first, &in_bytes, &out_bytes);
    if (rc != NVX_OK || n_in == 0) return rc;
    if ((rc = select_device(b->device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_in, in_bytes, what, "input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out, out_bytes, what, "output")) != NVX_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    if ((rc = b->state.align(b->fresh.data(), s)) != NVX_OK) return rc;     // a fresh row is zeroed by the launch
    return launch(b, 0, b->n_streams, consumed, b->state.parity[0], d_in, pitch_in, n_in, (uint32_t *)d_out, pitch_out, out_first, s);
}

extern "C" int nvx_blank_push(nvx_blanker *b, int stream, const void *in, size_t n_in, int16_t *out_iq)
{
    const char *what = "nvx_blank_push";
    if (!valid(b, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(b->mu);
    if (stream < 0 || stream >= b->n_streams || !in || !out_iq || n_in > NVX_BLANK_MAX_IN) {
        set_error("%s: bad argument (stream %d of %d, null pointer, or more than 2^30 samples)", what, stream, b->n_streams);
        return NVX_ERR_ARG;
    }
    const uint64_t consumed = b->consumed[stream];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(b->device, NOUN)) != NVX_OK) return rc;
    const size_t in_bytes = n_in * (size_t)BPS[b->format];
    if ((rc = b->push.reserve(what, in_bytes, n_in)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(b->push.d_in, in, in_bytes, hipMemcpyHostToDevice));
    if ((rc = launch(b, stream, 1, consumed, b->state.parity[stream], b->push.d_in, n_in, n_in, b->push.d_out, n_in, 0, nullptr)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(out_iq, b->push.d_out, n_in * 4, hipMemcpyDeviceToHost));     // waits for the null stream
    return NVX_OK;
}
