// nvx_align_host.cpp -- the row aligner's entry points that need a device (include/navtex_amd_align.h): the config checks, the
// plan with its carried positions, delays and state rows, the checks of a call, a push's staging and the measurement's
// tables.  The launch arithmetic is nvx_align_plan.h's, the estimate and the taps nvx_align_find.c's.  The library stands
// alone: it shares no state with any other.
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "nvx_companion.h"
#include "nvx_align_plan.h"

extern "C" const char *nvx_align_last_error(void) { return nvx_error_text(); }

static const uint32_t MAGIC = 0x4e414c31u;      // "NAL1"
static const int BPS[4] = { 4, 2, 2, 8 };       // bytes per input sample, by format
static const char *const NOUN = "the row aligner";
static const int SLOTS = 8;                     // delay tables a launch may still be reading

struct nvx_row_aligner {
    uint32_t magic = MAGIC;
    std::mutex mu;
    int device = 0, n_pairs = 0, format = 0, max_delay = 0, min_contrast = 0;
    nvx_state_rows<uint32_t> state;                         // [n_pairs][NVX_ALIGN_STATE_WORDS(max_delay)]
    uint32_t *d_taps = nullptr;                             // [32][8] tap words
    // The delays as the kernels read them: SLOTS tables of n_pairs in pinned host memory.  A launch reads the current one; a
    // delay set since goes into the next, which waits only for the launch that read that slot SLOTS changes ago.
    std::vector<int32_t> delay;
    int32_t *h_slots = nullptr, *d_slots = nullptr;         // the same memory, as the host and as the device name it
    hipEvent_t slot_event[SLOTS] = {};
    bool slot_used[SLOTS] = {};
    int slot = 0;
    bool dirty = true;
    unsigned long long *d_table = nullptr;                  // a measurement's [n_pairs][n_lags][2] and behind it [n_pairs][2]
    size_t table_cap = 0;                                   // in words
    std::vector<uint64_t> consumed;
    nvx_event_timer timer;
    nvx_push_staging push;                                  // a push's two input rows and two output rows, one behind the other
    struct { int chunks, tiles_per_chunk, form; } last = {};
    int64_t kernel_launches = 0;
};

static bool valid(const nvx_row_aligner *c, const char *what)
{
    if (!c || c->magic != MAGIC) { set_error("%s: not a row aligner", what); return false; }
    return true;
}

extern "C" void nvx_align_config_default(nvx_align_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0; cfg->format = NVX_ALIGN_CS16; cfg->n_pairs = 1;
    cfg->max_delay = NVX_ALIGN_MAX_DELAY_DEFAULT; cfg->min_contrast = NVX_ALIGN_MIN_CONTRAST_DEFAULT;
}

// --------------------------------------------------------------------------------------------------------------- plans
static void release(nvx_row_aligner *c)
{
    c->state.release(); (void)hipFree(c->d_taps); (void)hipFree(c->d_table); c->push.release();
    if (c->h_slots) (void)hipHostFree(c->h_slots);
    for (hipEvent_t e : c->slot_event) if (e) (void)hipEventDestroy(e);
    c->timer.destroy();
    c->magic = 0;
    delete c;
}

// Pairs [first, first + n) start anew: nothing but zeros in front of them, in the row their next launch reads.  The caller
// holds the lock, has selected the device and has waited for it.
static int write_fresh_rows(nvx_row_aligner *c, int first, int n)
{
    for (int i = first, j; i < first + n; i = j) {
        j = c->state.run_end(i, first + n);
        HIP_TRY(hipMemset(c->state.row(i), 0, c->state.bytes((size_t)(j - i))));
    }
    HIP_TRY(hipDeviceSynchronize());
    return NVX_OK;
}

extern "C" int nvx_align_create(const nvx_align_config *cfg, nvx_row_aligner **out)
{
    const char *what = "nvx_align_create";
    if (!cfg || !out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    *out = nullptr;
    if (cfg->struct_size != sizeof *cfg) { set_error("%s: struct_size %u, this library's nvx_align_config has %zu bytes", what, cfg->struct_size, sizeof *cfg); return NVX_ERR_ARG; }
    if (cfg->n_pairs < 1 || cfg->n_pairs > 65535) { set_error("%s: n_pairs %d (1 .. 65535)", what, cfg->n_pairs); return NVX_ERR_ARG; }
    if (cfg->format < NVX_ALIGN_CS16 || cfg->format > NVX_ALIGN_CF32) { set_error("%s: format %d (NVX_ALIGN_CS16 .. NVX_ALIGN_CF32)", what, cfg->format); return NVX_ERR_ARG; }
    if (cfg->device < 0) { set_error("%s: device %d", what, cfg->device); return NVX_ERR_ARG; }
    if (cfg->max_delay < 1 || cfg->max_delay > NVX_ALIGN_MAX_DELAY_LIMIT) { set_error("%s: max_delay %d (1 .. 2^20)", what, cfg->max_delay); return NVX_ERR_ARG; }
    if (cfg->min_contrast < 1 || cfg->min_contrast > (1 << 20)) { set_error("%s: min_contrast %d (1 .. 2^20)", what, cfg->min_contrast); return NVX_ERR_ARG; }
    nvx_row_aligner *c = new (std::nothrow) nvx_row_aligner;
    if (!c) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    int rc = select_device(cfg->device, NOUN);
    if (rc != NVX_OK) { release(c); return rc; }
    c->device = cfg->device; c->n_pairs = cfg->n_pairs; c->format = cfg->format; c->max_delay = cfg->max_delay; c->min_contrast = cfg->min_contrast;
    c->consumed.assign(cfg->n_pairs, 0); c->delay.assign(cfg->n_pairs, 0);
    int16_t taps[NVX_ALIGN_PHASES * NVX_ALIGN_TAPS];
    uint32_t words[NVX_ALIGN_PHASES * NVX_ALIGN_TAPS / 2];
    if ((rc = nvx_align_design_taps(taps)) != NVX_OK) { set_error("%s: out of memory", what); release(c); return rc; }
    for (int f = 0; f < NVX_ALIGN_PHASES; f++)
        for (int q = 0; q < NVX_ALIGN_TAPS / 2; q++)
            words[f * 8 + q] = ((uint32_t)(uint16_t)taps[f * 16 + 15 - 2 * q]) | ((uint32_t)(uint16_t)taps[f * 16 + 14 - 2 * q] << 16);
    const size_t slot_bytes = (size_t)SLOTS * cfg->n_pairs * sizeof(int32_t);
    hipError_t e = c->state.allocate(cfg->n_pairs, NVX_ALIGN_STATE_WORDS(cfg->max_delay));
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_taps, sizeof words);
    if (e == hipSuccess) e = hipHostMalloc((void **)&c->h_slots, slot_bytes, hipHostMallocDefault);
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_NOMEM; }
    memset(c->h_slots, 0, slot_bytes);
    e = hipHostGetDevicePointer((void **)&c->d_slots, c->h_slots, 0);
    for (int i = 0; i < SLOTS && e == hipSuccess; i++) e = hipEventCreateWithFlags(&c->slot_event[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemcpy(c->d_taps, words, sizeof words, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(c->state.d[0], 0, c->state.bytes(cfg->n_pairs));
    if (e == hipSuccess) e = hipMemset(c->state.d[1], 0, c->state.bytes(cfg->n_pairs));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: preparing the state failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_HIP; }
    *out = c;
    return NVX_OK;
}

extern "C" void nvx_align_destroy(nvx_row_aligner *c)
{
    if (!c || c->magic != MAGIC) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    release(c);
}

extern "C" int nvx_align_plan(nvx_row_aligner *c, int *format, int *n_pairs, int *max_delay, int *min_contrast)
{
    if (!valid(c, "nvx_align_plan")) return NVX_ERR_ARG;
    if (format) *format = c->format;
    if (n_pairs) *n_pairs = c->n_pairs;
    if (max_delay) *max_delay = c->max_delay;
    if (min_contrast) *min_contrast = c->min_contrast;
    return NVX_OK;
}

// `pair` (-1: all) stands at `position` with nothing in front of it
static int restart(nvx_row_aligner *c, const char *what, int pair, uint64_t position)
{
    if (!row_ok(what, "pair", pair, -1, c->n_pairs)) return NVX_ERR_ARG;
    if (!position_ok(what, position)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const int first = pair < 0 ? 0 : pair, n = pair < 0 ? c->n_pairs : 1;
    if ((rc = write_fresh_rows(c, first, n)) != NVX_OK) return rc;
    for (int i = first; i < first + n; i++) c->consumed[i] = position;
    return NVX_OK;
}

extern "C" int nvx_align_reset(nvx_row_aligner *c, int pair)
{
    return valid(c, "nvx_align_reset") ? restart(c, "nvx_align_reset", pair, 0) : NVX_ERR_ARG;
}

extern "C" int nvx_align_debug_set_position(nvx_row_aligner *c, int pair, uint64_t position)
{
    return valid(c, "nvx_align_debug_set_position") ? restart(c, "nvx_align_debug_set_position", pair, position) : NVX_ERR_ARG;
}

extern "C" int nvx_align_position(nvx_row_aligner *c, int pair, uint64_t *consumed)
{
    const char *what = "nvx_align_position";
    if (!valid(c, what) || !row_ok(what, "pair", pair, 0, c->n_pairs)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (consumed) *consumed = c->consumed[pair];
    return NVX_OK;
}

extern "C" int nvx_align_set_delay(nvx_row_aligner *c, int pair, int delay_q5)
{
    const char *what = "nvx_align_set_delay";
    if (!valid(c, what) || !row_ok(what, "pair", pair, -1, c->n_pairs)) return NVX_ERR_ARG;
    if (delay_q5 < -32 * c->max_delay || delay_q5 > 32 * c->max_delay) {
        set_error("%s: delay_q5 %d: |delay_q5| <= 32 max_delay = %d", what, delay_q5, 32 * c->max_delay);
        return NVX_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    for (int i = pair < 0 ? 0 : pair; i < (pair < 0 ? c->n_pairs : pair + 1); i++) c->delay[i] = delay_q5;
    c->dirty = true;
    return NVX_OK;
}

extern "C" int nvx_align_get_delay(nvx_row_aligner *c, int pair, int *delay_q5)
{
    const char *what = "nvx_align_get_delay";
    if (!valid(c, what) || !row_ok(what, "pair", pair, 0, c->n_pairs)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (delay_q5) *delay_q5 = c->delay[pair];
    return NVX_OK;
}

extern "C" int nvx_align_timing(nvx_row_aligner *c, int enable)
{
    return valid(c, "nvx_align_timing") ? timing_enable(c->mu, c->timer, enable) : NVX_ERR_ARG;
}

extern "C" int nvx_align_time_stats(nvx_row_aligner *c, double *sum_ms, uint64_t *calls, int reset)
{
    return valid(c, "nvx_align_time_stats") ? timing_collect(c->mu, c->timer, sum_ms, calls, reset) : NVX_ERR_ARG;
}

extern "C" int64_t nvx_align_debug_last_launch(nvx_row_aligner *c, int *chunks, int *tiles_per_chunk, int *form)
{
    if (!valid(c, "nvx_align_debug_last_launch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->kernel_launches) {
        if (chunks) *chunks = c->last.chunks;
        if (tiles_per_chunk) *tiles_per_chunk = c->last.tiles_per_chunk;
        if (form) *form = c->last.form;
    }
    return c->kernel_launches;
}

// ------------------------------------------------------------------------------------------------------------ launches
// the delays a launch reads: the current table, or the next one where a delay was set since
static int current_delays(nvx_row_aligner *c)
{
    if (!c->dirty) return NVX_OK;
    const int next = (c->slot + 1) % SLOTS;
    if (c->slot_used[next]) HIP_TRY(hipEventSynchronize(c->slot_event[next]));
    memcpy(c->h_slots + (size_t)next * c->n_pairs, c->delay.data(), (size_t)c->n_pairs * sizeof(int32_t));
    c->slot = next; c->dirty = false;
    return NVX_OK;
}

// One call over pairs [first, first + n) of the plan, which stand at `consumed` and read state row `parity`; the caller
// holds the plan's lock and has checked every span.
static int launch(nvx_row_aligner *c, int first, int n, uint64_t consumed, int parity, const void *d_main, size_t pitch_main, const void *d_sense,
                  size_t pitch_sense, size_t n_in, uint32_t *d_out_main, size_t pitch_out_main, uint32_t *d_out_sense, size_t pitch_out_sense,
                  size_t out_first, hipStream_t s)
{
    int rc;
    if ((rc = current_delays(c)) != NVX_OK) return rc;
    nvx_align_args a;
    const int chunks = nvx_align_fill_args(d_main, pitch_main, d_sense, pitch_sense, n_in, d_out_main, pitch_out_main, d_out_sense, pitch_out_sense, out_first,
                                           n, c->state.in(first, parity), c->state.out(first, parity),
                                           c->d_slots + (size_t)c->slot * c->n_pairs + first, c->d_taps, c->max_delay,
                                           nvx_stream_wanted(n, NVX_ALIGN_TARGET_WORKGROUPS), &a);
    nvx_event_timer::events ev;
    if ((rc = c->timer.begin(s, ev)) != NVX_OK) return rc;
    HIP_TRY(nvx_align_launch(&a, c->format, n, chunks, s));
    c->last = { chunks, a.tiles_per_chunk, chunks > 1 ? 2 : 1 };
    c->kernel_launches += 1;
    if ((rc = c->timer.end(s, ev)) != NVX_OK) return rc;
    HIP_TRY(hipEventRecord(c->slot_event[c->slot], s));
    c->slot_used[c->slot] = true;
    for (int i = first; i < first + n; i++) c->consumed[i] = consumed + n_in;
    c->state.flip(first, n, parity);
    return NVX_OK;
}

// [p, p + bytes) and [q, q + size) have a byte in common
static bool overlap(const void *p, size_t bytes, const void *q, size_t size)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return bytes && size && a < b + size && b < a + bytes;
}

// the two input spans of a call over `rows` pairs, in bytes from each operand's first
static int input_spans(const char *what, size_t rows, size_t bps, const void *d_main, size_t pitch_main, const void *d_sense, size_t pitch_sense, size_t n_in,
                       size_t *main_bytes, size_t *sense_bytes)
{
    if (!span_bytes(rows - 1, pitch_main, n_in, bps, main_bytes) || !span_bytes(rows - 1, pitch_sense, n_in, bps, sense_bytes) ||
        (uintptr_t)d_main + *main_bytes < *main_bytes || (uintptr_t)d_sense + *sense_bytes < *sense_bytes) {
        set_error("%s: the span of %zu samples of %zu pairs at pitch %zu or %zu overflows", what, n_in, rows, pitch_main, pitch_sense);
        return NVX_ERR_ARG;
    }
    if (rows > 1 && (n_in > pitch_main || ((pitch_main * bps) & 15) || n_in > pitch_sense || ((pitch_sense * bps) & 15))) {
        set_error("%s: %zu samples per pair at pitches %zu and %zu (a row must hold them, and input rows are 16-byte aligned)", what, n_in, pitch_main,
                  pitch_sense);
        return NVX_ERR_ARG;
    }
    return NVX_OK;
}

extern "C" int nvx_align_resident(nvx_row_aligner *c, const void *d_main, size_t pitch_main, const void *d_sense, size_t pitch_sense, size_t n_in,
                                  void *d_out_main, size_t pitch_out_main, void *d_out_sense, size_t pitch_out_sense, size_t out_first, void *hip_stream)
{
    const char *what = "nvx_align_resident";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!d_main || !d_sense || !d_out_main || !d_out_sense || ((uintptr_t)d_main & 15) || ((uintptr_t)d_sense & 15) || ((uintptr_t)d_out_main & 3) ||
        ((uintptr_t)d_out_sense & 3) || n_in > NVX_ALIGN_MAX_IN) {
        set_error("%s: bad argument (null pointer, an input not 16-byte aligned, an output not 4-byte aligned, or more than 2^30 samples)", what);
        return NVX_ERR_ARG;
    }
    if (!all_stand_together(what, "pair", c->consumed)) return NVX_ERR_STATE;
    const uint64_t consumed = c->consumed[0];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    const size_t rows = (size_t)c->n_pairs, bps = (size_t)BPS[c->format];
    size_t out_end, main_bytes, sense_bytes, om_bytes, os_bytes;
    int rc;
    if ((rc = input_spans(what, rows, bps, d_main, pitch_main, d_sense, pitch_sense, n_in, &main_bytes, &sense_bytes)) != NVX_OK) return rc;
    if (__builtin_add_overflow(out_first, n_in, &out_end) || !span_bytes(rows - 1, pitch_out_main, out_end, 4, &om_bytes) ||
        !span_bytes(rows - 1, pitch_out_sense, out_end, 4, &os_bytes) || (uintptr_t)d_out_main + om_bytes < om_bytes ||
        (uintptr_t)d_out_sense + os_bytes < os_bytes) {
        set_error("%s: the span of %zu words of %d pairs from %zu at pitch %zu or %zu overflows", what, n_in, c->n_pairs, out_first, pitch_out_main,
                  pitch_out_sense);
        return NVX_ERR_ARG;
    }
    if (rows > 1 && (out_end > pitch_out_main || out_end > pitch_out_sense)) {
        set_error("%s: words up to %zu at pitches %zu and %zu (a row must hold them)", what, out_end, pitch_out_main, pitch_out_sense);
        return NVX_ERR_ARG;
    }
    // the words written, from the first to the last, against both inputs and against each other
    const char *const om_lo = (const char *)d_out_main + out_first * 4, *const os_lo = (const char *)d_out_sense + out_first * 4;
    const size_t om_span = om_bytes - out_first * 4, os_span = os_bytes - out_first * 4;
    if (overlap(om_lo, om_span, d_main, main_bytes) || overlap(om_lo, om_span, d_sense, sense_bytes) || overlap(os_lo, os_span, d_main, main_bytes) ||
        overlap(os_lo, os_span, d_sense, sense_bytes) || overlap(om_lo, om_span, os_lo, os_span)) {
        set_error("%s: an output span (%zu bytes from %p, %zu bytes from %p) overlaps an input span (%zu bytes from %p, %zu bytes from %p) or the other "
                  "output's: a workgroup would read words another has written", what, om_span, (const void *)om_lo, os_span, (const void *)os_lo, main_bytes,
                  d_main, sense_bytes, d_sense);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) return NVX_OK;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_main, main_bytes, what, "main input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_sense, sense_bytes, what, "sense input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out_main, om_bytes, what, "main output")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out_sense, os_bytes, what, "sense output")) != NVX_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    if ((rc = c->state.align(nullptr, s)) != NVX_OK) return rc;
    return launch(c, 0, c->n_pairs, consumed, c->state.parity[0], d_main, pitch_main, d_sense, pitch_sense, n_in, (uint32_t *)d_out_main, pitch_out_main,
                  (uint32_t *)d_out_sense, pitch_out_sense, out_first, s);
}

extern "C" int nvx_align_push(nvx_row_aligner *c, int pair, const void *main_in, const void *sense_in, size_t n_in, int16_t *out_main, int16_t *out_sense)
{
    const char *what = "nvx_align_push";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (pair < 0 || pair >= c->n_pairs || !main_in || !sense_in || !out_main || !out_sense || n_in > NVX_ALIGN_MAX_IN) {
        set_error("%s: bad argument (pair %d of %d, null pointer, or more than 2^30 samples)", what, pair, c->n_pairs);
        return NVX_ERR_ARG;
    }
    const uint64_t consumed = c->consumed[pair];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    // the sense row lies behind the main row, 16-byte aligned; so do the two outputs
    const size_t in_bytes = n_in * (size_t)BPS[c->format], row_bytes = (in_bytes + 15) & ~(size_t)15, out_words = (n_in + 3) & ~(size_t)3;
    if ((rc = c->push.reserve(what, 2 * row_bytes, 2 * out_words)) != NVX_OK) return rc;
    void *const d_sense = (char *)c->push.d_in + row_bytes;
    uint32_t *const d_os = c->push.d_out + out_words;
    HIP_TRY(hipMemcpy(c->push.d_in, main_in, in_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_sense, sense_in, in_bytes, hipMemcpyHostToDevice));
    if ((rc = launch(c, pair, 1, consumed, c->state.parity[pair], c->push.d_in, n_in, d_sense, n_in, n_in, c->push.d_out, n_in, d_os, n_in, 0, nullptr)) != NVX_OK)
        return rc;
    HIP_TRY(hipMemcpy(out_main, c->push.d_out, n_in * 4, hipMemcpyDeviceToHost));     // waits for the null stream
    HIP_TRY(hipMemcpy(out_sense, d_os, n_in * 4, hipMemcpyDeviceToHost));
    return NVX_OK;
}

extern "C" int nvx_align_measure_resident(nvx_row_aligner *c, int format, const void *d_main, size_t pitch_main, const void *d_sense, size_t pitch_sense,
                                          size_t n_in, int lag_first, int n_lags, int64_t *r_out, int64_t *power_out, void *hip_stream)
{
    const char *what = "nvx_align_measure_resident";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!d_main || !d_sense || !r_out || !power_out || ((uintptr_t)d_main & 15) || ((uintptr_t)d_sense & 15) || n_in > NVX_ALIGN_MAX_IN ||
        format < NVX_ALIGN_CS16 || format > NVX_ALIGN_CF32) {
        set_error("%s: bad argument (null pointer, an input not 16-byte aligned, format %d, or more than 2^30 samples)", what, format);
        return NVX_ERR_ARG;
    }
    if (n_lags < 64 || n_lags > NVX_ALIGN_MAX_LAGS || (n_lags & 63)) {
        set_error("%s: n_lags %d (a multiple of 64, 64 .. %d)", what, n_lags, NVX_ALIGN_MAX_LAGS);
        return NVX_ERR_ARG;
    }
    const int64_t lag_last = (int64_t)lag_first + n_lags - 1;
    if (lag_first < -c->max_delay || lag_first > c->max_delay || lag_last < -c->max_delay || lag_last > c->max_delay) {
        set_error("%s: lags %d .. %lld leave +-max_delay = %d", what, lag_first, (long long)lag_last, c->max_delay);
        return NVX_ERR_ARG;
    }
    if (!nvx_align_window(n_in, lag_first, n_lags)) {
        set_error("%s: %zu samples leave a window of fewer than %d for lags %d .. %lld", what, n_in, NVX_ALIGN_MIN_WINDOW, lag_first, (long long)lag_last);
        return NVX_ERR_ARG;
    }
    const size_t rows = (size_t)c->n_pairs;
    size_t main_bytes, sense_bytes;
    int rc;
    if ((rc = input_spans(what, rows, (size_t)BPS[format], d_main, pitch_main, d_sense, pitch_sense, n_in, &main_bytes, &sense_bytes)) != NVX_OK) return rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_main, main_bytes, what, "main input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_sense, sense_bytes, what, "sense input")) != NVX_OK) return rc;
    const size_t table_words = rows * (size_t)n_lags * 2, words = table_words + rows * 2;
    if (words > c->table_cap) {
        HIP_TRY(hipDeviceSynchronize());
        (void)hipFree(c->d_table); c->d_table = nullptr; c->table_cap = 0;
        if (hipMalloc((void **)&c->d_table, words * sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: hipMalloc of %zu table words failed", what, words);
            return NVX_ERR_NOMEM;
        }
        c->table_cap = words;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    nvx_align_measure_args a;
    const int chunks = nvx_align_fill_measure_args(d_main, pitch_main, d_sense, pitch_sense, n_in, lag_first, n_lags, c->n_pairs, c->d_table,
                                                   c->d_table + table_words, &a);
    if (!chunks) { set_error("%s: refused", what); return NVX_ERR_ARG; }
    nvx_event_timer::events ev;
    HIP_TRY(hipMemsetAsync(c->d_table, 0, words * sizeof(unsigned long long), s));
    if ((rc = c->timer.begin(s, ev)) != NVX_OK) return rc;
    HIP_TRY(nvx_align_measure_launch(&a, format, c->n_pairs, chunks, s));
    c->kernel_launches += 1;
    if ((rc = c->timer.end(s, ev)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(r_out, c->d_table, table_words * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(power_out, c->d_table + table_words, rows * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return NVX_OK;
}
