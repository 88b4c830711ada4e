// nvx_spec_host.cpp -- the spectrum monitor's entry points (include/navtex_amd_spec.h): the config checks, the plan with its
// carried positions, rings, surveys and scratch rows, the checks of a call, a push's staging, and the calls that restart a
// survey (reset, measure: both change the host's words only, which reach the device in front of the next call, on its
// stream).  The launch arithmetic is nvx_spec_plan.h's.  The library stands alone: it shares no state with any other.
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "nvx_companion.h"
#include "nvx_spec_plan.h"

extern "C" const char *nvx_spec_last_error(void) { return nvx_error_text(); }

static const uint32_t MAGIC = 0x4e535031u;      // "NSP1"
static const int BPS[4] = { 4, 2, 2, 8 };       // bytes per input sample, by format
static const char *const NOUN = "the spectrum monitor";

struct nvx_spectrum {
    uint32_t magic = MAGIC;
    std::mutex mu;
    int device = 0, n_rows = 0, format = 0, n_log2 = 0, avg = 0;
    uint32_t *d_ring = nullptr;                             // [n_rows][NVX_SPEC_RING_WORDS]
    double *d_survey = nullptr;                             // [n_rows][3][N]
    unsigned long long *d_count = nullptr;                  // [n_rows]
    uint32_t *d_cfg = nullptr;                              // [n_rows][NVX_SPEC_CFG_WORDS]
    double *d_scratch = nullptr;                            // [rows of a launch][lines of a batch][3][N]
    size_t scratch_cap = 0;                                 // in lines of one row
    size_t scratch_bytes = NVX_SPEC_SCRATCH_BYTES;          // a launch's scratch rows stay below this
    std::vector<uint32_t> cfg;                              // what the next call hands over
    std::vector<uint64_t> consumed, from;                   // from: where the row's survey began
    std::vector<uint8_t> restart, silence;                  // the survey starts anew with the next call; the ring is zeroed in front of it
    nvx_event_timer timer;
    nvx_push_staging push;
    struct { int lines, batch_lines, batches, carried; } last = {};
    int64_t kernel_launches = 0;

    int n() const { return 1 << n_log2; }
    size_t ring_words() const { return NVX_SPEC_RING_WORDS(n_log2, avg); }
};

static bool valid(const nvx_spectrum *s, const char *what)
{
    if (!s || s->magic != MAGIC) { set_error("%s: not a spectrum monitor", what); return false; }
    return true;
}

extern "C" void nvx_spec_config_default(nvx_spec_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0; cfg->format = NVX_SPEC_CS16; cfg->n_rows = 1; cfg->n_log2 = NVX_SPEC_LOG2_DEFAULT; cfg->avg = NVX_SPEC_AVG_DEFAULT;
}

// --------------------------------------------------------------------------------------------------------------- plans
static void release(nvx_spectrum *s)
{
    (void)hipFree(s->d_ring); (void)hipFree(s->d_survey); (void)hipFree(s->d_count); (void)hipFree(s->d_cfg); (void)hipFree(s->d_scratch);
    s->push.release();
    s->timer.destroy();
    s->magic = 0;
    delete s;
}

extern "C" int nvx_spec_create(const nvx_spec_config *cfg, nvx_spectrum **out)
{
    const char *what = "nvx_spec_create";
    if (!cfg || !out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    *out = nullptr;
    if (cfg->struct_size != sizeof *cfg) { set_error("%s: struct_size %u, this library's nvx_spec_config has %zu bytes", what, cfg->struct_size, sizeof *cfg); return NVX_ERR_ARG; }
    if (cfg->n_rows < 1 || cfg->n_rows > 65535) { set_error("%s: n_rows %d (1 .. 65535)", what, cfg->n_rows); return NVX_ERR_ARG; }
    if (cfg->n_log2 < NVX_SPEC_LOG2_MIN || cfg->n_log2 > NVX_SPEC_LOG2_MAX) {
        set_error("%s: n_log2 %d (%d .. %d)", what, cfg->n_log2, NVX_SPEC_LOG2_MIN, NVX_SPEC_LOG2_MAX);
        return NVX_ERR_ARG;
    }
    if (cfg->avg < 1 || (int64_t)cfg->avg << (cfg->n_log2 - 1) > NVX_SPEC_MAX_HOP) {
        set_error("%s: avg %d (1 .. %d at n_log2 %d: a line hops by at most %d samples)", what, cfg->avg, NVX_SPEC_MAX_HOP >> (cfg->n_log2 - 1), cfg->n_log2,
                  NVX_SPEC_MAX_HOP);
        return NVX_ERR_ARG;
    }
    if (cfg->format < NVX_SPEC_CS16 || cfg->format > NVX_SPEC_CF32) { set_error("%s: format %d (NVX_SPEC_CS16 .. NVX_SPEC_CF32)", what, cfg->format); return NVX_ERR_ARG; }
    if (cfg->device < 0) { set_error("%s: device %d", what, cfg->device); return NVX_ERR_ARG; }
    nvx_spectrum *s = new (std::nothrow) nvx_spectrum;
    if (!s) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    int rc = select_device(cfg->device, NOUN);
    if (rc != NVX_OK) { release(s); return rc; }
    s->device = cfg->device; s->n_rows = cfg->n_rows; s->format = cfg->format; s->n_log2 = cfg->n_log2; s->avg = cfg->avg;
    const size_t rows = (size_t)cfg->n_rows;
    s->consumed.assign(rows, 0); s->from.assign(rows, 0); s->restart.assign(rows, 1); s->silence.assign(rows, 0);
    s->cfg.assign(rows * NVX_SPEC_CFG_WORDS, 0);
    const size_t ring_bytes = rows * s->ring_words() * sizeof(uint32_t), survey_bytes = rows * NVX_SPEC_SURVEY_WORDS(s->n()) * sizeof(double);
    hipError_t e = hipMalloc((void **)&s->d_ring, ring_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_survey, survey_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_count, rows * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_cfg, s->cfg.size() * sizeof(uint32_t));
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); release(s); return NVX_ERR_NOMEM; }
    e = hipMemset(s->d_ring, 0, ring_bytes);
    if (e == hipSuccess) e = hipMemset(s->d_survey, 0, survey_bytes);
    if (e == hipSuccess) e = hipMemset(s->d_count, 0, rows * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: clearing the state failed: %s", what, hipGetErrorString(e)); release(s); return NVX_ERR_HIP; }
    *out = s;
    return NVX_OK;
}

extern "C" void nvx_spec_destroy(nvx_spectrum *s)
{
    if (!s || s->magic != MAGIC) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    release(s);
}

extern "C" int nvx_spec_plan(nvx_spectrum *s, int *format, int *n_rows, int *n_log2, int *avg)
{
    if (!valid(s, "nvx_spec_plan")) return NVX_ERR_ARG;
    if (format) *format = s->format;
    if (n_rows) *n_rows = s->n_rows;
    if (n_log2) *n_log2 = s->n_log2;
    if (avg) *avg = s->avg;
    return NVX_OK;
}

// `row` (-1: all) stands at `position` with nothing but silence in front of it, from the next call on
static int restart(nvx_spectrum *s, const char *what, int row, uint64_t position)
{
    if (!row_ok(what, "row", row, -1, s->n_rows)) return NVX_ERR_ARG;
    if (!position_ok(what, position)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    for (int i = row < 0 ? 0 : row; i < (row < 0 ? s->n_rows : row + 1); i++) {
        s->consumed[i] = position; s->from[i] = position; s->restart[i] = 1;
        s->silence[i] = position != 0;                      // at position 0 a row reads nothing of its ring
    }
    return NVX_OK;
}

extern "C" int nvx_spec_reset(nvx_spectrum *s, int row)
{
    return valid(s, "nvx_spec_reset") ? restart(s, "nvx_spec_reset", row, 0) : NVX_ERR_ARG;
}

extern "C" int nvx_spec_debug_set_position(nvx_spectrum *s, int row, uint64_t position)
{
    return valid(s, "nvx_spec_debug_set_position") ? restart(s, "nvx_spec_debug_set_position", row, position) : NVX_ERR_ARG;
}

extern "C" int nvx_spec_measure(nvx_spectrum *s, int row)
{
    const char *what = "nvx_spec_measure";
    if (!valid(s, what) || !row_ok(what, "row", row, -1, s->n_rows)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    for (int i = row < 0 ? 0 : row; i < (row < 0 ? s->n_rows : row + 1); i++) { s->from[i] = s->consumed[i]; s->restart[i] = 1; }
    return NVX_OK;
}

extern "C" int nvx_spec_position(nvx_spectrum *s, int row, uint64_t *consumed)
{
    const char *what = "nvx_spec_position";
    if (!valid(s, what) || !row_ok(what, "row", row, 0, s->n_rows)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    if (consumed) *consumed = s->consumed[row];
    return NVX_OK;
}

extern "C" int64_t nvx_spec_lines_for(nvx_spectrum *s, int row, size_t n_in)
{
    const char *what = "nvx_spec_lines_for";
    if (!valid(s, what) || !row_ok(what, "row", row, 0, s->n_rows)) return NVX_ERR_ARG;
    if (n_in > NVX_SPEC_MAX_IN) { set_error("%s: more than 2^30 samples", what); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(s->mu);
    if (!position_ok(what, s->consumed[row] + n_in)) return NVX_ERR_ARG;
    return (int64_t)(nvx_spec_lines_at(s->consumed[row] + n_in, s->n_log2, s->avg) - nvx_spec_lines_at(s->consumed[row], s->n_log2, s->avg));
}

extern "C" int nvx_spec_get(nvx_spectrum *s, int row, double *power, double *lag_re, double *lag_im, uint64_t *lines)
{
    const char *what = "nvx_spec_get";
    if (!valid(s, what) || !row_ok(what, "row", row, 0, s->n_rows)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    const size_t n = (size_t)s->n();
    double *const dst[3] = { power, lag_re, lag_im };
    if (s->restart[row]) {                                  // as the next call will find it: empty
        for (double *d : dst) if (d) memset(d, 0, n * sizeof(double));
        if (lines) *lines = 0;
        return NVX_OK;
    }
    int rc;
    if ((rc = select_device(s->device, NOUN)) != NVX_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    for (int k = 0; k < 3; k++)
        if (dst[k]) HIP_TRY(hipMemcpy(dst[k], s->d_survey + (size_t)row * NVX_SPEC_SURVEY_WORDS(n) + (size_t)k * n, n * sizeof(double), hipMemcpyDeviceToHost));
    unsigned long long count = 0;
    HIP_TRY(hipMemcpy(&count, s->d_count + row, sizeof count, hipMemcpyDeviceToHost));
    if (lines) *lines = count;
    return NVX_OK;
}

extern "C" int nvx_spec_timing(nvx_spectrum *s, int enable)
{
    return valid(s, "nvx_spec_timing") ? timing_enable(s->mu, s->timer, enable) : NVX_ERR_ARG;
}

extern "C" int nvx_spec_time_stats(nvx_spectrum *s, double *sum_ms, uint64_t *calls, int reset)
{
    return valid(s, "nvx_spec_time_stats") ? timing_collect(s->mu, s->timer, sum_ms, calls, reset) : NVX_ERR_ARG;
}

extern "C" int64_t nvx_spec_debug_last_launch(nvx_spectrum *s, int *lines, int *batch_lines, int *batches, int *carried)
{
    if (!valid(s, "nvx_spec_debug_last_launch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->kernel_launches) {
        if (lines) *lines = s->last.lines;
        if (batch_lines) *batch_lines = s->last.batch_lines;
        if (batches) *batches = s->last.batches;
        if (carried) *carried = s->last.carried;
    }
    return s->kernel_launches;
}

extern "C" int nvx_spec_debug_set_scratch(nvx_spectrum *s, size_t bytes)
{
    if (!valid(s, "nvx_spec_debug_set_scratch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    s->scratch_bytes = bytes;
    return NVX_OK;
}

// ------------------------------------------------------------------------------------------------------------ launches
// One call over rows [first, first + rows) of the plan, which stand at `consumed`; the caller holds the plan's lock and has
// checked every span.  Returns the lines completed per row, or an error code.
static int launch(nvx_spectrum *s, int first, int rows, uint64_t consumed, const void *d_in, size_t pitch_in, size_t n_in, uint16_t *d_levels,
                  size_t line_cap, hipStream_t st)
{
    nvx_spec_args a;
    nvx_spec_fill_args(consumed, n_in, s->n_log2, s->avg, &a);
    const size_t n = (size_t)s->n(), line_bytes = (size_t)rows * NVX_SPEC_SURVEY_WORDS(n) * sizeof(double);
    size_t batch = s->scratch_bytes / line_bytes;
    if (batch < 1) batch = 1;
    if (batch > (size_t)a.lines) batch = (size_t)a.lines;
    if (batch * (size_t)rows > s->scratch_cap) {
        HIP_TRY(hipDeviceSynchronize());                    // an earlier call may still use the old rows
        (void)hipFree(s->d_scratch); s->d_scratch = nullptr; s->scratch_cap = 0;
        if (hipMalloc((void **)&s->d_scratch, batch * line_bytes) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: hipMalloc of %zu scratch rows failed", "nvx_spec", batch * (size_t)rows);
            return NVX_ERR_NOMEM;
        }
        s->scratch_cap = batch * (size_t)rows;
    }
    a.in = d_in; a.pitch_in = pitch_in; a.levels = d_levels; a.line_cap = line_cap; a.n_rows = rows;
    a.ring = s->d_ring + (size_t)first * s->ring_words(); a.ring_words = s->ring_words();
    a.scratch = s->d_scratch; a.survey = s->d_survey + (size_t)first * NVX_SPEC_SURVEY_WORDS(n); a.count = s->d_count + first;
    a.cfg = s->d_cfg + (size_t)first * NVX_SPEC_CFG_WORDS;
    // a row set to a position has silence in front of it
    for (int i = first; i < first + rows; i++)
        if (s->silence[i]) {
            HIP_TRY(hipMemsetAsync(s->d_ring + (size_t)i * s->ring_words(), 0, s->ring_words() * sizeof(uint32_t), st));
            s->silence[i] = 0;
        }
    const uint64_t hop = (uint64_t)NVX_SPEC_HOP(s->n_log2, s->avg), line0 = nvx_spec_lines_at(consumed, s->n_log2, s->avg);
    if (a.lines) {
        // the restarts and the lines in front of them: pageable memory, staged by the runtime before it returns
        for (int i = first; i < first + rows; i++) {
            const uint64_t counts_from = (s->from[i] + hop - 1) / hop;           // the first line that begins at or behind the restart
            const uint64_t skip = counts_from > line0 ? counts_from - line0 : 0;
            s->cfg[(size_t)i * NVX_SPEC_CFG_WORDS] = s->restart[i] ? NVX_SPEC_ROW_RESTART : 0u;
            s->cfg[(size_t)i * NVX_SPEC_CFG_WORDS + 1] = (uint32_t)(skip < (uint64_t)a.lines ? skip : (uint64_t)a.lines);
        }
        HIP_TRY(hipMemcpyAsync(s->d_cfg + (size_t)first * NVX_SPEC_CFG_WORDS, s->cfg.data() + (size_t)first * NVX_SPEC_CFG_WORDS,
                               (size_t)rows * NVX_SPEC_CFG_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    nvx_event_timer::events ev;
    int rc;
    if ((rc = s->timer.begin(st, ev)) != NVX_OK) return rc;
    int batches = 0;
    for (int l = 0; l < a.lines; l += (int)batch, batches++) {
        a.line0 = l; a.batch_lines = a.lines - l < (int)batch ? a.lines - l : (int)batch;
        HIP_TRY(nvx_spec_launch_lines(&a, s->format, st));
        s->kernel_launches += 2;
    }
    HIP_TRY(nvx_spec_launch_carry(&a, s->format, st));
    s->kernel_launches += 1;
    s->last = { a.lines, (int)batch, batches, a.carried };
    if ((rc = s->timer.end(st, ev)) != NVX_OK) return rc;
    for (int i = first; i < first + rows; i++) {
        s->consumed[i] = consumed + n_in;
        if (a.lines) s->restart[i] = 0;
    }
    return a.lines;
}

// [p, p + bytes) and [q, q + size) have a byte in common
static bool overlap(const void *p, size_t bytes, const void *q, size_t size)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return bytes && size && a < b + size && b < a + bytes;
}

extern "C" int nvx_spec_resident(nvx_spectrum *s, const void *d_in, size_t pitch_in, size_t n_in, void *d_levels, size_t line_cap, void *hip_stream)
{
    const char *what = "nvx_spec_resident";
    if (!valid(s, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    if (!d_in || ((uintptr_t)d_in & 15) || ((uintptr_t)d_levels & 15) || n_in > NVX_SPEC_MAX_IN) {
        set_error("%s: bad argument (null input, input or level words not 16-byte aligned, or more than 2^30 samples)", what);
        return NVX_ERR_ARG;
    }
    if (!all_stand_together(what, "row", s->consumed)) return NVX_ERR_STATE;
    const uint64_t consumed = s->consumed[0];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    const size_t rows = (size_t)s->n_rows, bps = (size_t)BPS[s->format];
    size_t in_bytes, out_bytes = 0;
    if (!span_bytes(rows - 1, pitch_in, n_in, bps, &in_bytes) || (d_levels && !span_bytes(rows, line_cap, 0, (size_t)s->n() * 2, &out_bytes))) {
        set_error("%s: the span of %zu samples of %d rows at pitch %zu, or of %zu lines of level words per row, overflows", what, n_in, s->n_rows, pitch_in, line_cap);
        return NVX_ERR_ARG;
    }
    if (rows > 1 && (n_in > pitch_in || ((pitch_in * bps) & 15))) {
        set_error("%s: %zu samples per row at pitch %zu (a row must hold them, and input rows are 16-byte aligned)", what, n_in, pitch_in);
        return NVX_ERR_ARG;
    }
    if ((uintptr_t)d_in + in_bytes < in_bytes || (uintptr_t)d_levels + out_bytes < out_bytes) {
        set_error("%s: the span of %zu samples of %d rows at pitch %zu, or of %zu lines of level words per row, wraps", what, n_in, s->n_rows, pitch_in, line_cap);
        return NVX_ERR_ARG;
    }
    if (overlap(d_levels, out_bytes, d_in, in_bytes)) {
        set_error("%s: the level words (%zu bytes from %p) overlap the input span (%zu bytes from %p): a line would be written over samples another reads",
                  what, out_bytes, d_levels, in_bytes, d_in);
        return NVX_ERR_ARG;
    }
    const uint64_t lines = nvx_spec_lines_at(consumed + n_in, s->n_log2, s->avg) - nvx_spec_lines_at(consumed, s->n_log2, s->avg);
    if (d_levels && lines > line_cap) {
        set_error("%s: %zu samples complete %llu lines per row, line_cap is %zu", what, n_in, (unsigned long long)lines, line_cap);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) return 0;
    int rc;
    if ((rc = select_device(s->device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_in, in_bytes, what, "input")) != NVX_OK) return rc;
    if (d_levels && (rc = check_device_span(d_levels, out_bytes, what, "level words")) != NVX_OK) return rc;
    return launch(s, 0, s->n_rows, consumed, d_in, pitch_in, n_in, (uint16_t *)d_levels, line_cap, (hipStream_t)hip_stream);
}

extern "C" int nvx_spec_push(nvx_spectrum *s, int row, const void *in, size_t n_in, uint16_t *levels, size_t line_cap)
{
    const char *what = "nvx_spec_push";
    if (!valid(s, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    if (row < 0 || row >= s->n_rows || !in || n_in > NVX_SPEC_MAX_IN) {
        set_error("%s: bad argument (row %d of %d, null pointer, or more than 2^30 samples)", what, row, s->n_rows);
        return NVX_ERR_ARG;
    }
    const uint64_t consumed = s->consumed[row];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    const uint64_t lines = nvx_spec_lines_at(consumed + n_in, s->n_log2, s->avg) - nvx_spec_lines_at(consumed, s->n_log2, s->avg);
    if (levels && lines > line_cap) {
        set_error("%s: %zu samples complete %llu lines, line_cap is %zu", what, n_in, (unsigned long long)lines, line_cap);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) return 0;
    int rc;
    if ((rc = select_device(s->device, NOUN)) != NVX_OK) return rc;
    const size_t in_bytes = n_in * (size_t)BPS[s->format], level_words = levels ? (size_t)lines * (size_t)s->n() / 2 : 0;      // two to a uint32
    if ((rc = s->push.reserve(what, in_bytes, level_words ? level_words : 1)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(s->push.d_in, in, in_bytes, hipMemcpyHostToDevice));
    if ((rc = launch(s, row, 1, consumed, s->push.d_in, n_in, n_in, levels ? (uint16_t *)s->push.d_out : nullptr, (size_t)lines, nullptr)) < 0) return rc;
    if (level_words) HIP_TRY(hipMemcpy(levels, s->push.d_out, level_words * 4, hipMemcpyDeviceToHost));      // waits for the null stream
    else HIP_TRY(hipStreamSynchronize(nullptr));
    return rc;
}
