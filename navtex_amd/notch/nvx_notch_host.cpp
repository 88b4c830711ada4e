// nvx_notch_host.cpp -- the tone notch's entry points (include/navtex_amd_notch.h): the config checks, the plan with its
// carried positions, state rows, configuration words, block records and table, the checks of a call, a push's staging, and
// the calls that change a notch (set_freq, enable, measure, refine, reset: all of them change the host's configuration words
// only, which reach the device in front of the next call, on its stream).  The launch arithmetic is nvx_notch_plan.h's.  The
// library stands alone: it shares no state with any other.
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "nvx_companion.h"
#include "nvx_notch_plan.h"
#include "nvx_ddc_table.h"

extern "C" const char *nvx_notch_last_error(void) { return nvx_error_text(); }

static const uint32_t MAGIC = 0x4e4e5431u;      // "NNT1"
static const int BPS[4] = { 4, 2, 2, 8 };       // bytes per input sample, by format
static const char *const NOUN = "the tone notch";

struct nvx_tone_notch {
    uint32_t magic = MAGIC;
    std::mutex mu;
    int device = 0, n_rows = 0, format = 0, n_notches = 0, width_log2 = 0;
    nvx_state_rows<int64_t> state;                          // [n_rows][NVX_NOTCH_STATE_WORDS(width_log2, n_notches)]
    std::vector<uint32_t> cfg;                              // [n_rows][NVX_NOTCH_CFG_WORDS(n_notches)]: the host's copy, the master
    uint32_t *d_cfg = nullptr;
    bool cfg_dirty = true;
    uint32_t *d_table = nullptr;                            // [NVX_NOTCH_TABLE]
    unsigned long long *d_records = nullptr;                // [rows of a call][blocks of a call][n_notches][2]
    size_t records_cap = 0;                                 // in records of one notch
    std::vector<uint64_t> consumed, samples;                // samples: since creation
    nvx_event_timer timer;
    nvx_push_staging push;
    struct { int chunks, tiles_per_chunk, records, form; } last = {};
    int64_t kernel_launches = 0;

    int cfg_words() const { return NVX_NOTCH_CFG_WORDS(n_notches); }
    uint32_t &row_flags(int row) { return cfg[(size_t)row * cfg_words()]; }
    uint32_t &step(int row, int notch) { return cfg[(size_t)row * cfg_words() + 2 + 2 * notch]; }
    uint32_t &flags(int row, int notch) { return cfg[(size_t)row * cfg_words() + 3 + 2 * notch]; }
};

static bool valid(const nvx_tone_notch *n, const char *what)
{
    if (!n || n->magic != MAGIC) { set_error("%s: not a tone notch", what); return false; }
    return true;
}

extern "C" void nvx_notch_config_default(nvx_notch_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0; cfg->format = NVX_NOTCH_CS16; cfg->n_rows = 1; cfg->n_notches = 1; cfg->width_log2 = NVX_NOTCH_WIDTH_LOG2_DEFAULT;
}

extern "C" uint32_t nvx_notch_step_from_hz(double hz, double rate)
{
    if (!(rate > 0.0) || !std::isfinite(hz)) return 0;
    const double turns = hz / rate;
    return (uint32_t)(int64_t)std::llrint((turns - std::floor(turns)) * 4294967296.0);
}

extern "C" double nvx_notch_hz_from_step(uint32_t step, double rate) { return (double)(int32_t)step * rate / 4294967296.0; }

// --------------------------------------------------------------------------------------------------------------- plans
static void release(nvx_tone_notch *n)
{
    n->state.release(); (void)hipFree(n->d_cfg); (void)hipFree(n->d_table); (void)hipFree(n->d_records); n->push.release();
    n->timer.destroy();
    n->magic = 0;
    delete n;
}

extern "C" int nvx_notch_create(const nvx_notch_config *cfg, nvx_tone_notch **out)
{
    const char *what = "nvx_notch_create";
    if (!cfg || !out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    *out = nullptr;
    if (cfg->struct_size != sizeof *cfg) { set_error("%s: struct_size %u, this library's nvx_notch_config has %zu bytes", what, cfg->struct_size, sizeof *cfg); return NVX_ERR_ARG; }
    if (cfg->n_rows < 1 || cfg->n_rows > 65535) { set_error("%s: n_rows %d (1 .. 65535)", what, cfg->n_rows); return NVX_ERR_ARG; }
    if (cfg->n_notches < 1 || cfg->n_notches > NVX_NOTCH_MAX_NOTCHES) { set_error("%s: n_notches %d (1 .. %d)", what, cfg->n_notches, NVX_NOTCH_MAX_NOTCHES); return NVX_ERR_ARG; }
    if (cfg->width_log2 < NVX_NOTCH_WIDTH_LOG2_MIN || cfg->width_log2 > NVX_NOTCH_WIDTH_LOG2_MAX) {
        set_error("%s: width_log2 %d (%d .. %d)", what, cfg->width_log2, NVX_NOTCH_WIDTH_LOG2_MIN, NVX_NOTCH_WIDTH_LOG2_MAX);
        return NVX_ERR_ARG;
    }
    if (cfg->format < NVX_NOTCH_CS16 || cfg->format > NVX_NOTCH_CF32) { set_error("%s: format %d (NVX_NOTCH_CS16 .. NVX_NOTCH_CF32)", what, cfg->format); return NVX_ERR_ARG; }
    if (cfg->device < 0) { set_error("%s: device %d", what, cfg->device); return NVX_ERR_ARG; }
    nvx_tone_notch *n = new (std::nothrow) nvx_tone_notch;
    if (!n) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    int rc = select_device(cfg->device, NOUN);
    if (rc != NVX_OK) { release(n); return rc; }
    n->device = cfg->device; n->n_rows = cfg->n_rows; n->format = cfg->format; n->n_notches = cfg->n_notches; n->width_log2 = cfg->width_log2;
    n->consumed.assign(cfg->n_rows, 0); n->samples.assign(cfg->n_rows, 0);
    n->cfg.assign((size_t)cfg->n_rows * n->cfg_words(), 0);
    // the bank's table, packed: c in the low half, s in the high half
    std::vector<uint32_t> table(NVX_NOTCH_TABLE);
    static_assert(NVX_NOTCH_TABLE == NVX_DDC_TAB_N, "the notch's NCO reads the bank's table");
    for (int j = 0; j < NVX_NOTCH_TABLE; j++) {
        int16_t c, s;
        nvx_ddc_w(j, &c, &s);
        table[j] = (uint32_t)(uint16_t)c | ((uint32_t)(uint16_t)s << 16);
    }
    hipError_t e = n->state.allocate(cfg->n_rows, NVX_NOTCH_STATE_WORDS(cfg->width_log2, cfg->n_notches));
    if (e == hipSuccess) e = hipMalloc((void **)&n->d_cfg, n->cfg.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&n->d_table, table.size() * sizeof(uint32_t));
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); release(n); return NVX_ERR_NOMEM; }
    e = hipMemset(n->state.d[0], 0, n->state.bytes(cfg->n_rows));
    if (e == hipSuccess) e = hipMemset(n->state.d[1], 0, n->state.bytes(cfg->n_rows));
    if (e == hipSuccess) e = hipMemcpy(n->d_table, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: clearing the state failed: %s", what, hipGetErrorString(e)); release(n); return NVX_ERR_HIP; }
    *out = n;
    return NVX_OK;
}

extern "C" void nvx_notch_destroy(nvx_tone_notch *n)
{
    if (!n || n->magic != MAGIC) return;
    (void)hipSetDevice(n->device);
    (void)hipDeviceSynchronize();
    release(n);
}

extern "C" int nvx_notch_plan(nvx_tone_notch *n, int *format, int *n_rows, int *n_notches, int *width_log2)
{
    if (!valid(n, "nvx_notch_plan")) return NVX_ERR_ARG;
    if (format) *format = n->format;
    if (n_rows) *n_rows = n->n_rows;
    if (n_notches) *n_notches = n->n_notches;
    if (width_log2) *width_log2 = n->width_log2;
    return NVX_OK;
}

extern "C" int64_t nvx_notch_delay(nvx_tone_notch *n)
{
    return valid(n, "nvx_notch_delay") ? (int64_t)NVX_NOTCH_DELAY(n->width_log2) : (int64_t)NVX_ERR_ARG;
}

// `row` (-1: all) stands at `position` with nothing in front of it, from the next call on
static int restart(nvx_tone_notch *n, const char *what, int row, uint64_t position)
{
    if (!row_ok(what, "row", row, -1, n->n_rows)) return NVX_ERR_ARG;
    if (!position_ok(what, position)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(n->mu);
    for (int i = row < 0 ? 0 : row; i < (row < 0 ? n->n_rows : row + 1); i++) { n->row_flags(i) |= NVX_NOTCH_ROW_RESET; n->consumed[i] = position; }
    n->cfg_dirty = true;
    return NVX_OK;
}

extern "C" int nvx_notch_reset(nvx_tone_notch *n, int row)
{
    return valid(n, "nvx_notch_reset") ? restart(n, "nvx_notch_reset", row, 0) : NVX_ERR_ARG;
}

extern "C" int nvx_notch_debug_set_position(nvx_tone_notch *n, int row, uint64_t position)
{
    return valid(n, "nvx_notch_debug_set_position") ? restart(n, "nvx_notch_debug_set_position", row, position) : NVX_ERR_ARG;
}

extern "C" int nvx_notch_position(nvx_tone_notch *n, int row, uint64_t *consumed)
{
    const char *what = "nvx_notch_position";
    if (!valid(n, what) || !row_ok(what, "row", row, 0, n->n_rows)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(n->mu);
    if (consumed) *consumed = n->consumed[row];
    return NVX_OK;
}

// the flags of `notch` of `row` (-1: all rows): those in `clear` go, those in `set` come; with `step`, that too.  The lock is held.
static void change(nvx_tone_notch *n, int row, int notch, uint32_t clear, uint32_t set, const uint32_t *step)
{
    for (int i = row < 0 ? 0 : row; i < (row < 0 ? n->n_rows : row + 1); i++) {
        n->flags(i, notch) = (n->flags(i, notch) & ~clear) | set;
        if (step) n->step(i, notch) = *step;
    }
    n->cfg_dirty = true;
}

static bool notch_ok(const nvx_tone_notch *n, const char *what, int row, int lowest_row, int notch)
{
    if (!row_ok(what, "row", row, lowest_row, n->n_rows)) return false;
    return row_ok(what, "notch", notch, 0, n->n_notches);
}

extern "C" int nvx_notch_set_freq(nvx_tone_notch *n, int row, int notch, uint32_t step)
{
    const char *what = "nvx_notch_set_freq";
    if (!valid(n, what) || !notch_ok(n, what, row, -1, notch)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(n->mu);
    change(n, row, notch, 0, NVX_NOTCH_RESTART, &step);
    return NVX_OK;
}

extern "C" int nvx_notch_enable(nvx_tone_notch *n, int row, int notch, int enable)
{
    const char *what = "nvx_notch_enable";
    if (!valid(n, what) || !notch_ok(n, what, row, -1, notch)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(n->mu);
    change(n, row, notch, NVX_NOTCH_ENABLED, enable ? NVX_NOTCH_ENABLED : 0, nullptr);
    return NVX_OK;
}

extern "C" int nvx_notch_measure(nvx_tone_notch *n, int row, int notch)
{
    const char *what = "nvx_notch_measure";
    if (!valid(n, what) || !notch_ok(n, what, row, -1, notch)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(n->mu);
    change(n, row, notch, 0, NVX_NOTCH_MEASURE, nullptr);
    return NVX_OK;
}

// X and its count of one notch as the next call will find them; the caller holds the lock
static int read_x(nvx_tone_notch *n, int row, int notch, int64_t *x_re, int64_t *x_im, uint64_t *pairs)
{
    *x_re = *x_im = 0; *pairs = 0;
    if ((n->row_flags(row) & NVX_NOTCH_ROW_RESET) || (n->flags(row, notch) & (NVX_NOTCH_RESTART | NVX_NOTCH_MEASURE))) return NVX_OK;
    int rc;
    if ((rc = select_device(n->device, NOUN)) != NVX_OK) return rc;
    int64_t w[4];
    const int64_t *at = n->state.row(row) + NVX_NOTCH_ROW_SCALARS + (size_t)notch * NVX_NOTCH_NOTCH_WORDS(n->width_log2) +
                        2 * NVX_NOTCH_HIST(n->width_log2) + NVX_NOTCH_ST_X;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(w, at, sizeof w, hipMemcpyDeviceToHost));
    *x_re = w[0]; *x_im = w[1]; *pairs = (uint64_t)w[NVX_NOTCH_ST_PAIRS - NVX_NOTCH_ST_X];
    return NVX_OK;
}

extern "C" int nvx_notch_get(nvx_tone_notch *n, int row, int notch, nvx_notch_status *out)
{
    const char *what = "nvx_notch_get";
    if (!valid(n, what) || !notch_ok(n, what, row, 0, notch)) return NVX_ERR_ARG;
    if (!out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(n->mu);
    memset(out, 0, sizeof *out);
    const int rc = read_x(n, row, notch, &out->x_re, &out->x_im, &out->pairs);
    if (rc != NVX_OK) return rc;
    out->samples = n->samples[row]; out->step = n->step(row, notch); out->enabled = (n->flags(row, notch) & NVX_NOTCH_ENABLED) ? 1 : 0;
    return NVX_OK;
}

extern "C" int nvx_notch_refine(nvx_tone_notch *n, int row, int notch, uint32_t *new_step)
{
    const char *what = "nvx_notch_refine";
    if (!valid(n, what) || !notch_ok(n, what, row, 0, notch)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(n->mu);
    int64_t x_re, x_im; uint64_t pairs;
    const int rc = read_x(n, row, notch, &x_re, &x_im, &pairs);
    if (rc != NVX_OK) return rc;
    uint32_t step = n->step(row, notch);
    if (x_re != 0 || x_im != 0) {
        const double arg = std::atan2((double)x_im, (double)x_re);
        step += (uint32_t)(int64_t)std::llrint(arg * 4294967296.0 / (2.0 * M_PI * NVX_NOTCH_BLOCK));
        change(n, row, notch, 0, NVX_NOTCH_RESTART, &step);
    }
    if (new_step) *new_step = step;
    return NVX_OK;
}

extern "C" int nvx_notch_timing(nvx_tone_notch *n, int enable)
{
    return valid(n, "nvx_notch_timing") ? timing_enable(n->mu, n->timer, enable) : NVX_ERR_ARG;
}

extern "C" int nvx_notch_time_stats(nvx_tone_notch *n, double *sum_ms, uint64_t *calls, int reset)
{
    return valid(n, "nvx_notch_time_stats") ? timing_collect(n->mu, n->timer, sum_ms, calls, reset) : NVX_ERR_ARG;
}

extern "C" int64_t nvx_notch_debug_last_launch(nvx_tone_notch *n, int *chunks, int *tiles_per_chunk, int *records, int *form)
{
    if (!valid(n, "nvx_notch_debug_last_launch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(n->mu);
    if (n->kernel_launches) {
        if (chunks) *chunks = n->last.chunks;
        if (tiles_per_chunk) *tiles_per_chunk = n->last.tiles_per_chunk;
        if (records) *records = n->last.records;
        if (form) *form = n->last.form;
    }
    return n->kernel_launches;
}

// ------------------------------------------------------------------------------------------------------------ launches
// One call over rows [first, first + rows) of the plan, which stand at `consumed` and read state row `parity`; the caller
// holds the plan's lock and has checked every span.
static int launch(nvx_tone_notch *n, int first, int rows, uint64_t consumed, int parity, const void *d_in, size_t pitch_in, size_t n_in, uint32_t *d_out,
                  size_t pitch_out, size_t out_first, hipStream_t s)
{
    const int wanted = nvx_stream_wanted(rows, NVX_NOTCH_TARGET_WORKGROUPS);
    nvx_notch_args a;
    int chunks = nvx_notch_fill_args(consumed, d_in, pitch_in, n_in, d_out, pitch_out, out_first, rows, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     n->n_notches, n->width_log2, wanted, &a);
    const size_t records = (size_t)rows * (size_t)a.blocks, record_bytes = (size_t)n->n_notches * 2 * sizeof(unsigned long long);
    if (records > n->records_cap) {
        HIP_TRY(hipDeviceSynchronize());                    // an earlier call may still use the old ones
        (void)hipFree(n->d_records); n->d_records = nullptr; n->records_cap = 0;
        if (hipMalloc((void **)&n->d_records, records * record_bytes) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: hipMalloc of %zu block records failed", "nvx_notch", records);
            return NVX_ERR_NOMEM;
        }
        n->records_cap = records;
    }
    const size_t cw = (size_t)n->cfg_words();
    chunks = nvx_notch_fill_args(consumed, d_in, pitch_in, n_in, d_out, pitch_out, out_first, rows, n->state.in(first, parity), n->state.out(first, parity),
                                 n->d_cfg + (size_t)first * cw, n->d_table, n->d_records, n->n_notches, n->width_log2, wanted, &a);
    // the steps and flags, where they changed since the last call: pageable memory, staged by the runtime before it returns
    if (n->cfg_dirty) {
        HIP_TRY(hipMemcpyAsync(n->d_cfg, n->cfg.data(), n->cfg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        n->cfg_dirty = false;
    }
    nvx_event_timer::events ev;
    int rc;
    if ((rc = n->timer.begin(s, ev)) != NVX_OK) return rc;
    // a call that starts inside a block adds to the records from several waves; one that starts on a block's first sample writes each once
    if (a.off0) HIP_TRY(hipMemsetAsync(n->d_records, 0, records * record_bytes, s));
    HIP_TRY(nvx_notch_launch(&a, n->format, rows, chunks, s));
    n->last = { chunks, a.tiles_per_chunk, a.blocks, chunks > 1 ? 2 : 1 };
    n->kernel_launches += 3;
    if ((rc = n->timer.end(s, ev)) != NVX_OK) return rc;
    for (int i = first; i < first + rows; i++) {
        n->consumed[i] = consumed + n_in; n->samples[i] += n_in;
        // what held for this call only
        if (n->row_flags(i) & NVX_NOTCH_ROW_RESET) { n->row_flags(i) &= ~NVX_NOTCH_ROW_RESET; n->cfg_dirty = true; }
        for (int k = 0; k < n->n_notches; k++)
            if (n->flags(i, k) & (NVX_NOTCH_RESTART | NVX_NOTCH_MEASURE)) { n->flags(i, k) &= ~(NVX_NOTCH_RESTART | NVX_NOTCH_MEASURE); n->cfg_dirty = true; }
    }
    n->state.flip(first, rows, parity);
    return NVX_OK;
}

// [p, p + bytes) and [q, q + size) have a byte in common
static bool overlap(const void *p, size_t bytes, const void *q, size_t size)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return bytes && size && a < b + size && b < a + bytes;
}

extern "C" int nvx_notch_resident(nvx_tone_notch *n, const void *d_in, size_t pitch_in, size_t n_in, void *d_out, size_t pitch_out, size_t out_first,
                                  void *hip_stream)
{
    const char *what = "nvx_notch_resident";
    if (!valid(n, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(n->mu);
    if (!d_in || !d_out || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 3) || n_in > NVX_NOTCH_MAX_IN) {
        set_error("%s: bad argument (null pointer, input not 16-byte aligned, output not 4-byte aligned, or more than 2^30 samples)", what);
        return NVX_ERR_ARG;
    }
    if (!all_stand_together(what, "row", n->consumed)) return NVX_ERR_STATE;
    const uint64_t consumed = n->consumed[0];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    size_t in_bytes, out_bytes;
    int rc;
    if ((rc = resident_spans(what, n->n_rows, (size_t)BPS[n->format], n_in, pitch_in, n_in, "as many", pitch_out, out_first, &in_bytes, &out_bytes)) != NVX_OK)
        return rc;
    if ((uintptr_t)d_in + in_bytes < in_bytes || (uintptr_t)d_out + out_bytes < out_bytes) {
        set_error("%s: the span of %zu samples of %d rows at pitch %zu, or of as many words from %zu at pitch %zu, wraps", what, n_in, n->n_rows, pitch_in,
                  out_first, pitch_out);
        return NVX_ERR_ARG;
    }
    // the words written, from the first to the last, against the input
    const char *const out_lo = (const char *)d_out + out_first * 4;
    const size_t out_span = out_bytes - out_first * 4;
    if (overlap(out_lo, out_span, d_in, in_bytes)) {
        set_error("%s: the output span (%zu bytes from %p) overlaps the input span (%zu bytes from %p): the second pass would read words the first has not "
                  "seen", what, out_span, (const void *)out_lo, in_bytes, d_in);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) return NVX_OK;
    if ((rc = select_device(n->device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_in, in_bytes, what, "input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out, out_bytes, what, "output")) != NVX_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    // a row that starts anew with this call reads nothing of its state row
    std::vector<uint8_t> skip(n->n_rows);
    for (int i = 0; i < n->n_rows; i++) skip[i] = (n->row_flags(i) & NVX_NOTCH_ROW_RESET) ? 1 : 0;
    if ((rc = n->state.align(skip.data(), s)) != NVX_OK) return rc;
    return launch(n, 0, n->n_rows, consumed, n->state.parity[0], d_in, pitch_in, n_in, (uint32_t *)d_out, pitch_out, out_first, s);
}

extern "C" int nvx_notch_push(nvx_tone_notch *n, int row, const void *in, size_t n_in, int16_t *out_iq)
{
    const char *what = "nvx_notch_push";
    if (!valid(n, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(n->mu);
    if (row < 0 || row >= n->n_rows || !in || !out_iq || n_in > NVX_NOTCH_MAX_IN) {
        set_error("%s: bad argument (row %d of %d, null pointer, or more than 2^30 samples)", what, row, n->n_rows);
        return NVX_ERR_ARG;
    }
    const uint64_t consumed = n->consumed[row];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(n->device, NOUN)) != NVX_OK) return rc;
    const size_t in_bytes = n_in * (size_t)BPS[n->format];
    if ((rc = n->push.reserve(what, in_bytes, n_in)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(n->push.d_in, in, in_bytes, hipMemcpyHostToDevice));
    if ((rc = launch(n, row, 1, consumed, n->state.parity[row], n->push.d_in, n_in, n_in, n->push.d_out, n_in, 0, nullptr)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(out_iq, n->push.d_out, n_in * 4, hipMemcpyDeviceToHost));      // waits for the null stream
    return NVX_OK;
}
