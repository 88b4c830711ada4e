// nvx_div_host.cpp -- the diversity combiner's entry points (include/navtex_amd_div.h): the config checks, the plan with its
// carried positions, state rows, configuration words, block records, weight lists, counters and table, the checks of a call,
// a push's staging, and the calls that change a target (set_freq, set, set_mode, reset: all of them change the host's
// configuration words only, which reach the device in front of the next call, on its stream).  The launch arithmetic is
// nvx_div_plan.h's.  The library stands alone: it shares no state with any other.
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "nvx_companion.h"
#include "nvx_div_plan.h"
#include "nvx_ddc_table.h"

extern "C" const char *nvx_div_last_error(void) { return nvx_error_text(); }

static const uint32_t MAGIC = 0x4e445631u;      // "NDV1"
static const int BPS[4] = { 4, 2, 2, 8 };       // bytes per input sample, by format
static const char *const NOUN = "the diversity combiner";

struct nvx_diversity_combiner {
    uint32_t magic = MAGIC;
    std::mutex mu;
    int device = 0, n_pairs = 0, n_targets = 0, format = 0, window_log2 = 0;
    nvx_state_rows<int64_t> state;                          // [n_pairs][n_targets * NVX_DIV_STATE_WORDS(window_log2)]
    std::vector<uint32_t> cfg;                              // [n_pairs][NVX_DIV_CFG_WORDS(n_targets)]
    bool cfg_dirty = true;
    uint32_t *d_cfg = nullptr;
    uint32_t *d_table = nullptr;                            // [NVX_DIV_TABLE]
    unsigned long long *d_counters = nullptr;               // [n_pairs][n_targets][2]: cells solved, cells rejected
    unsigned long long *d_records = nullptr;                // [pairs of a call][blocks of a call][n_targets][NVX_DIV_SUMS]
    size_t records_cap = 0;                                 // in records of one target
    nvx_div_weight *d_weights = nullptr;                    // [pairs of a call][cells of a call][n_targets]
    size_t weights_cap = 0;                                 // in entries of one target
    std::vector<uint64_t> consumed, samples;                // samples: since creation
    nvx_event_timer timer;
    nvx_push_staging push;                                  // a push's two input rows, one behind the other, and its output rows
    struct { int chunks, tiles_per_chunk, records, form; } last = {};
    int64_t kernel_launches = 0;

    int cfg_words() const { return NVX_DIV_CFG_WORDS(n_targets); }
    uint32_t &pair_flags(int pair) { return cfg[(size_t)pair * cfg_words()]; }
    uint32_t *target(int pair, int t) { return cfg.data() + (size_t)pair * cfg_words() + 2 + NVX_DIV_CFG_TARGET * t; }
    // the target starts anew with the next call: nothing of its state row counts
    bool fresh(int pair, int t) { return (pair_flags(pair) & NVX_DIV_PAIR_RESET) || (target(pair, t)[NVX_DIV_CFG_FLAGS] & NVX_DIV_RESTART); }
};

static bool valid(const nvx_diversity_combiner *c, const char *what)
{
    if (!c || c->magic != MAGIC) { set_error("%s: not a diversity combiner", what); return false; }
    return true;
}

extern "C" void nvx_div_config_default(nvx_div_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0; cfg->format = NVX_DIV_CS16; cfg->n_pairs = 1; cfg->n_targets = 1; cfg->window_log2 = NVX_DIV_WINDOW_LOG2_DEFAULT;
}

extern "C" uint32_t nvx_div_step_from_hz(double hz, double rate)
{
    if (!(rate > 0.0) || !std::isfinite(hz)) return 0;
    const double turns = hz / rate;
    return (uint32_t)(int64_t)std::llrint((turns - std::floor(turns)) * 4294967296.0);
}

extern "C" double nvx_div_hz_from_step(uint32_t step, double rate) { return (double)(int32_t)step * rate / 4294967296.0; }

// --------------------------------------------------------------------------------------------------------------- plans
static void release(nvx_diversity_combiner *c)
{
    c->state.release(); (void)hipFree(c->d_cfg); (void)hipFree(c->d_table); (void)hipFree(c->d_counters); (void)hipFree(c->d_records);
    (void)hipFree(c->d_weights); c->push.release();
    c->timer.destroy();
    c->magic = 0;
    delete c;
}

extern "C" int nvx_div_create(const nvx_div_config *cfg, nvx_diversity_combiner **out)
{
    const char *what = "nvx_div_create";
    if (!cfg || !out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    *out = nullptr;
    if (cfg->struct_size != sizeof *cfg) { set_error("%s: struct_size %u, this library's nvx_div_config has %zu bytes", what, cfg->struct_size, sizeof *cfg); return NVX_ERR_ARG; }
    if (cfg->n_pairs < 1 || cfg->n_pairs > 65535) { set_error("%s: n_pairs %d (1 .. 65535)", what, cfg->n_pairs); return NVX_ERR_ARG; }
    if (cfg->n_targets < 1 || cfg->n_targets > NVX_DIV_MAX_TARGETS) { set_error("%s: n_targets %d (1 .. %d)", what, cfg->n_targets, NVX_DIV_MAX_TARGETS); return NVX_ERR_ARG; }
    if (cfg->format < NVX_DIV_CS16 || cfg->format > NVX_DIV_CF32) { set_error("%s: format %d (NVX_DIV_CS16 .. NVX_DIV_CF32)", what, cfg->format); return NVX_ERR_ARG; }
    if (cfg->device < 0) { set_error("%s: device %d", what, cfg->device); return NVX_ERR_ARG; }
    if (cfg->window_log2 != 0 && cfg->window_log2 != 1 && cfg->window_log2 != 2 && cfg->window_log2 != 4) {
        set_error("%s: window_log2 %d (0, 1, 2 or 4)", what, cfg->window_log2);
        return NVX_ERR_ARG;
    }
    nvx_diversity_combiner *c = new (std::nothrow) nvx_diversity_combiner;
    if (!c) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    int rc = select_device(cfg->device, NOUN);
    if (rc != NVX_OK) { release(c); return rc; }
    c->device = cfg->device; c->n_pairs = cfg->n_pairs; c->n_targets = cfg->n_targets; c->format = cfg->format; c->window_log2 = cfg->window_log2;
    c->consumed.assign(cfg->n_pairs, 0); c->samples.assign(cfg->n_pairs, 0);
    // every pair starts as after a reset: its state rows are not read before they are written
    c->cfg.assign((size_t)cfg->n_pairs * c->cfg_words(), 0);
    for (int i = 0; i < cfg->n_pairs; i++) c->pair_flags(i) = NVX_DIV_PAIR_RESET;
    // the bank's table, packed: c in the low half, s in the high half
    std::vector<uint32_t> table(NVX_DIV_TABLE);
    static_assert(NVX_DIV_TABLE == NVX_DDC_TAB_N, "the combiner's NCO reads the bank's table");
    for (int j = 0; j < NVX_DIV_TABLE; j++) {
        int16_t cs, sn;
        nvx_ddc_w(j, &cs, &sn);
        table[j] = (uint32_t)(uint16_t)cs | ((uint32_t)(uint16_t)sn << 16);
    }
    const size_t counter_bytes = (size_t)cfg->n_pairs * cfg->n_targets * 2 * sizeof(unsigned long long);
    hipError_t e = c->state.allocate(cfg->n_pairs, (size_t)cfg->n_targets * NVX_DIV_STATE_WORDS(cfg->window_log2));
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_cfg, c->cfg.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_table, table.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_counters, counter_bytes);
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_NOMEM; }
    e = hipMemset(c->state.d[0], 0, c->state.bytes(cfg->n_pairs));
    if (e == hipSuccess) e = hipMemset(c->state.d[1], 0, c->state.bytes(cfg->n_pairs));
    if (e == hipSuccess) e = hipMemset(c->d_counters, 0, counter_bytes);
    if (e == hipSuccess) e = hipMemcpy(c->d_table, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: clearing the state failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_HIP; }
    *out = c;
    return NVX_OK;
}

extern "C" void nvx_div_destroy(nvx_diversity_combiner *c)
{
    if (!c || c->magic != MAGIC) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    release(c);
}

extern "C" int nvx_div_plan(nvx_diversity_combiner *c, int *format, int *n_pairs, int *n_targets, int *window_log2)
{
    if (!valid(c, "nvx_div_plan")) return NVX_ERR_ARG;
    if (format) *format = c->format;
    if (n_pairs) *n_pairs = c->n_pairs;
    if (n_targets) *n_targets = c->n_targets;
    if (window_log2) *window_log2 = c->window_log2;
    return NVX_OK;
}

// `pair` (-1: all) stands at `position` with nothing in front of it, from the next call on; weights set and not yet applied go
static int restart(nvx_diversity_combiner *c, const char *what, int pair, uint64_t position)
{
    if (!row_ok(what, "pair", pair, -1, c->n_pairs)) return NVX_ERR_ARG;
    if (!position_ok(what, position)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    for (int i = pair < 0 ? 0 : pair; i < (pair < 0 ? c->n_pairs : pair + 1); i++) {
        c->pair_flags(i) |= NVX_DIV_PAIR_RESET; c->consumed[i] = position;
        for (int t = 0; t < c->n_targets; t++) c->target(i, t)[NVX_DIV_CFG_FLAGS] &= ~NVX_DIV_SET;
    }
    c->cfg_dirty = true;
    return NVX_OK;
}

extern "C" int nvx_div_reset(nvx_diversity_combiner *c, int pair)
{
    return valid(c, "nvx_div_reset") ? restart(c, "nvx_div_reset", pair, 0) : NVX_ERR_ARG;
}

extern "C" int nvx_div_debug_set_position(nvx_diversity_combiner *c, int pair, uint64_t position)
{
    return valid(c, "nvx_div_debug_set_position") ? restart(c, "nvx_div_debug_set_position", pair, position) : NVX_ERR_ARG;
}

extern "C" int nvx_div_position(nvx_diversity_combiner *c, int pair, uint64_t *consumed)
{
    const char *what = "nvx_div_position";
    if (!valid(c, what) || !row_ok(what, "pair", pair, 0, c->n_pairs)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (consumed) *consumed = c->consumed[pair];
    return NVX_OK;
}

static bool target_ok(const nvx_diversity_combiner *c, const char *what, int pair, int lowest_pair, int target)
{
    if (!row_ok(what, "pair", pair, lowest_pair, c->n_pairs)) return false;
    return row_ok(what, "target", target, 0, c->n_targets);
}

extern "C" int nvx_div_set_freq(nvx_diversity_combiner *c, int pair, int target, uint32_t step)
{
    const char *what = "nvx_div_set_freq";
    if (!valid(c, what) || !target_ok(c, what, pair, -1, target)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    for (int i = pair < 0 ? 0 : pair; i < (pair < 0 ? c->n_pairs : pair + 1); i++) {
        uint32_t *const t = c->target(i, target);
        t[NVX_DIV_CFG_STEP] = step;
        t[NVX_DIV_CFG_FLAGS] = (t[NVX_DIV_CFG_FLAGS] & ~NVX_DIV_SET) | NVX_DIV_RESTART;
    }
    c->cfg_dirty = true;
    return NVX_OK;
}

extern "C" int nvx_div_set(nvx_diversity_combiner *c, int pair, int target, int lead, int w_re, int w_im)
{
    const char *what = "nvx_div_set";
    if (!valid(c, what) || !target_ok(c, what, pair, -1, target)) return NVX_ERR_ARG;
    if ((lead != 0 && lead != 1) || w_re < -NVX_DIV_W_MAX || w_re > NVX_DIV_W_MAX || w_im < -NVX_DIV_W_MAX || w_im > NVX_DIV_W_MAX) {
        set_error("%s: lead %d, (%d, %d): lead 0 or 1, |w_re|, |w_im| <= %d", what, lead, w_re, w_im, NVX_DIV_W_MAX);
        return NVX_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    for (int i = pair < 0 ? 0 : pair; i < (pair < 0 ? c->n_pairs : pair + 1); i++) {
        uint32_t *const t = c->target(i, target);
        t[NVX_DIV_CFG_LEAD] = (uint32_t)lead; t[NVX_DIV_CFG_WRE] = (uint32_t)w_re; t[NVX_DIV_CFG_WIM] = (uint32_t)w_im;
        t[NVX_DIV_CFG_FLAGS] |= NVX_DIV_SET;
    }
    c->cfg_dirty = true;
    return NVX_OK;
}

extern "C" int nvx_div_set_mode(nvx_diversity_combiner *c, int pair, int target, int mode)
{
    const char *what = "nvx_div_set_mode";
    if (!valid(c, what) || !target_ok(c, what, pair, -1, target)) return NVX_ERR_ARG;
    if (mode != NVX_DIV_TRACK && mode != NVX_DIV_HOLD) { set_error("%s: mode %d (NVX_DIV_TRACK or NVX_DIV_HOLD)", what, mode); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    for (int i = pair < 0 ? 0 : pair; i < (pair < 0 ? c->n_pairs : pair + 1); i++) {
        uint32_t *const t = c->target(i, target);
        t[NVX_DIV_CFG_FLAGS] = (t[NVX_DIV_CFG_FLAGS] & ~NVX_DIV_HELD) | (mode == NVX_DIV_HOLD ? NVX_DIV_HELD : 0u);
    }
    c->cfg_dirty = true;
    return NVX_OK;
}

extern "C" int nvx_div_get(nvx_diversity_combiner *c, int pair, int target, nvx_div_status *out)
{
    const char *what = "nvx_div_get";
    if (!valid(c, what) || !target_ok(c, what, pair, 0, target)) return NVX_ERR_ARG;
    if (!out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    const size_t sw = NVX_DIV_STATE_WORDS(c->window_log2);
    std::vector<int64_t> row(sw, 0);
    unsigned long long counters[2] = { 0, 0 };
    HIP_TRY(hipDeviceSynchronize());
    // a target that starts anew with the next call is what that call will find: empty
    if (!c->fresh(pair, target)) HIP_TRY(hipMemcpy(row.data(), c->state.row(pair) + (size_t)target * sw, sw * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counters, c->d_counters + 2 * ((size_t)pair * c->n_targets + target), sizeof counters, hipMemcpyDeviceToHost));
    const int W = 1 << c->window_log2;
    const int64_t *sc = row.data() + NVX_DIV_SUMS * W + 2 * NVX_DIV_SUMS;
    const uint32_t *t = c->target(pair, target);
    memset(out, 0, sizeof *out);
    out->lead = (int32_t)sc[NVX_DIV_ST_LEAD]; out->w_re = (int32_t)sc[NVX_DIV_ST_WRE]; out->w_im = (int32_t)sc[NVX_DIV_ST_WIM];
    if (t[NVX_DIV_CFG_FLAGS] & NVX_DIV_SET) { out->lead = (int32_t)t[NVX_DIV_CFG_LEAD]; out->w_re = (int32_t)t[NVX_DIV_CFG_WRE]; out->w_im = (int32_t)t[NVX_DIV_CFG_WIM]; }
    out->mode = (t[NVX_DIV_CFG_FLAGS] & NVX_DIV_HELD) ? NVX_DIV_HOLD : NVX_DIV_TRACK;
    out->last_reason = (int32_t)sc[NVX_DIV_ST_REASON]; out->coherence_q14 = (int32_t)sc[NVX_DIV_ST_COHERENCE];
    for (int b = 0; b < W; b++)                             // cells not complete since the restart are zero
        for (int k = 0; k < NVX_DIV_SUMS; k++) out->sums[k] += row[(size_t)b * NVX_DIV_SUMS + k];
    out->step = t[NVX_DIV_CFG_STEP];
    out->samples = c->samples[pair]; out->cells_solved = counters[0]; out->cells_rejected = counters[1];
    return NVX_OK;
}

extern "C" int nvx_div_timing(nvx_diversity_combiner *c, int enable)
{
    return valid(c, "nvx_div_timing") ? timing_enable(c->mu, c->timer, enable) : NVX_ERR_ARG;
}

extern "C" int nvx_div_time_stats(nvx_diversity_combiner *c, double *sum_ms, uint64_t *calls, int reset)
{
    return valid(c, "nvx_div_time_stats") ? timing_collect(c->mu, c->timer, sum_ms, calls, reset) : NVX_ERR_ARG;
}

extern "C" int64_t nvx_div_debug_last_launch(nvx_diversity_combiner *c, int *chunks, int *tiles_per_chunk, int *records, int *form)
{
    if (!valid(c, "nvx_div_debug_last_launch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->kernel_launches) {
        if (chunks) *chunks = c->last.chunks;
        if (tiles_per_chunk) *tiles_per_chunk = c->last.tiles_per_chunk;
        if (records) *records = c->last.records;
        if (form) *form = c->last.form;
    }
    return c->kernel_launches;
}

// ------------------------------------------------------------------------------------------------------------ launches
// a device buffer of `units` units of `unit_bytes` grows to hold them; an earlier call may still use the old one
template <typename T> static int grow(const char *what, T **p, size_t *cap, size_t units, size_t unit_bytes)
{
    if (units <= *cap) return NVX_OK;
    HIP_TRY(hipDeviceSynchronize());
    (void)hipFree(*p); *p = nullptr; *cap = 0;
    if (hipMalloc((void **)p, units * unit_bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("nvx_div: hipMalloc of %zu %s failed", units, what);
        return NVX_ERR_NOMEM;
    }
    *cap = units;
    return NVX_OK;
}

// One call over pairs [first, first + n) of the plan, which stand at `consumed` and read state row `parity`; the caller
// holds the plan's lock and has checked every span.
static int launch(nvx_diversity_combiner *c, int first, int n, uint64_t consumed, int parity, const void *d_main, size_t pitch_main, const void *d_second,
                  size_t pitch_second, size_t n_in, uint32_t *d_out, size_t pitch_out, size_t out_first, hipStream_t s)
{
    const int wanted = nvx_stream_wanted(n, NVX_DIV_TARGET_WORKGROUPS), K = c->n_targets;
    nvx_div_args a;
    int chunks = nvx_div_fill_args(consumed, d_main, pitch_main, d_second, pitch_second, n_in, d_out, pitch_out, out_first, n, K, nullptr, nullptr, nullptr,
                                   nullptr, nullptr, nullptr, nullptr, c->window_log2, wanted, &a);
    const size_t records = (size_t)n * (size_t)a.blocks, record_bytes = (size_t)K * NVX_DIV_SUMS * sizeof(unsigned long long);
    const size_t weights = (size_t)n * (size_t)a.cells;
    int rc;
    if ((rc = grow("block records", &c->d_records, &c->records_cap, records, record_bytes)) != NVX_OK) return rc;
    if ((rc = grow("cell weights", &c->d_weights, &c->weights_cap, weights, (size_t)K * sizeof(nvx_div_weight))) != NVX_OK) return rc;
    const size_t cw = (size_t)c->cfg_words();
    chunks = nvx_div_fill_args(consumed, d_main, pitch_main, d_second, pitch_second, n_in, d_out, pitch_out, out_first, n, K, c->state.in(first, parity),
                               c->state.out(first, parity), c->d_cfg + (size_t)first * cw, c->d_table, c->d_records, c->d_weights,
                               c->d_counters + 2 * (size_t)first * K, c->window_log2, wanted, &a);
    // the steps and flags, where they changed since the last call: pageable memory, staged by the runtime before it returns
    if (c->cfg_dirty) {
        HIP_TRY(hipMemcpyAsync(c->d_cfg, c->cfg.data(), c->cfg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        c->cfg_dirty = false;
    }
    nvx_event_timer::events ev;
    if ((rc = c->timer.begin(s, ev)) != NVX_OK) return rc;
    // a call that starts inside a block adds to the records from several waves; one that starts on a block's first sample writes each once
    if (a.off0) HIP_TRY(hipMemsetAsync(c->d_records, 0, records * record_bytes, s));
    HIP_TRY(nvx_div_launch(&a, c->format, n, chunks, s));
    c->last = { chunks, a.tiles_per_chunk, a.blocks, chunks > 1 ? 2 : 1 };
    c->kernel_launches += 3;
    if ((rc = c->timer.end(s, ev)) != NVX_OK) return rc;
    for (int i = first; i < first + n; i++) {
        c->consumed[i] = consumed + n_in; c->samples[i] += n_in;
        // what held for this call only
        if (c->pair_flags(i) & NVX_DIV_PAIR_RESET) { c->pair_flags(i) &= ~NVX_DIV_PAIR_RESET; c->cfg_dirty = true; }
        for (int t = 0; t < K; t++) {
            uint32_t &f = c->target(i, t)[NVX_DIV_CFG_FLAGS];
            if (f & (NVX_DIV_RESTART | NVX_DIV_SET)) { f &= ~(NVX_DIV_RESTART | NVX_DIV_SET); c->cfg_dirty = true; }
        }
    }
    c->state.flip(first, n, parity);
    return NVX_OK;
}

// [p, p + bytes) and [q, q + size) have a byte in common
static bool overlap(const void *p, size_t bytes, const void *q, size_t size)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return bytes && size && a < b + size && b < a + bytes;
}

extern "C" int nvx_div_resident(nvx_diversity_combiner *c, const void *d_main, size_t pitch_main, const void *d_second, size_t pitch_second, size_t n_in,
                                void *d_out, size_t pitch_out, size_t out_first, void *hip_stream)
{
    const char *what = "nvx_div_resident";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!d_main || !d_second || !d_out || ((uintptr_t)d_main & 15) || ((uintptr_t)d_second & 15) || ((uintptr_t)d_out & 3) || n_in > NVX_DIV_MAX_IN) {
        set_error("%s: bad argument (null pointer, an input not 16-byte aligned, output not 4-byte aligned, or more than 2^30 samples)", what);
        return NVX_ERR_ARG;
    }
    if (!all_stand_together(what, "pair", c->consumed)) return NVX_ERR_STATE;
    const uint64_t consumed = c->consumed[0];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    // every row's last sample read and last word written, in samples of its row (out_end) and in bytes of the whole operand
    const size_t rows = (size_t)c->n_pairs, out_rows = rows * (size_t)c->n_targets, bps = (size_t)BPS[c->format];
    size_t out_end, main_bytes, second_bytes, out_bytes;
    if (__builtin_add_overflow(out_first, n_in, &out_end) || !span_bytes(rows - 1, pitch_main, n_in, bps, &main_bytes) ||
        !span_bytes(rows - 1, pitch_second, n_in, bps, &second_bytes) || !span_bytes(out_rows - 1, pitch_out, out_end, 4, &out_bytes) ||
        (uintptr_t)d_main + main_bytes < main_bytes || (uintptr_t)d_second + second_bytes < second_bytes || (uintptr_t)d_out + out_bytes < out_bytes) {
        set_error("%s: the span of %zu samples of %d pairs at pitch %zu or %zu, or of as many words of %zu rows from %zu at pitch %zu, overflows", what, n_in,
                  c->n_pairs, pitch_main, pitch_second, out_rows, out_first, pitch_out);
        return NVX_ERR_ARG;
    }
    if ((rows > 1 && (n_in > pitch_main || ((pitch_main * bps) & 15) || n_in > pitch_second || ((pitch_second * bps) & 15))) ||
        (out_rows > 1 && out_end > pitch_out)) {
        set_error("%s: %zu samples per pair at pitches %zu and %zu, words up to %zu at pitch %zu (a row must hold them, and input rows are 16-byte aligned)",
                  what, n_in, pitch_main, pitch_second, out_end, pitch_out);
        return NVX_ERR_ARG;
    }
    // the words written, from the first to the last, against both inputs
    const char *const out_lo = (const char *)d_out + out_first * 4;
    const size_t out_span = out_bytes - out_first * 4;
    if (overlap(out_lo, out_span, d_main, main_bytes) || overlap(out_lo, out_span, d_second, second_bytes)) {
        set_error("%s: the output span (%zu bytes from %p) overlaps an input span (%zu bytes from %p, %zu bytes from %p): the second pass would read words "
                  "the first has not seen", what, out_span, (const void *)out_lo, main_bytes, d_main, second_bytes, d_second);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_main, main_bytes, what, "main input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_second, second_bytes, what, "second input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out, out_bytes, what, "output")) != NVX_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    // a pair that starts anew with this call reads nothing of its state row
    std::vector<uint8_t> skip(c->n_pairs);
    for (int i = 0; i < c->n_pairs; i++) skip[i] = (c->pair_flags(i) & NVX_DIV_PAIR_RESET) ? 1 : 0;
    if ((rc = c->state.align(skip.data(), s)) != NVX_OK) return rc;
    return launch(c, 0, c->n_pairs, consumed, c->state.parity[0], d_main, pitch_main, d_second, pitch_second, n_in, (uint32_t *)d_out, pitch_out, out_first, s);
}

extern "C" int nvx_div_push(nvx_diversity_combiner *c, int pair, const void *main_in, const void *second_in, size_t n_in, int16_t *out_iq)
{
    const char *what = "nvx_div_push";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (pair < 0 || pair >= c->n_pairs || !main_in || !second_in || !out_iq || n_in > NVX_DIV_MAX_IN) {
        set_error("%s: bad argument (pair %d of %d, null pointer, or more than 2^30 samples)", what, pair, c->n_pairs);
        return NVX_ERR_ARG;
    }
    const uint64_t consumed = c->consumed[pair];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    // the second row lies behind the main row, 16-byte aligned; the targets' output rows one after another
    const size_t in_bytes = n_in * (size_t)BPS[c->format], row_bytes = (in_bytes + 15) & ~(size_t)15, K = (size_t)c->n_targets;
    if ((rc = c->push.reserve(what, 2 * row_bytes, K * n_in)) != NVX_OK) return rc;
    void *const d_second = (char *)c->push.d_in + row_bytes;
    HIP_TRY(hipMemcpy(c->push.d_in, main_in, in_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_second, second_in, in_bytes, hipMemcpyHostToDevice));
    if ((rc = launch(c, pair, 1, consumed, c->state.parity[pair], c->push.d_in, n_in, d_second, n_in, n_in, c->push.d_out, n_in, 0, nullptr)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(out_iq, c->push.d_out, K * n_in * 4, hipMemcpyDeviceToHost));   // waits for the null stream
    return NVX_OK;
}
