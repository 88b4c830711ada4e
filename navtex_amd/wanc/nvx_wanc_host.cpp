// nvx_wanc_host.cpp -- the multi-tap canceller's entry points (include/navtex_amd_wanc.h): the config checks, the plan with its
// carried positions, state rows, block records, weight records and counters, the checks of a call, a push's staging, and the
// calls that read or write a pair's state row (reset, set, set_mode, get).  The launch arithmetic is nvx_wanc_plan.h's.  The
// library stands alone: it shares no state with any other.
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "nvx_companion.h"
#include "nvx_wanc_plan.h"

extern "C" const char *nvx_wanc_last_error(void) { return nvx_error_text(); }

static const uint32_t MAGIC = 0x4e574e31u;      // "NWN1"
static const int BPS[4] = { 4, 2, 2, 8 };       // bytes per input sample, by format
static const char *const NOUN = "the multi-tap canceller";

struct nvx_wide_canceller {
    uint32_t magic = MAGIC;
    std::mutex mu;
    int device = 0, n_pairs = 0, format = 0, window_log2 = 0, n_taps = 0, load_log2 = 0;
    nvx_state_rows<int64_t> state;                          // [n_pairs][NVX_WANC_STATE_WORDS(n_taps, window_log2)]
    unsigned long long *d_counters = nullptr;               // [n_pairs][2]: blocks solved, blocks rejected
    unsigned long long *d_records = nullptr;                // [pairs of a call][blocks of a call][NVX_WANC_SUMS(n_taps)]
    int32_t *d_weights = nullptr;                           // [pairs of a call][blocks of a call][NVX_WANC_WREC(n_taps)]
    size_t records_cap = 0;                                 // in records
    std::vector<uint64_t> consumed, samples;                // samples: since creation
    std::vector<uint8_t> mode;
    nvx_event_timer timer;
    nvx_push_staging push;                                  // a push's two input rows, one behind the other, and its output
    struct { int chunks, tiles_per_chunk, records, form; } last = {};
    int64_t kernel_launches = 0;

    size_t scalars() const { return NVX_WANC_ST_SCALARS(n_taps, window_log2); }
    size_t weights() const { return NVX_WANC_ST_WEIGHTS(n_taps, window_log2); }
};

static bool valid(const nvx_wide_canceller *c, const char *what)
{
    if (!c || c->magic != MAGIC) { set_error("%s: not a multi-tap canceller", what); return false; }
    return true;
}

extern "C" void nvx_wanc_config_default(nvx_wanc_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0; cfg->format = NVX_WANC_CS16; cfg->n_pairs = 1; cfg->window_log2 = NVX_WANC_WINDOW_LOG2_DEFAULT;
    cfg->n_taps = NVX_WANC_TAPS_DEFAULT; cfg->load_log2 = NVX_WANC_LOAD_LOG2_DEFAULT;
}

// --------------------------------------------------------------------------------------------------------------- plans
static void release(nvx_wide_canceller *c)
{
    c->state.release(); (void)hipFree(c->d_counters); (void)hipFree(c->d_records); (void)hipFree(c->d_weights); c->push.release();
    c->timer.destroy();
    c->magic = 0;
    delete c;
}

// Pairs [first, first + n) start anew: empty rows with zero weights, silence in front and each pair's mode, into the row its
// next launch reads.  The caller holds the lock, has selected the device and has waited for it.
static int write_fresh_rows(nvx_wide_canceller *c, int first, int n)
{
    const size_t sw = c->state.words;
    std::vector<int64_t> image;
    for (int i = first, j; i < first + n; i = j) {
        j = c->state.run_end(i, first + n);
        image.assign((size_t)(j - i) * sw, 0);
        for (int k = i; k < j; k++) image[(size_t)(k - i) * sw + c->scalars() + NVX_WANC_SC_MODE] = c->mode[k];
        HIP_TRY(hipMemcpy(c->state.row(i), image.data(), image.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    return NVX_OK;
}

extern "C" int nvx_wanc_create(const nvx_wanc_config *cfg, nvx_wide_canceller **out)
{
    const char *what = "nvx_wanc_create";
    if (!cfg || !out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    *out = nullptr;
    if (cfg->struct_size != sizeof *cfg) { set_error("%s: struct_size %u, this library's nvx_wanc_config has %zu bytes", what, cfg->struct_size, sizeof *cfg); return NVX_ERR_ARG; }
    if (cfg->n_pairs < 1 || cfg->n_pairs > 65535) { set_error("%s: n_pairs %d (1 .. 65535)", what, cfg->n_pairs); return NVX_ERR_ARG; }
    if (cfg->format < NVX_WANC_CS16 || cfg->format > NVX_WANC_CF32) { set_error("%s: format %d (NVX_WANC_CS16 .. NVX_WANC_CF32)", what, cfg->format); return NVX_ERR_ARG; }
    if (cfg->device < 0) { set_error("%s: device %d", what, cfg->device); return NVX_ERR_ARG; }
    if (cfg->window_log2 != 2 && cfg->window_log2 != 4 && cfg->window_log2 != 6) { set_error("%s: window_log2 %d (2, 4 or 6)", what, cfg->window_log2); return NVX_ERR_ARG; }
    if (cfg->n_taps != 4 && cfg->n_taps != 8 && cfg->n_taps != 16) { set_error("%s: n_taps %d (4, 8 or 16)", what, cfg->n_taps); return NVX_ERR_ARG; }
    if (cfg->load_log2 < 8 || cfg->load_log2 > 20) { set_error("%s: load_log2 %d (8 .. 20)", what, cfg->load_log2); return NVX_ERR_ARG; }
    nvx_wide_canceller *c = new (std::nothrow) nvx_wide_canceller;
    if (!c) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    int rc = select_device(cfg->device, NOUN);
    if (rc != NVX_OK) { release(c); return rc; }
    c->device = cfg->device; c->n_pairs = cfg->n_pairs; c->format = cfg->format; c->window_log2 = cfg->window_log2;
    c->n_taps = cfg->n_taps; c->load_log2 = cfg->load_log2;
    c->consumed.assign(cfg->n_pairs, 0); c->samples.assign(cfg->n_pairs, 0); c->mode.assign(cfg->n_pairs, NVX_WANC_TRACK);
    const size_t counter_bytes = (size_t)cfg->n_pairs * 2 * sizeof(unsigned long long);
    hipError_t e = c->state.allocate(cfg->n_pairs, NVX_WANC_STATE_WORDS(cfg->n_taps, cfg->window_log2));
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_counters, counter_bytes);
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_NOMEM; }
    e = hipMemset(c->state.d[1], 0, c->state.bytes(cfg->n_pairs));
    if (e == hipSuccess) e = hipMemset(c->d_counters, 0, counter_bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: clearing the state failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_HIP; }
    if ((rc = write_fresh_rows(c, 0, cfg->n_pairs)) != NVX_OK) { release(c); return rc; }
    *out = c;
    return NVX_OK;
}

extern "C" void nvx_wanc_destroy(nvx_wide_canceller *c)
{
    if (!c || c->magic != MAGIC) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    release(c);
}

extern "C" int nvx_wanc_plan(nvx_wide_canceller *c, int *format, int *n_pairs, int *window_log2, int *n_taps, int *load_log2)
{
    if (!valid(c, "nvx_wanc_plan")) return NVX_ERR_ARG;
    if (format) *format = c->format;
    if (n_pairs) *n_pairs = c->n_pairs;
    if (window_log2) *window_log2 = c->window_log2;
    if (n_taps) *n_taps = c->n_taps;
    if (load_log2) *load_log2 = c->load_log2;
    return NVX_OK;
}

// `pair` (-1: all) stands at `position` with nothing in front of it
static int restart(nvx_wide_canceller *c, const char *what, int pair, uint64_t position)
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

extern "C" int nvx_wanc_reset(nvx_wide_canceller *c, int pair)
{
    return valid(c, "nvx_wanc_reset") ? restart(c, "nvx_wanc_reset", pair, 0) : NVX_ERR_ARG;
}

extern "C" int nvx_wanc_debug_set_position(nvx_wide_canceller *c, int pair, uint64_t position)
{
    return valid(c, "nvx_wanc_debug_set_position") ? restart(c, "nvx_wanc_debug_set_position", pair, position) : NVX_ERR_ARG;
}

extern "C" int nvx_wanc_position(nvx_wide_canceller *c, int pair, uint64_t *consumed)
{
    const char *what = "nvx_wanc_position";
    if (!valid(c, what) || !row_ok(what, "pair", pair, 0, c->n_pairs)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (consumed) *consumed = c->consumed[pair];
    return NVX_OK;
}

// `count` words of the state rows of `pair` (-1: all), from word `at` on, become `values`
static int write_words(nvx_wide_canceller *c, int pair, size_t at, const int64_t *values, int count)
{
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    for (int i = pair < 0 ? 0 : pair; i < (pair < 0 ? c->n_pairs : pair + 1); i++)
        HIP_TRY(hipMemcpy(c->state.row(i) + at, values, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice));
    return NVX_OK;
}

extern "C" int nvx_wanc_set(nvx_wide_canceller *c, int pair, const int32_t *w_re, const int32_t *w_im)
{
    const char *what = "nvx_wanc_set";
    if (!valid(c, what) || !row_ok(what, "pair", pair, -1, c->n_pairs)) return NVX_ERR_ARG;
    if (!w_re || !w_im) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    int64_t v[2 * NVX_WANC_TAPS_MAX], l1 = 0;
    for (int k = 0; k < 2 * c->n_taps; k++) {
        v[k] = k < c->n_taps ? w_re[k] : w_im[k - c->n_taps];
        if (v[k] < -NVX_WANC_W_MAX || v[k] > NVX_WANC_W_MAX) { set_error("%s: weight %d is (%d, %d): |w_re|, |w_im| <= %d", what, k % c->n_taps, w_re[k % c->n_taps], w_im[k % c->n_taps], NVX_WANC_W_MAX); return NVX_ERR_ARG; }
        l1 += v[k] < 0 ? -v[k] : v[k];
    }
    if (l1 > NVX_WANC_L1_MAX) { set_error("%s: the weights' L1 sum is %lld: at most %d", what, (long long)l1, NVX_WANC_L1_MAX); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    return write_words(c, pair, c->weights(), v, 2 * c->n_taps);
}

extern "C" int nvx_wanc_set_mode(nvx_wide_canceller *c, int pair, int mode)
{
    const char *what = "nvx_wanc_set_mode";
    if (!valid(c, what) || !row_ok(what, "pair", pair, -1, c->n_pairs)) return NVX_ERR_ARG;
    if (mode != NVX_WANC_TRACK && mode != NVX_WANC_HOLD) { set_error("%s: mode %d (NVX_WANC_TRACK or NVX_WANC_HOLD)", what, mode); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    const int64_t v = mode;
    const int rc = write_words(c, pair, c->scalars() + NVX_WANC_SC_MODE, &v, 1);
    if (rc == NVX_OK)
        for (int i = pair < 0 ? 0 : pair; i < (pair < 0 ? c->n_pairs : pair + 1); i++) c->mode[i] = (uint8_t)mode;
    return rc;
}

extern "C" int nvx_wanc_get(nvx_wide_canceller *c, int pair, nvx_wanc_status *out)
{
    const char *what = "nvx_wanc_get";
    if (!valid(c, what) || !row_ok(what, "pair", pair, 0, c->n_pairs)) return NVX_ERR_ARG;
    if (!out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    std::vector<int64_t> row(c->state.words);
    unsigned long long counters[2] = { 0, 0 };
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(row.data(), c->state.row(pair), row.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counters, c->d_counters + 2 * (size_t)pair, sizeof counters, hipMemcpyDeviceToHost));
    const int W = 1 << c->window_log2, K = c->n_taps, NS = NVX_WANC_SUMS(K);
    const int64_t *sc = row.data() + c->scalars(), *w = row.data() + c->weights();
    memset(out, 0, sizeof *out);
    out->n_taps = K; out->mode = (int32_t)sc[NVX_WANC_SC_MODE]; out->last_reason = (int32_t)sc[NVX_WANC_SC_REASON];
    out->coherence_q14 = (int32_t)sc[NVX_WANC_SC_COHERENCE];
    for (int k = 0; k < K; k++) { out->w_re[k] = (int32_t)w[k]; out->w_im[k] = (int32_t)w[K + k]; }
    for (int b = 0; b < W; b++) {                           // blocks not complete since the reset are zero
        const int64_t *s = row.data() + (size_t)b * NS;
        for (int k = 0; k < K; k++) { out->r_re[k] += s[k]; out->r_im[k] += s[K + k]; out->q_re[k] += s[2 * K + k]; out->q_im[k] += s[3 * K + k]; }
        out->saa += s[4 * K];
    }
    out->samples = c->samples[pair]; out->blocks_solved = counters[0]; out->blocks_rejected = counters[1];
    return NVX_OK;
}

extern "C" int nvx_wanc_timing(nvx_wide_canceller *c, int enable)
{
    return valid(c, "nvx_wanc_timing") ? timing_enable(c->mu, c->timer, enable) : NVX_ERR_ARG;
}

extern "C" int nvx_wanc_time_stats(nvx_wide_canceller *c, double *sum_ms, uint64_t *calls, int reset)
{
    return valid(c, "nvx_wanc_time_stats") ? timing_collect(c->mu, c->timer, sum_ms, calls, reset) : NVX_ERR_ARG;
}

extern "C" int64_t nvx_wanc_debug_last_launch(nvx_wide_canceller *c, int *chunks, int *tiles_per_chunk, int *records, int *form)
{
    if (!valid(c, "nvx_wanc_debug_last_launch")) return NVX_ERR_ARG;
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
// One call over pairs [first, first + n) of the plan, which stand at `consumed` and read state row `parity`; the caller
// holds the plan's lock and has checked every span.
static int launch(nvx_wide_canceller *c, int first, int n, uint64_t consumed, int parity, const void *d_main, size_t pitch_main, const void *d_sense,
                  size_t pitch_sense, size_t n_in, uint32_t *d_out, size_t pitch_out, size_t out_first, hipStream_t s)
{
    const int wanted = nvx_stream_wanted(n, NVX_WANC_TARGET_WORKGROUPS);
    const int K = c->n_taps;
    nvx_wanc_args a;
    int chunks = nvx_wanc_fill_args(consumed, d_main, pitch_main, d_sense, pitch_sense, n_in, d_out, pitch_out, out_first, n, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, c->window_log2, K, c->load_log2, wanted, &a);
    // the call's block records, from zero, and its weight records
    const size_t records = (size_t)n * (size_t)a.blocks;
    if (records > c->records_cap) {
        HIP_TRY(hipDeviceSynchronize());                    // an earlier call may still use the old ones
        (void)hipFree(c->d_records); (void)hipFree(c->d_weights); c->d_records = nullptr; c->d_weights = nullptr; c->records_cap = 0;
        if (hipMalloc((void **)&c->d_records, records * NVX_WANC_SUMS(K) * sizeof(unsigned long long)) != hipSuccess ||
            hipMalloc((void **)&c->d_weights, records * NVX_WANC_WREC(K) * sizeof(int32_t)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(c->d_records); c->d_records = nullptr;
            set_error("%s: hipMalloc of %zu block records failed", "nvx_wanc", records);
            return NVX_ERR_NOMEM;
        }
        c->records_cap = records;
    }
    chunks = nvx_wanc_fill_args(consumed, d_main, pitch_main, d_sense, pitch_sense, n_in, d_out, pitch_out, out_first, n, c->state.in(first, parity),
                                c->state.out(first, parity), c->d_records, c->d_weights, c->d_counters + 2 * (size_t)first, c->window_log2, K, c->load_log2,
                                wanted, &a);
    nvx_event_timer::events ev;
    int rc;
    if ((rc = c->timer.begin(s, ev)) != NVX_OK) return rc;
    HIP_TRY(hipMemsetAsync(c->d_records, 0, records * NVX_WANC_SUMS(K) * sizeof(unsigned long long), s));
    HIP_TRY(nvx_wanc_launch(&a, c->format, n, chunks, s));
    c->last = { chunks, a.tiles_per_chunk, a.blocks, chunks > 1 ? 2 : 1 };
    c->kernel_launches += 3;
    if ((rc = c->timer.end(s, ev)) != NVX_OK) return rc;
    for (int i = first; i < first + n; i++) { c->consumed[i] = consumed + n_in; c->samples[i] += n_in; }
    c->state.flip(first, n, parity);
    return NVX_OK;
}

// [p, p + bytes) and [q, q + size) have a byte in common
static bool overlap(const void *p, size_t bytes, const void *q, size_t size)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return bytes && size && a < b + size && b < a + bytes;
}

extern "C" int nvx_wanc_resident(nvx_wide_canceller *c, const void *d_main, size_t pitch_main, const void *d_sense, size_t pitch_sense, size_t n_in,
                                 void *d_out, size_t pitch_out, size_t out_first, void *hip_stream)
{
    const char *what = "nvx_wanc_resident";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!d_main || !d_sense || !d_out || ((uintptr_t)d_main & 15) || ((uintptr_t)d_sense & 15) || ((uintptr_t)d_out & 3) || n_in > NVX_WANC_MAX_IN) {
        set_error("%s: bad argument (null pointer, an input not 16-byte aligned, output not 4-byte aligned, or more than 2^30 samples)", what);
        return NVX_ERR_ARG;
    }
    if (!all_stand_together(what, "pair", c->consumed)) return NVX_ERR_STATE;
    const uint64_t consumed = c->consumed[0];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    // every row's last sample read and last word written, in samples of its row (out_end) and in bytes of the whole operand
    const size_t rows = (size_t)c->n_pairs, bps = (size_t)BPS[c->format];
    size_t out_end, main_bytes, sense_bytes, out_bytes;
    if (__builtin_add_overflow(out_first, n_in, &out_end) || !span_bytes(rows - 1, pitch_main, n_in, bps, &main_bytes) ||
        !span_bytes(rows - 1, pitch_sense, n_in, bps, &sense_bytes) || !span_bytes(rows - 1, pitch_out, out_end, 4, &out_bytes) ||
        (uintptr_t)d_main + main_bytes < main_bytes || (uintptr_t)d_sense + sense_bytes < sense_bytes || (uintptr_t)d_out + out_bytes < out_bytes) {
        set_error("%s: the span of %zu samples of %d pairs at pitch %zu or %zu, or of as many words from %zu at pitch %zu, overflows", what, n_in,
                  c->n_pairs, pitch_main, pitch_sense, out_first, pitch_out);
        return NVX_ERR_ARG;
    }
    if (rows > 1 && (n_in > pitch_main || ((pitch_main * bps) & 15) || n_in > pitch_sense || ((pitch_sense * bps) & 15) || out_end > pitch_out)) {
        set_error("%s: %zu samples per pair at pitches %zu and %zu, words up to %zu at pitch %zu (a row must hold them, and input rows are 16-byte aligned)",
                  what, n_in, pitch_main, pitch_sense, out_end, pitch_out);
        return NVX_ERR_ARG;
    }
    // the words written, from the first to the last, against both inputs
    const char *const out_lo = (const char *)d_out + out_first * 4;
    const size_t out_span = out_bytes - out_first * 4;
    if (overlap(out_lo, out_span, d_main, main_bytes) || overlap(out_lo, out_span, d_sense, sense_bytes)) {
        set_error("%s: the output span (%zu bytes from %p) overlaps an input span (%zu bytes from %p, %zu bytes from %p): the second pass would read words "
                  "the first has not seen", what, out_span, (const void *)out_lo, main_bytes, d_main, sense_bytes, d_sense);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_main, main_bytes, what, "main input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_sense, sense_bytes, what, "sense input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out, out_bytes, what, "output")) != NVX_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    if ((rc = c->state.align(nullptr, s)) != NVX_OK) return rc;
    return launch(c, 0, c->n_pairs, consumed, c->state.parity[0], d_main, pitch_main, d_sense, pitch_sense, n_in, (uint32_t *)d_out, pitch_out, out_first, s);
}

extern "C" int nvx_wanc_push(nvx_wide_canceller *c, int pair, const void *main_in, const void *sense_in, size_t n_in, int16_t *out_iq)
{
    const char *what = "nvx_wanc_push";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (pair < 0 || pair >= c->n_pairs || !main_in || !sense_in || !out_iq || n_in > NVX_WANC_MAX_IN) {
        set_error("%s: bad argument (pair %d of %d, null pointer, or more than 2^30 samples)", what, pair, c->n_pairs);
        return NVX_ERR_ARG;
    }
    const uint64_t consumed = c->consumed[pair];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    // the sense row lies behind the main row, 16-byte aligned
    const size_t in_bytes = n_in * (size_t)BPS[c->format], row_bytes = (in_bytes + 15) & ~(size_t)15;
    if ((rc = c->push.reserve(what, 2 * row_bytes, n_in)) != NVX_OK) return rc;
    void *const d_sense = (char *)c->push.d_in + row_bytes;
    HIP_TRY(hipMemcpy(c->push.d_in, main_in, in_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_sense, sense_in, in_bytes, hipMemcpyHostToDevice));
    if ((rc = launch(c, pair, 1, consumed, c->state.parity[pair], c->push.d_in, n_in, d_sense, n_in, n_in, c->push.d_out, n_in, 0, nullptr)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(out_iq, c->push.d_out, n_in * 4, hipMemcpyDeviceToHost));     // waits for the null stream
    return NVX_OK;
}
