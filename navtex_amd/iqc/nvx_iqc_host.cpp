// nvx_iqc_host.cpp -- the IQ corrector's entry points (include/navtex_amd_iqc.h): the config checks, the plan with its
// carried positions, state rows, block records and counters, the checks of a call, a push's staging, and the calls that
// read or write a stream's state row (reset, set, set_mode, get).  The launch arithmetic is nvx_iqc_plan.h's.  The library
// stands alone: it shares no state with any other.
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "nvx_companion.h"
#include "nvx_iqc_plan.h"

extern "C" const char *nvx_iqc_last_error(void) { return nvx_error_text(); }

static const uint32_t MAGIC = 0x4e495131u;      // "NIQ1"
static const int BPS[4] = { 4, 2, 2, 8 };       // bytes per input sample, by format
static const char *const NOUN = "the IQ corrector";

struct nvx_iq_corrector {
    uint32_t magic = MAGIC;
    std::mutex mu;
    int device = 0, n_streams = 0, format = 0, window_log2 = 0;
    nvx_state_rows<int64_t> state;                          // [n_streams][NVX_IQC_STATE_WORDS(window_log2)]
    unsigned long long *d_counters = nullptr;               // [n_streams][2]: blocks solved, blocks rejected
    unsigned long long *d_records = nullptr;                // [streams of a call][blocks of a call][NVX_IQC_SUMS]
    size_t records_cap = 0;                                 // in records
    std::vector<uint64_t> consumed, samples;                // samples: since creation
    std::vector<uint8_t> mode;
    nvx_event_timer timer;
    nvx_push_staging push;
    struct { int chunks, tiles_per_chunk, records, form; } last = {};
    int64_t kernel_launches = 0;

    int64_t *scalars(int stream) { return state.row(stream) + NVX_IQC_SUMS * ((size_t)1 << window_log2) + NVX_IQC_SUMS; }
};

static bool valid(const nvx_iq_corrector *c, const char *what)
{
    if (!c || c->magic != MAGIC) { set_error("%s: not an IQ corrector", what); return false; }
    return true;
}

extern "C" void nvx_iqc_config_default(nvx_iqc_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0; cfg->format = NVX_IQC_CS16; cfg->n_streams = 1; cfg->window_log2 = NVX_IQC_WINDOW_LOG2_DEFAULT;
}

// --------------------------------------------------------------------------------------------------------------- plans
static void release(nvx_iq_corrector *c)
{
    c->state.release(); (void)hipFree(c->d_counters); (void)hipFree(c->d_records); c->push.release();
    c->timer.destroy();
    c->magic = 0;
    delete c;
}

// Streams [first, first + n) start anew: empty rows with the identity and each stream's mode, into the row its next launch
// reads.  The caller holds the lock, has selected the device and has waited for it.
static int write_fresh_rows(nvx_iq_corrector *c, int first, int n)
{
    const size_t sw = c->state.words, scalars = sw - NVX_IQC_STATE_SCALARS;
    std::vector<int64_t> image;
    for (int i = first, j; i < first + n; i = j) {
        j = c->state.run_end(i, first + n);
        image.assign((size_t)(j - i) * sw, 0);
        for (int k = i; k < j; k++) {
            image[(size_t)(k - i) * sw + scalars + NVX_IQC_ST_CQ] = NVX_IQC_CQ_IDENTITY;
            image[(size_t)(k - i) * sw + scalars + NVX_IQC_ST_MODE] = c->mode[k];
        }
        HIP_TRY(hipMemcpy(c->state.row(i), image.data(), image.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    return NVX_OK;
}

extern "C" int nvx_iqc_create(const nvx_iqc_config *cfg, nvx_iq_corrector **out)
{
    const char *what = "nvx_iqc_create";
    if (!cfg || !out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    *out = nullptr;
    if (cfg->struct_size != sizeof *cfg) { set_error("%s: struct_size %u, this library's nvx_iqc_config has %zu bytes", what, cfg->struct_size, sizeof *cfg); return NVX_ERR_ARG; }
    if (cfg->n_streams < 1 || cfg->n_streams > 65535) { set_error("%s: n_streams %d (1 .. 65535)", what, cfg->n_streams); return NVX_ERR_ARG; }
    if (cfg->format < NVX_IQC_CS16 || cfg->format > NVX_IQC_CF32) { set_error("%s: format %d (NVX_IQC_CS16 .. NVX_IQC_CF32)", what, cfg->format); return NVX_ERR_ARG; }
    if (cfg->device < 0) { set_error("%s: device %d", what, cfg->device); return NVX_ERR_ARG; }
    if (cfg->window_log2 != 2 && cfg->window_log2 != 4 && cfg->window_log2 != 6) { set_error("%s: window_log2 %d (2, 4 or 6)", what, cfg->window_log2); return NVX_ERR_ARG; }
    nvx_iq_corrector *c = new (std::nothrow) nvx_iq_corrector;
    if (!c) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    int rc = select_device(cfg->device, NOUN);
    if (rc != NVX_OK) { release(c); return rc; }
    c->device = cfg->device; c->n_streams = cfg->n_streams; c->format = cfg->format; c->window_log2 = cfg->window_log2;
    c->consumed.assign(cfg->n_streams, 0); c->samples.assign(cfg->n_streams, 0); c->mode.assign(cfg->n_streams, NVX_IQC_TRACK);
    const size_t counter_bytes = (size_t)cfg->n_streams * 2 * sizeof(unsigned long long);
    hipError_t e = c->state.allocate(cfg->n_streams, NVX_IQC_STATE_WORDS(cfg->window_log2));
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_counters, counter_bytes);
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_NOMEM; }
    e = hipMemset(c->state.d[1], 0, c->state.bytes(cfg->n_streams));
    if (e == hipSuccess) e = hipMemset(c->d_counters, 0, counter_bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: clearing the state failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_HIP; }
    if ((rc = write_fresh_rows(c, 0, cfg->n_streams)) != NVX_OK) { release(c); return rc; }
    *out = c;
    return NVX_OK;
}

extern "C" void nvx_iqc_destroy(nvx_iq_corrector *c)
{
    if (!c || c->magic != MAGIC) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    release(c);
}

extern "C" int nvx_iqc_plan(nvx_iq_corrector *c, int *format, int *n_streams, int *window_log2)
{
    if (!valid(c, "nvx_iqc_plan")) return NVX_ERR_ARG;
    if (format) *format = c->format;
    if (n_streams) *n_streams = c->n_streams;
    if (window_log2) *window_log2 = c->window_log2;
    return NVX_OK;
}

// `stream` (-1: all) stands at `position` with nothing in front of it
static int restart(nvx_iq_corrector *c, const char *what, int stream, uint64_t position)
{
    if (!row_ok(what, "stream", stream, -1, c->n_streams)) return NVX_ERR_ARG;
    if (!position_ok(what, position)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const int first = stream < 0 ? 0 : stream, n = stream < 0 ? c->n_streams : 1;
    if ((rc = write_fresh_rows(c, first, n)) != NVX_OK) return rc;
    for (int i = first; i < first + n; i++) c->consumed[i] = position;
    return NVX_OK;
}

extern "C" int nvx_iqc_reset(nvx_iq_corrector *c, int stream)
{
    return valid(c, "nvx_iqc_reset") ? restart(c, "nvx_iqc_reset", stream, 0) : NVX_ERR_ARG;
}

extern "C" int nvx_iqc_debug_set_position(nvx_iq_corrector *c, int stream, uint64_t position)
{
    return valid(c, "nvx_iqc_debug_set_position") ? restart(c, "nvx_iqc_debug_set_position", stream, position) : NVX_ERR_ARG;
}

extern "C" int nvx_iqc_position(nvx_iq_corrector *c, int stream, uint64_t *consumed)
{
    const char *what = "nvx_iqc_position";
    if (!valid(c, what) || !row_ok(what, "stream", stream, 0, c->n_streams)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (consumed) *consumed = c->consumed[stream];
    return NVX_OK;
}

// `count` scalars of the state rows of `stream` (-1: all), from scalar `at` on, become `values`
static int write_scalars(nvx_iq_corrector *c, int stream, int at, const int64_t *values, int count)
{
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    for (int i = stream < 0 ? 0 : stream; i < (stream < 0 ? c->n_streams : stream + 1); i++)
        HIP_TRY(hipMemcpy(c->scalars(i) + at, values, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice));
    return NVX_OK;
}

extern "C" int nvx_iqc_set(nvx_iq_corrector *c, int stream, int dI, int dQ, int c_i, int c_q)
{
    const char *what = "nvx_iqc_set";
    if (!valid(c, what) || !row_ok(what, "stream", stream, -1, c->n_streams)) return NVX_ERR_ARG;
    if (dI < -32768 || dI > 32767 || dQ < -32768 || dQ > 32767 || c_i < -NVX_IQC_CI_MAX || c_i > NVX_IQC_CI_MAX || c_q < NVX_IQC_CQ_MIN || c_q > NVX_IQC_CQ_MAX) {
        set_error("%s: (%d, %d, %d, %d): dI, dQ in -32768 .. 32767, |c_i| <= %d, c_q in %d .. %d", what, dI, dQ, c_i, c_q, NVX_IQC_CI_MAX, NVX_IQC_CQ_MIN,
                  NVX_IQC_CQ_MAX);
        return NVX_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    const int64_t v[4] = { dI, dQ, c_i, c_q };
    return write_scalars(c, stream, NVX_IQC_ST_DI, v, 4);
}

extern "C" int nvx_iqc_set_mode(nvx_iq_corrector *c, int stream, int mode)
{
    const char *what = "nvx_iqc_set_mode";
    if (!valid(c, what) || !row_ok(what, "stream", stream, -1, c->n_streams)) return NVX_ERR_ARG;
    if (mode != NVX_IQC_TRACK && mode != NVX_IQC_HOLD) { set_error("%s: mode %d (NVX_IQC_TRACK or NVX_IQC_HOLD)", what, mode); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    const int64_t v = mode;
    const int rc = write_scalars(c, stream, NVX_IQC_ST_MODE, &v, 1);
    if (rc == NVX_OK)
        for (int i = stream < 0 ? 0 : stream; i < (stream < 0 ? c->n_streams : stream + 1); i++) c->mode[i] = (uint8_t)mode;
    return rc;
}

extern "C" int nvx_iqc_get(nvx_iq_corrector *c, int stream, nvx_iqc_status *out)
{
    const char *what = "nvx_iqc_get";
    if (!valid(c, what) || !row_ok(what, "stream", stream, 0, c->n_streams)) return NVX_ERR_ARG;
    if (!out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    std::vector<int64_t> row(c->state.words);
    unsigned long long counters[2] = { 0, 0 };
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(row.data(), c->state.row(stream),row.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counters, c->d_counters + 2 * (size_t)stream, sizeof counters, hipMemcpyDeviceToHost));
    const int W = 1 << c->window_log2;
    const int64_t *sc = row.data() + NVX_IQC_SUMS * W + NVX_IQC_SUMS;
    memset(out, 0, sizeof *out);
    out->dI = (int32_t)sc[NVX_IQC_ST_DI]; out->dQ = (int32_t)sc[NVX_IQC_ST_DQ]; out->c_i = (int32_t)sc[NVX_IQC_ST_CI]; out->c_q = (int32_t)sc[NVX_IQC_ST_CQ];
    out->mode = (int32_t)sc[NVX_IQC_ST_MODE]; out->last_reason = (int32_t)sc[NVX_IQC_ST_REASON];
    for (int b = 0; b < W; b++)                             // blocks not complete since the reset are zero
        for (int k = 0; k < NVX_IQC_SUMS; k++) out->sums[k] += row[(size_t)b * NVX_IQC_SUMS + k];
    out->samples = c->samples[stream]; out->blocks_solved = counters[0]; out->blocks_rejected = counters[1];
    return NVX_OK;
}

extern "C" int nvx_iqc_timing(nvx_iq_corrector *c, int enable)
{
    return valid(c, "nvx_iqc_timing") ? timing_enable(c->mu, c->timer, enable) : NVX_ERR_ARG;
}

extern "C" int nvx_iqc_time_stats(nvx_iq_corrector *c, double *sum_ms, uint64_t *calls, int reset)
{
    return valid(c, "nvx_iqc_time_stats") ? timing_collect(c->mu, c->timer, sum_ms, calls, reset) : NVX_ERR_ARG;
}

extern "C" int64_t nvx_iqc_debug_last_launch(nvx_iq_corrector *c, int *chunks, int *tiles_per_chunk, int *records, int *form)
{
    if (!valid(c, "nvx_iqc_debug_last_launch")) return NVX_ERR_ARG;
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
// One call over streams [first, first + n) of the plan, which stand at `consumed` and read state row `parity`; the caller
// holds the plan's lock and has checked every span.
static int launch(nvx_iq_corrector *c, int first, int n, uint64_t consumed, int parity, const void *d_in, size_t pitch_in, size_t n_in,
                  uint32_t *d_out, size_t pitch_out, size_t out_first, hipStream_t s)
{
    const int wanted = nvx_stream_wanted(n, NVX_IQC_TARGET_WORKGROUPS);
    nvx_iqc_args a;
    int chunks = nvx_iqc_fill_args(consumed, d_in, pitch_in, n_in, d_out, pitch_out, out_first, n, nullptr, nullptr, nullptr, nullptr, c->window_log2, wanted, &a);
    // the call's block records, from zero
    const size_t records = (size_t)n * (size_t)a.blocks;
    if (records > c->records_cap) {
        HIP_TRY(hipDeviceSynchronize());                    // an earlier call may still use the old ones
        (void)hipFree(c->d_records); c->d_records = nullptr; c->records_cap = 0;
        if (hipMalloc((void **)&c->d_records, records * NVX_IQC_SUMS * sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: hipMalloc of %zu block records failed", "nvx_iqc", records);
            return NVX_ERR_NOMEM;
        }
        c->records_cap = records;
    }
    chunks = nvx_iqc_fill_args(consumed, d_in, pitch_in, n_in, d_out, pitch_out, out_first, n, c->state.in(first, parity), c->state.out(first, parity),
                               c->d_records, c->d_counters + 2 * (size_t)first, c->window_log2, wanted, &a);
    nvx_event_timer::events ev;
    int rc;
    if ((rc = c->timer.begin(s, ev)) != NVX_OK) return rc;
    HIP_TRY(hipMemsetAsync(c->d_records, 0, records * NVX_IQC_SUMS * sizeof(unsigned long long), s));
    HIP_TRY(nvx_iqc_launch(&a, c->format, n, chunks, s));
    c->last = { chunks, a.tiles_per_chunk, a.blocks, chunks > 1 ? 2 : 1 };
    c->kernel_launches += 2;
    if ((rc = c->timer.end(s, ev)) != NVX_OK) return rc;
    for (int i = first; i < first + n; i++) { c->consumed[i] = consumed + n_in; c->samples[i] += n_in; }
    c->state.flip(first, n, parity);
    return NVX_OK;
}

extern "C" int nvx_iqc_resident(nvx_iq_corrector *c, const void *d_in, size_t pitch_in, size_t n_in, void *d_out, size_t pitch_out,
                                size_t out_first, void *hip_stream)
{
    const char *what = "nvx_iqc_resident";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!d_in || !d_out || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 3) || n_in > NVX_IQC_MAX_IN) {
        set_error("%s: bad argument (null pointer, input not 16-byte aligned, output not 4-byte aligned, or more than 2^30 samples)", what);
        return NVX_ERR_ARG;
    }
    if (!all_stand_together(what, "stream", c->consumed)) return NVX_ERR_STATE;
    const uint64_t consumed = c->consumed[0];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    size_t in_bytes, out_bytes;
    int rc = resident_spans(what, c->n_streams, (size_t)BPS[c->format], n_in, pitch_in, n_in, "as many", pitch_out, out_first, &in_bytes, &out_bytes);
    if (rc != NVX_OK || n_in == 0) return rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_in, in_bytes, what, "input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out, out_bytes, what, "output")) != NVX_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    if ((rc = c->state.align(nullptr, s)) != NVX_OK) return rc;
    return launch(c, 0, c->n_streams, consumed, c->state.parity[0], d_in, pitch_in, n_in, (uint32_t *)d_out, pitch_out, out_first, s);
}

extern "C" int nvx_iqc_push(nvx_iq_corrector *c, int stream, const void *in, size_t n_in, int16_t *out_iq)
{
    const char *what = "nvx_iqc_push";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (stream < 0 || stream >= c->n_streams || !in || !out_iq || n_in > NVX_IQC_MAX_IN) {
        set_error("%s: bad argument (stream %d of %d, null pointer, or more than 2^30 samples)", what, stream, c->n_streams);
        return NVX_ERR_ARG;
    }
    const uint64_t consumed = c->consumed[stream];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    const size_t in_bytes = n_in * (size_t)BPS[c->format];
    if ((rc = c->push.reserve(what, in_bytes, n_in)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(c->push.d_in, in, in_bytes, hipMemcpyHostToDevice));
    if ((rc = launch(c, stream, 1, consumed, c->state.parity[stream], c->push.d_in, n_in, n_in, c->push.d_out, n_in, 0, nullptr)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(out_iq, c->push.d_out, n_in * 4, hipMemcpyDeviceToHost));     // waits for the null stream
    return NVX_OK;
}
