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
    int device = 0, n_streams = 0, format = 0, window_log2 = 0, state_words = 0;
    int64_t *d_state[2] = { nullptr, nullptr };             // [n_streams][state_words], read and written alternately
    unsigned long long *d_counters = nullptr;               // [n_streams][2]: blocks solved, blocks rejected
    unsigned long long *d_records = nullptr;                // [streams of a call][blocks of a call][NVX_IQC_SUMS]
    size_t records_cap = 0;                                 // in records
    std::vector<uint64_t> consumed, samples;                // samples: since creation
    std::vector<uint8_t> parity;                            // which state row the stream's next launch reads
    std::vector<uint8_t> mode;
    nvx_event_timer timer;
    void *d_push_in = nullptr; uint32_t *d_push_out = nullptr;
    size_t push_in_cap = 0, push_out_cap = 0;
    struct { int chunks, tiles_per_chunk, records, form; } last = {};
    int64_t kernel_launches = 0;

    int64_t *row(int stream) { return d_state[parity[stream]] + (size_t)stream * state_words; }
    int64_t *scalars(int stream) { return row(stream) + NVX_IQC_SUMS * ((size_t)1 << window_log2) + NVX_IQC_SUMS; }
};

static bool valid(const nvx_iq_corrector *c, const char *what)
{
    if (!c || c->magic != MAGIC) { set_error("%s: not an IQ corrector", what); return false; }
    return true;
}

static bool stream_ok(const nvx_iq_corrector *c, const char *what, int stream, int lowest)
{
    if (stream < lowest || stream >= c->n_streams) { set_error("%s: stream %d of %d", what, stream, c->n_streams); return false; }
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
    (void)hipFree(c->d_state[0]); (void)hipFree(c->d_state[1]); (void)hipFree(c->d_counters); (void)hipFree(c->d_records);
    (void)hipFree(c->d_push_in); (void)hipFree(c->d_push_out);
    c->timer.destroy();
    c->magic = 0;
    delete c;
}

// Streams [first, first + n) start anew: empty rows with the identity and each stream's mode, into the row its next launch
// reads.  The caller holds the lock, has selected the device and has waited for it.
static int write_fresh_rows(nvx_iq_corrector *c, int first, int n)
{
    const size_t sw = (size_t)c->state_words, scalars = sw - NVX_IQC_STATE_SCALARS;
    std::vector<int64_t> image;
    for (int i = first; i < first + n;) {
        int j = i;
        while (j < first + n && c->parity[j] == c->parity[i]) j++;
        image.assign((size_t)(j - i) * sw, 0);
        for (int k = i; k < j; k++) {
            image[(size_t)(k - i) * sw + scalars + NVX_IQC_ST_CQ] = NVX_IQC_CQ_IDENTITY;
            image[(size_t)(k - i) * sw + scalars + NVX_IQC_ST_MODE] = c->mode[k];
        }
        HIP_TRY(hipMemcpy(c->row(i), image.data(), image.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        i = j;
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
    c->state_words = NVX_IQC_STATE_WORDS(cfg->window_log2);
    c->consumed.assign(cfg->n_streams, 0); c->samples.assign(cfg->n_streams, 0);
    c->parity.assign(cfg->n_streams, 0); c->mode.assign(cfg->n_streams, NVX_IQC_TRACK);
    const size_t state_bytes = (size_t)cfg->n_streams * c->state_words * sizeof(int64_t), counter_bytes = (size_t)cfg->n_streams * 2 * sizeof(unsigned long long);
    hipError_t e = hipMalloc((void **)&c->d_state[0], state_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_state[1], state_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_counters, counter_bytes);
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_NOMEM; }
    e = hipMemset(c->d_state[1], 0, state_bytes);
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
    if (!stream_ok(c, what, stream, -1)) return NVX_ERR_ARG;
    if (position >> 62) { set_error("%s: the position passes 2^62", what); return NVX_ERR_ARG; }
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
    if (!valid(c, what) || !stream_ok(c, what, stream, 0)) return NVX_ERR_ARG;
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
    if (!valid(c, what) || !stream_ok(c, what, stream, -1)) return NVX_ERR_ARG;
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
    if (!valid(c, what) || !stream_ok(c, what, stream, -1)) return NVX_ERR_ARG;
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
    if (!valid(c, what) || !stream_ok(c, what, stream, 0)) return NVX_ERR_ARG;
    if (!out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    std::vector<int64_t> row((size_t)c->state_words);
    unsigned long long counters[2] = { 0, 0 };
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(row.data(), c->row(stream), row.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
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
    if (!valid(c, "nvx_iqc_timing")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    c->timer.enabled = enable != 0;
    return NVX_OK;
}

extern "C" int nvx_iqc_time_stats(nvx_iq_corrector *c, double *sum_ms, uint64_t *calls, int reset)
{
    if (!valid(c, "nvx_iqc_time_stats")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    return c->timer.collect(sum_ms, calls, reset);
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
    // a workgroup per stream fills the chip from a few workgroups per CU on; below that a stream's tiles are spread out
    const int wanted = n >= 1024 ? 1 : (NVX_IQC_TARGET_WORKGROUPS + n - 1) / n;
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
    chunks = nvx_iqc_fill_args(consumed, d_in, pitch_in, n_in, d_out, pitch_out, out_first, n, c->d_state[parity] + (size_t)first * c->state_words,
                               c->d_state[parity ^ 1] + (size_t)first * c->state_words, c->d_records, c->d_counters + 2 * (size_t)first, c->window_log2,
                               wanted, &a);
    nvx_event_timer::events ev;
    int rc;
    if ((rc = c->timer.begin(s, ev)) != NVX_OK) return rc;
    HIP_TRY(hipMemsetAsync(c->d_records, 0, records * NVX_IQC_SUMS * sizeof(unsigned long long), s));
    HIP_TRY(nvx_iqc_launch(&a, c->format, n, chunks, s));
    c->last = { chunks, a.tiles_per_chunk, a.blocks, chunks > 1 ? 2 : 1 };
    c->kernel_launches += 2;
    if ((rc = c->timer.end(s, ev)) != NVX_OK) return rc;
    for (int i = first; i < first + n; i++) { c->consumed[i] = consumed + n_in; c->samples[i] += n_in; c->parity[i] = (uint8_t)(parity ^ 1); }
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
    for (int i = 1; i < c->n_streams; i++)
        if (c->consumed[i] != c->consumed[0]) {
            set_error("%s: stream %d stands at %llu, stream 0 at %llu: all streams of a call stand at the same position", what, i,
                      (unsigned long long)c->consumed[i], (unsigned long long)c->consumed[0]);
            return NVX_ERR_STATE;
        }
    const uint64_t consumed = c->consumed[0];
    if ((consumed + n_in) >> 62) { set_error("%s: the position passes 2^62", what); return NVX_ERR_ARG; }
    // every row's last sample read and last word written, in samples of its row (out_end) and in bytes of the whole operand
    const size_t rows = (size_t)c->n_streams;
    size_t out_end, in_bytes, out_bytes;
    if (__builtin_add_overflow(out_first, n_in, &out_end) || !span_bytes(rows - 1, pitch_in, n_in, (size_t)BPS[c->format], &in_bytes) ||
        !span_bytes(rows - 1, pitch_out, out_end, 4, &out_bytes)) {
        set_error("%s: the span of %zu samples of %d streams at pitch %zu, or of as many words from %zu at pitch %zu, overflows", what, n_in,
                  c->n_streams, pitch_in, out_first, pitch_out);
        return NVX_ERR_ARG;
    }
    if ((rows > 1 && (n_in > pitch_in || ((pitch_in * (size_t)BPS[c->format]) & 15))) || (rows > 1 && out_end > pitch_out)) {
        set_error("%s: %zu samples per stream at pitch %zu, words up to %zu at pitch %zu (a row must hold them, and input rows are 16-byte aligned)",
                  what, n_in, pitch_in, out_end, pitch_out);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_in, in_bytes, what, "input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out, out_bytes, what, "output")) != NVX_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    // the state rows of streams pushed one by one are brought to stream 0's parity
    const int parity = c->parity[0];
    for (int i = 1; i < c->n_streams; i++)
        if (c->parity[i] != parity) {
            HIP_TRY(hipMemcpyAsync(c->d_state[parity] + (size_t)i * c->state_words, c->d_state[parity ^ 1] + (size_t)i * c->state_words,
                                   (size_t)c->state_words * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
            c->parity[i] = (uint8_t)parity;
        }
    return launch(c, 0, c->n_streams, consumed, parity, d_in, pitch_in, n_in, (uint32_t *)d_out, pitch_out, out_first, s);
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
    if ((consumed + n_in) >> 62) { set_error("%s: the position passes 2^62", what); return NVX_ERR_ARG; }
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    const size_t in_bytes = n_in * (size_t)BPS[c->format];
    if (in_bytes > c->push_in_cap) {
        (void)hipFree(c->d_push_in); c->d_push_in = nullptr; c->push_in_cap = 0;
        if (hipMalloc(&c->d_push_in, in_bytes) != hipSuccess) { set_error("%s: hipMalloc of %zu bytes failed", what, in_bytes); return NVX_ERR_NOMEM; }
        c->push_in_cap = in_bytes;
    }
    if (n_in > c->push_out_cap) {
        (void)hipFree(c->d_push_out); c->d_push_out = nullptr; c->push_out_cap = 0;
        if (hipMalloc((void **)&c->d_push_out, n_in * 4) != hipSuccess) { set_error("%s: hipMalloc of %zu bytes failed", what, n_in * 4); return NVX_ERR_NOMEM; }
        c->push_out_cap = n_in;
    }
    HIP_TRY(hipMemcpy(c->d_push_in, in, in_bytes, hipMemcpyHostToDevice));
    if ((rc = launch(c, stream, 1, consumed, c->parity[stream], c->d_push_in, n_in, n_in, c->d_push_out, n_in, 0, nullptr)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(out_iq, c->d_push_out, n_in * 4, hipMemcpyDeviceToHost));     // waits for the null stream
    return NVX_OK;
}
