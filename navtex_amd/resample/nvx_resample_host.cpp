// nvx_resample_host.cpp -- the resampler's entry points (include/navtex_amd_resample.h): the design without a device,
// the config checks, the choice of kernel form.  The plan, its carried positions, the launch arithmetic and the checks of a
// call are nvx_rs_host.h's, which the down-converter bank compiles too; HIP-event timing is nvx_companion.h's.  The library
// stands alone: it shares no state with libnavtex_amd.so.
#include <cstring>
#include <new>

#include "nvx_rs_host.h"

extern "C" const char *nvx_resample_last_error(void) { return nvx_error_text(); }

static const uint32_t MAGIC = 0x4e525331u;      // "NRS1"

struct nvx_resampler {
    uint32_t magic = MAGIC;
    nvx_rs_plan p{ "the resampler", "stream" };
    int form = 0;
    struct { int K, tiles, tiles_per_chunk, chunks, taps_in_lds; size_t lds_bytes; } last = {};      // nvx_resample_debug_last_launch
    int64_t kernel_launches = 0;
};

static bool valid(const nvx_resampler *r, const char *what)
{
    if (!r || r->magic != MAGIC) { set_error("%s: not a resampler", what); return false; }
    return true;
}

// ------------------------------------------------------------------------------------------------------ without a device
extern "C" int nvx_resample_design(uint32_t input_rate_hz, int *L, int *M, int *T, int *S, int16_t *taps, int cap)
{
    int l, m, t;
    const char *why = "";
    if (nvx_rs_plan_numbers(input_rate_hz, &l, &m, &t, &why) != NVX_OK) { set_error("nvx_resample_design: %u S/s: %s", input_rate_hz, why); return NVX_ERR_ARG; }
    if (cap < 0) { set_error("nvx_resample_design: cap %d", cap); return NVX_ERR_ARG; }
    if (L) *L = l;
    if (M) *M = m;
    if (T) *T = t;
    if (S) *S = NVX_RS_SHIFT;
    if (taps && cap >= l * t) {
        const int rc = nvx_rs_plan_taps(input_rate_hz, l, t, taps, &why);
        if (rc != NVX_OK) { set_error("nvx_resample_design: %u S/s: %s", input_rate_hz, why); return rc; }
    }
    return l * t;
}

extern "C" int64_t nvx_resample_out_count(uint32_t input_rate_hz, uint64_t consumed_before, uint64_t n_in)
{
    int l, m, t;
    const char *why = "";
    if (nvx_rs_plan_numbers(input_rate_hz, &l, &m, &t, &why) != NVX_OK) { set_error("nvx_resample_out_count: %u S/s: %s", input_rate_hz, why); return -1; }
    uint64_t end;
    if (__builtin_add_overflow(consumed_before, n_in, &end) || end >> 63) { set_error("nvx_resample_out_count: the position passes 2^63"); return -1; }
    return (int64_t)(nvx_rs_outputs_after(end, l, m) - nvx_rs_outputs_after(consumed_before, l, m));
}

extern "C" void nvx_resample_config_default(nvx_resample_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0; cfg->n_streams = 1; cfg->input_rate_hz = 2048000; cfg->format = NVX_RS_CS16;
}

// --------------------------------------------------------------------------------------------------------------- plans
static void release(nvx_resampler *r)
{
    nvx_rs_plan_release(r->p);
    r->magic = 0;
    delete r;
}

extern "C" int nvx_resample_create(const nvx_resample_config *cfg, nvx_resampler **out)
{
    const char *what = "nvx_resample_create";
    if (!cfg || !out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    *out = nullptr;
    if (cfg->struct_size != sizeof *cfg) { set_error("%s: struct_size %u, this library's nvx_resample_config has %zu bytes", what, cfg->struct_size, sizeof *cfg); return NVX_ERR_ARG; }
    if (cfg->n_streams < 1 || cfg->n_streams > 65535) { set_error("%s: n_streams %d (1 .. 65535)", what, cfg->n_streams); return NVX_ERR_ARG; }
    if (cfg->format < NVX_RS_CS16 || cfg->format > NVX_RS_CF32) { set_error("%s: format %d (NVX_RS_CS16 .. NVX_RS_CF32)", what, cfg->format); return NVX_ERR_ARG; }
    if (cfg->device < 0) { set_error("%s: device %d", what, cfg->device); return NVX_ERR_ARG; }
    nvx_resampler *r = new (std::nothrow) nvx_resampler;
    if (!r) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    const int rc = nvx_rs_plan_create(r->p, what, cfg->device, cfg->n_streams, cfg->format, cfg->input_rate_hz);
    if (rc != NVX_OK) { release(r); return rc; }
    nvx_rs_prepare();
    *out = r;
    return NVX_OK;
}

extern "C" void nvx_resample_destroy(nvx_resampler *r)
{
    if (!r || r->magic != MAGIC) return;
    (void)hipSetDevice(r->p.device);
    (void)hipDeviceSynchronize();
    release(r);
}

extern "C" int nvx_resample_plan(nvx_resampler *r, int *L, int *M, int *T, int *n_streams, int *format)
{
    if (!valid(r, "nvx_resample_plan")) return NVX_ERR_ARG;
    if (L) *L = r->p.L;
    if (M) *M = r->p.M;
    if (T) *T = r->p.T;
    if (n_streams) *n_streams = r->p.n_inputs;
    if (format) *format = r->p.format;
    return NVX_OK;
}

extern "C" int nvx_resample_reset(nvx_resampler *r, int stream)
{
    return valid(r, "nvx_resample_reset") ? nvx_rs_reset(r->p, "nvx_resample_reset", stream) : NVX_ERR_ARG;
}

extern "C" int nvx_resample_position(nvx_resampler *r, int stream, uint64_t *consumed, uint64_t *produced)
{
    return valid(r, "nvx_resample_position") ? nvx_rs_position(r->p, "nvx_resample_position", stream, consumed, produced) : NVX_ERR_ARG;
}

extern "C" int nvx_resample_set_form(nvx_resampler *r, int form)
{
    if (!valid(r, "nvx_resample_set_form")) return NVX_ERR_ARG;
    if (form < 0 || form > 2) { set_error("nvx_resample_set_form: form %d (0, 1 or 2)", form); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(r->p.mu);
    r->form = form;
    return NVX_OK;
}

extern "C" int nvx_resample_timing(nvx_resampler *r, int enable)
{
    return valid(r, "nvx_resample_timing") ? timing_enable(r->p.mu, r->p.timer, enable) : NVX_ERR_ARG;
}

extern "C" int nvx_resample_time_stats(nvx_resampler *r, double *sum_ms, uint64_t *launches, int reset)
{
    return valid(r, "nvx_resample_time_stats") ? timing_collect(r->p.mu, r->p.timer, sum_ms, launches, reset) : NVX_ERR_ARG;
}

extern "C" int64_t nvx_resample_debug_last_launch(nvx_resampler *r, int *K, int *tiles, int *tiles_per_chunk, int *chunks,
                                                  int *taps_in_lds, size_t *lds_bytes)
{
    if (!valid(r, "nvx_resample_debug_last_launch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(r->p.mu);
    if (r->kernel_launches) {
        if (K) *K = r->last.K;
        if (tiles) *tiles = r->last.tiles;
        if (tiles_per_chunk) *tiles_per_chunk = r->last.tiles_per_chunk;
        if (chunks) *chunks = r->last.chunks;
        if (taps_in_lds) *taps_in_lds = r->last.taps_in_lds;
        if (lds_bytes) *lds_bytes = r->last.lds_bytes;
    }
    return r->kernel_launches;
}

// ------------------------------------------------------------------------------------------------------------ launches
// One launch over streams [first_stream, first_stream + n_streams) of the plan, which stand at c.consumed and read history
// row c.parity; the caller holds the plan's lock and has checked every span.
static int launch(nvx_resampler *r, int first_stream, int n_streams, const nvx_rs_call &c, const void *d_in, size_t pitch_in, size_t n_in,
                  uint32_t *d_out, size_t pitch_out, size_t out_first, hipStream_t s)
{
    nvx_rs_plan &p = r->p;
    // a workgroup per stream fills the chip from a few workgroups per CU on; below that a stream's tiles are spread out
    const int form = r->form ? r->form : (n_streams >= 1024 ? 1 : 2);
    nvx_rs_args a;
    const int chunks = nvx_rs_fill_args(p, first_stream, c.consumed, c.parity, d_in, pitch_in, n_in, d_out, pitch_out, out_first, c.outs,
                                        form == 2 ? (NVX_RS_TARGET_WORKGROUPS + n_streams - 1) / n_streams : 1, &a);
    nvx_event_timer::events ev;
    int rc;
    if ((rc = p.timer.begin(s, ev)) != NVX_OK) return rc;
    HIP_TRY(nvx_rs_launch(&a, p.format, n_streams, chunks, p.taps_in_lds, s));
    r->last = { a.K, a.tiles, a.tiles_per_chunk, chunks, p.taps_in_lds ? 1 : 0, nvx_rs_lds_bytes(&a, p.taps_in_lds) };
    r->kernel_launches++;
    if ((rc = p.timer.end(s, ev)) != NVX_OK) return rc;
    nvx_rs_advance(p, first_stream, n_streams, n_in, c);
    return NVX_OK;
}

extern "C" int nvx_resample_resident(nvx_resampler *r, const void *d_in, size_t pitch_in, size_t n_in, void *d_out,
                                     size_t pitch_out, size_t out_first, size_t *n_out, void *hip_stream)
{
    const char *what = "nvx_resample_resident";
    if (!valid(r, what)) return NVX_ERR_ARG;
    nvx_rs_plan &p = r->p;
    std::lock_guard<std::mutex> lk(p.mu);
    nvx_rs_call c;
    int rc;
    if ((rc = nvx_rs_resident_open(p, what, d_in, n_in, d_out, &c)) != NVX_OK) return rc;
    if (!nvx_rs_resident_spans(p, (size_t)p.n_inputs, pitch_in, n_in, pitch_out, out_first, &c)) {
        set_error("%s: the span of %zu samples of %d streams at pitch %zu, or of %zu outputs from %zu at pitch %zu, overflows", what, n_in,
                  p.n_inputs, pitch_in, c.outs, out_first, pitch_out);
        return NVX_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    if ((rc = nvx_rs_resident_ready(p, what, (size_t)p.n_inputs, d_in, pitch_in, n_in, d_out, pitch_out, c, s)) != NVX_OK) return rc;
    if (n_in && (rc = launch(r, 0, p.n_inputs, c, d_in, pitch_in, n_in, (uint32_t *)d_out, pitch_out, out_first, s)) != NVX_OK) return rc;
    if (n_out) *n_out = c.outs;
    return NVX_OK;
}

extern "C" int nvx_resample_push(nvx_resampler *r, int stream, const void *in, size_t n_in, int16_t *out_iq, size_t cap_samples, size_t *n_out)
{
    const char *what = "nvx_resample_push";
    if (!valid(r, what)) return NVX_ERR_ARG;
    nvx_rs_plan &p = r->p;
    std::lock_guard<std::mutex> lk(p.mu);
    nvx_rs_call c;
    int rc;
    if ((rc = nvx_rs_push_open(p, what, stream, in, n_in, out_iq, cap_samples, &c)) != NVX_OK) return rc;
    if (c.outs > cap_samples || c.outs > 0x7fffffffu) {
        set_error("%s: %zu samples give %zu outputs, the buffer holds %zu: nothing consumed", what, n_in, c.outs, cap_samples);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) { if (n_out) *n_out = 0; return NVX_OK; }
    const size_t out_words = c.outs ? c.outs : 1;
    if ((rc = nvx_rs_push_stage(p, what, in, n_in, out_words)) != NVX_OK) return rc;
    if ((rc = launch(r, stream, 1, c, p.push.d_in, n_in, n_in, p.push.d_out, out_words, 0, nullptr)) != NVX_OK) return rc;
    if (c.outs) HIP_TRY(hipMemcpy(out_iq, p.push.d_out, c.outs * 4, hipMemcpyDeviceToHost));     // waits for the null stream
    else HIP_TRY(hipStreamSynchronize(nullptr));
    if (n_out) *n_out = c.outs;
    return NVX_OK;
}
