// nvx_ddc_host.cpp -- the down-converter bank's entry points (include/navtex_amd_ddc.h): the grid rule, the config
// checks, the carried shifts, the choice of launch shape.  The plan, its carried positions, the launch arithmetic and the
// checks of a call are the resampler's (navtex_amd/resample/nvx_rs_host.h), compiled into this library as its design
// (nvx_resample_design.c) is: code, not a library.  HIP-event timing is nvx_companion.h's.  The library stands alone: it shares no state with the
// other three.
#include <cmath>
#include <cstring>
#include <new>

#include "nvx_ddc_plan.h"
#include "nvx_ddc_table.h"
#include "nvx_rs_host.h"

extern "C" const char *nvx_ddc_last_error(void) { return nvx_error_text(); }

static const uint32_t MAGIC = 0x4e444431u;      // "NDD1"
static const int MANY_ROWS = 1024;              // from here on a workgroup per output row fills the chip

struct nvx_ddc {
    uint32_t magic = MAGIC;
    nvx_rs_plan p{ "the down-converter bank", "input" };
    int n_slices = 0;
    uint32_t *d_table = nullptr;
    int *d_k = nullptr, *h_k = nullptr;          // the shifts on the device, and the pinned row they are uploaded from
    hipEvent_t k_uploaded = nullptr;             // recorded behind the last upload: h_k is not rewritten before it
    bool k_dirty = false;
    std::vector<int> k;                          // [n_inputs][n_slices]
    struct { int K, tiles, tiles_per_chunk, chunks, slices, inputs, taps_in_lds; size_t lds_bytes; } last = {};
    int64_t kernel_launches = 0;
};

static bool valid(const nvx_ddc *d, const char *what)
{
    if (!d || d->magic != MAGIC) { set_error("%s: not a down-converter bank", what); return false; }
    return true;
}

// ------------------------------------------------------------------------------------------------------ without a device
// k = rint(hz N / fi), ties to even, decided on the exact remainder hz N - k fi (hz N is exact: N is a power of two)
static int grid_k(uint32_t fi, double hz, int *k_out, const char *what)
{
    int l, m, t;
    const char *why = "";
    if (nvx_rs_plan_numbers(fi, &l, &m, &t, &why) != NVX_OK) { set_error("%s: %u S/s: %s", what, fi, why); return NVX_ERR_ARG; }
    if (!std::isfinite(hz) || std::fabs(hz) > (double)fi) { set_error("%s: a shift of %g Hz at %u S/s", what, hz, fi); return NVX_ERR_ARG; }
    const double num = hz * NVX_DDC_GRID, half = fi / 2.0;
    long k = std::lrint(num / fi);
    const double rem = std::fma(-(double)k, (double)fi, num);       // exact: num and k fi lie within a factor of two, or k = 0
    if (rem > half || (rem == half && (k & 1))) k++;
    else if (rem < -half || (rem == -half && (k & 1))) k--;
    // |k fi / N| <= fi / 2 - 25000  <=>  |k| fi <= N (fi / 2 - 25000), in integers
    const int64_t lim = (int64_t)NVX_DDC_GRID * ((int64_t)fi - 2 * NVX_DDC_GUARD_HZ), mag = 2 * (int64_t)(k < 0 ? -k : k) * fi;
    if (mag > lim) {
        set_error("%s: %g Hz is grid step %ld = %g Hz; a slice's +-%d Hz must lie inside the input's band: |shift| <= %g Hz at %u S/s", what, hz, k,
                  (double)k * fi / NVX_DDC_GRID, NVX_DDC_GUARD_HZ, fi / 2.0 - NVX_DDC_GUARD_HZ, fi);
        return NVX_ERR_ARG;
    }
    *k_out = (int)k;
    return NVX_OK;
}

extern "C" int nvx_ddc_grid(uint32_t input_rate_hz, double hz, int *k, double *applied_hz)
{
    int kk;
    const int rc = grid_k(input_rate_hz, hz, &kk, "nvx_ddc_grid");
    if (rc != NVX_OK) return rc;
    if (k) *k = kk;
    if (applied_hz) *applied_hz = (double)kk * input_rate_hz / NVX_DDC_GRID;
    return NVX_OK;
}

extern "C" int nvx_ddc_table(int16_t *cs, int cap_pairs)
{
    if (cs && cap_pairs >= NVX_DDC_GRID)
        for (int j = 0; j < NVX_DDC_GRID; j++) nvx_ddc_w(j, &cs[2 * j], &cs[2 * j + 1]);
    return NVX_DDC_GRID;
}

extern "C" void nvx_ddc_config_default(nvx_ddc_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0; cfg->n_inputs = 1; cfg->n_slices = 1; cfg->input_rate_hz = 2400000; cfg->format = NVX_DDC_CU8;
}

// --------------------------------------------------------------------------------------------------------------- plans
static void release(nvx_ddc *d)
{
    nvx_rs_plan_release(d->p);
    (void)hipFree(d->d_table); (void)hipFree(d->d_k); (void)hipHostFree(d->h_k);
    if (d->k_uploaded) (void)hipEventDestroy(d->k_uploaded);
    d->magic = 0;
    delete d;
}

// the bank's own tables behind the plan's: the mixer's half turn, the shifts and the pinned row they are uploaded from
static int create_tables(nvx_ddc *d, const char *what)
{
    const size_t rows = (size_t)d->p.n_inputs * d->n_slices;
    d->k.assign(rows, 0);
    std::vector<uint32_t> half(NVX_DDC_TAB_DW, 0);
    for (int j = 0; j < NVX_DDC_HALF; j++) {
        int16_t c, s;
        nvx_ddc_w(j, &c, &s);
        half[NVX_DDC_SLOT(j)] = (uint32_t)(uint16_t)c | ((uint32_t)(uint16_t)s << 16);
    }
    hipError_t e = hipMalloc((void **)&d->d_table, half.size() * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d->d_k, rows * sizeof(int));
    if (e == hipSuccess) e = hipHostMalloc((void **)&d->h_k, rows * sizeof(int), hipHostMallocDefault);
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); return NVX_ERR_NOMEM; }
    e = hipEventCreateWithFlags(&d->k_uploaded, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemcpy(d->d_table, half.data(), half.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d->d_k, 0, rows * sizeof(int));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: filling the tables failed: %s", what, hipGetErrorString(e)); return NVX_ERR_HIP; }
    return NVX_OK;
}

extern "C" int nvx_ddc_create(const nvx_ddc_config *cfg, nvx_ddc **out)
{
    const char *what = "nvx_ddc_create";
    if (!cfg || !out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    *out = nullptr;
    if (cfg->struct_size != sizeof *cfg) { set_error("%s: struct_size %u, this library's nvx_ddc_config has %zu bytes", what, cfg->struct_size, sizeof *cfg); return NVX_ERR_ARG; }
    if (cfg->n_inputs < 1 || cfg->n_slices < 1 || cfg->n_inputs > 65535 || cfg->n_slices > 65535 || (int64_t)cfg->n_inputs * cfg->n_slices > 65535) {
        set_error("%s: %d inputs of %d slices (each at least 1, 65535 rows at most)", what, cfg->n_inputs, cfg->n_slices); return NVX_ERR_ARG;
    }
    if (cfg->format < NVX_DDC_CS16 || cfg->format > NVX_DDC_CF32) { set_error("%s: format %d (NVX_DDC_CS16 .. NVX_DDC_CF32)", what, cfg->format); return NVX_ERR_ARG; }
    if (cfg->device < 0) { set_error("%s: device %d", what, cfg->device); return NVX_ERR_ARG; }
    nvx_ddc *d = new (std::nothrow) nvx_ddc;
    if (!d) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    d->n_slices = cfg->n_slices;
    int rc = nvx_rs_plan_create(d->p, what, cfg->device, cfg->n_inputs, cfg->format, cfg->input_rate_hz);
    if (rc == NVX_OK) rc = create_tables(d, what);
    if (rc != NVX_OK) { release(d); return rc; }
    nvx_ddc_prepare();
    *out = d;
    return NVX_OK;
}

extern "C" void nvx_ddc_destroy(nvx_ddc *d)
{
    if (!d || d->magic != MAGIC) return;
    (void)hipSetDevice(d->p.device);
    (void)hipDeviceSynchronize();
    release(d);
}

extern "C" int nvx_ddc_plan(nvx_ddc *d, int *L, int *M, int *T, int *n_inputs, int *n_slices, int *format)
{
    if (!valid(d, "nvx_ddc_plan")) return NVX_ERR_ARG;
    if (L) *L = d->p.L;
    if (M) *M = d->p.M;
    if (T) *T = d->p.T;
    if (n_inputs) *n_inputs = d->p.n_inputs;
    if (n_slices) *n_slices = d->n_slices;
    if (format) *format = d->p.format;
    return NVX_OK;
}

extern "C" int nvx_ddc_set_shift(nvx_ddc *d, int input, int slice, double hz, double *applied_hz)
{
    const char *what = "nvx_ddc_set_shift";
    if (!valid(d, what)) return NVX_ERR_ARG;
    if (input < -1 || input >= d->p.n_inputs || slice < 0 || slice >= d->n_slices) {
        set_error("%s: input %d of %d, slice %d of %d", what, input, d->p.n_inputs, slice, d->n_slices); return NVX_ERR_ARG;
    }
    int k;
    const int rc = grid_k(d->p.rate, hz, &k, what);
    if (rc != NVX_OK) return rc;
    std::lock_guard<std::mutex> lk(d->p.mu);
    for (int i = input < 0 ? 0 : input; i < (input < 0 ? d->p.n_inputs : input + 1); i++) d->k[(size_t)i * d->n_slices + slice] = k;
    d->k_dirty = true;
    if (applied_hz) *applied_hz = (double)k * d->p.rate / NVX_DDC_GRID;
    return NVX_OK;
}

extern "C" int nvx_ddc_get_shift(nvx_ddc *d, int input, int slice, int *k, double *applied_hz)
{
    const char *what = "nvx_ddc_get_shift";
    if (!valid(d, what)) return NVX_ERR_ARG;
    if (input < 0 || input >= d->p.n_inputs || slice < 0 || slice >= d->n_slices) {
        set_error("%s: input %d of %d, slice %d of %d", what, input, d->p.n_inputs, slice, d->n_slices); return NVX_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(d->p.mu);
    const int kk = d->k[(size_t)input * d->n_slices + slice];
    if (k) *k = kk;
    if (applied_hz) *applied_hz = (double)kk * d->p.rate / NVX_DDC_GRID;
    return NVX_OK;
}

extern "C" int nvx_ddc_reset(nvx_ddc *d, int input)
{
    return valid(d, "nvx_ddc_reset") ? nvx_rs_reset(d->p, "nvx_ddc_reset", input) : NVX_ERR_ARG;
}

extern "C" int nvx_ddc_debug_set_position(nvx_ddc *d, int input, uint64_t consumed)
{
    const char *what = "nvx_ddc_debug_set_position";
    if (!valid(d, what)) return NVX_ERR_ARG;
    if (input < -1 || input >= d->p.n_inputs || consumed >> 62) { set_error("%s: input %d of %d, position %llu (below 2^62)", what, input, d->p.n_inputs, (unsigned long long)consumed); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(d->p.mu);
    int rc;
    if ((rc = select_device(d->p.device, d->p.library)) != NVX_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    for (int i = input < 0 ? 0 : input; i < (input < 0 ? d->p.n_inputs : input + 1); i++) {
        for (int row = 0; row < 2; row++) HIP_TRY(hipMemset(d->p.hist.in(i, row), 0, d->p.hist.bytes(1)));     // silence in front
        d->p.consumed[i] = consumed;
    }
    HIP_TRY(hipDeviceSynchronize());
    return NVX_OK;
}

extern "C" int nvx_ddc_position(nvx_ddc *d, int input, uint64_t *consumed, uint64_t *produced)
{
    return valid(d, "nvx_ddc_position") ? nvx_rs_position(d->p, "nvx_ddc_position", input, consumed, produced) : NVX_ERR_ARG;
}

extern "C" int nvx_ddc_timing(nvx_ddc *d, int enable)
{
    return valid(d, "nvx_ddc_timing") ? timing_enable(d->p.mu, d->p.timer, enable) : NVX_ERR_ARG;
}

extern "C" int nvx_ddc_time_stats(nvx_ddc *d, double *sum_ms, uint64_t *launches, int reset)
{
    return valid(d, "nvx_ddc_time_stats") ? timing_collect(d->p.mu, d->p.timer, sum_ms, launches, reset) : NVX_ERR_ARG;
}

extern "C" int64_t nvx_ddc_debug_last_launch(nvx_ddc *d, int *K, int *tiles, int *tiles_per_chunk, int *chunks, int *slices,
                                             int *inputs, int *taps_in_lds, size_t *lds_bytes)
{
    if (!valid(d, "nvx_ddc_debug_last_launch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(d->p.mu);
    if (d->kernel_launches) {
        if (K) *K = d->last.K;
        if (tiles) *tiles = d->last.tiles;
        if (tiles_per_chunk) *tiles_per_chunk = d->last.tiles_per_chunk;
        if (chunks) *chunks = d->last.chunks;
        if (slices) *slices = d->last.slices;
        if (inputs) *inputs = d->last.inputs;
        if (taps_in_lds) *taps_in_lds = d->last.taps_in_lds;
        if (lds_bytes) *lds_bytes = d->last.lds_bytes;
    }
    return d->kernel_launches;
}

// ------------------------------------------------------------------------------------------------------------ launches
// The shifts as they stand go to the device in front of the launch, on its stream, from the pinned row; the row is not
// rewritten while an earlier upload may still read it.
static int upload_shifts(nvx_ddc *d, hipStream_t s)
{
    if (!d->k_dirty) return NVX_OK;
    HIP_TRY(hipEventSynchronize(d->k_uploaded));
    memcpy(d->h_k, d->k.data(), d->k.size() * sizeof(int));
    HIP_TRY(hipMemcpyAsync(d->d_k, d->h_k, d->k.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(d->k_uploaded, s));
    d->k_dirty = false;
    return NVX_OK;
}

// One launch over inputs [first_input, first_input + n_inputs) of the plan, every slice of each, which stand at c.consumed
// and read history row c.parity; the caller holds the plan's lock and has checked every span.
static int launch(nvx_ddc *d, int first_input, int n_inputs, const nvx_rs_call &c, const void *d_in, size_t pitch_in, size_t n_in,
                  uint32_t *d_out, size_t pitch_out, size_t out_first, hipStream_t s)
{
    nvx_rs_plan &p = d->p;
    // a workgroup per output row fills the chip from a few workgroups per CU on; below that a row's tiles are spread out
    const int rows = n_inputs * d->n_slices;
    nvx_ddc_args da{};
    const int chunks = nvx_rs_fill_args(p, first_input, c.consumed, c.parity, d_in, pitch_in, n_in, d_out, pitch_out, out_first, c.outs,
                                        rows < MANY_ROWS ? (NVX_RS_TARGET_WORKGROUPS + rows - 1) / rows : 1, &da.rs);
    da.k = d->d_k + (size_t)first_input * d->n_slices; da.table = d->d_table; da.n_slices = d->n_slices;
    da.n0 = (uint32_t)(c.consumed % NVX_DDC_GRID);

    int rc;
    if ((rc = upload_shifts(d, s)) != NVX_OK) return rc;
    nvx_event_timer::events ev;
    if ((rc = p.timer.begin(s, ev)) != NVX_OK) return rc;
    HIP_TRY(nvx_ddc_launch(&da, p.format, n_inputs, chunks, p.taps_in_lds, s));
    d->last = { da.rs.K, da.rs.tiles, da.rs.tiles_per_chunk, chunks, d->n_slices, n_inputs, p.taps_in_lds ? 1 : 0, nvx_ddc_lds_bytes(&da, p.taps_in_lds) };
    d->kernel_launches++;
    if ((rc = p.timer.end(s, ev)) != NVX_OK) return rc;
    nvx_rs_advance(p, first_input, n_inputs, n_in, c);
    return NVX_OK;
}

extern "C" int nvx_ddc_resident(nvx_ddc *d, const void *d_in, size_t pitch_in, size_t n_in, void *d_out, size_t pitch_out,
                                size_t out_first, size_t *n_out, void *hip_stream)
{
    const char *what = "nvx_ddc_resident";
    if (!valid(d, what)) return NVX_ERR_ARG;
    nvx_rs_plan &p = d->p;
    std::lock_guard<std::mutex> lk(p.mu);
    const size_t rows = (size_t)p.n_inputs * d->n_slices;
    nvx_rs_call c;
    int rc;
    if ((rc = nvx_rs_resident_open(p, what, d_in, n_in, d_out, &c)) != NVX_OK) return rc;
    if (!nvx_rs_resident_spans(p, rows, pitch_in, n_in, pitch_out, out_first, &c)) {
        set_error("%s: the span of %zu samples of %d inputs at pitch %zu, or of %zu outputs from %zu of %zu rows at pitch %zu, overflows", what, n_in,
                  p.n_inputs, pitch_in, c.outs, out_first, rows, pitch_out);
        return NVX_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    if ((rc = nvx_rs_resident_ready(p, what, rows, d_in, pitch_in, n_in, d_out, pitch_out, c, s)) != NVX_OK) return rc;
    if (n_in && (rc = launch(d, 0, p.n_inputs, c, d_in, pitch_in, n_in, (uint32_t *)d_out, pitch_out, out_first, s)) != NVX_OK) return rc;
    if (n_out) *n_out = c.outs;
    return NVX_OK;
}

extern "C" int nvx_ddc_push(nvx_ddc *d, int input, const void *in, size_t n_in, int16_t *out_iq, size_t cap_samples, size_t *n_out)
{
    const char *what = "nvx_ddc_push";
    if (!valid(d, what)) return NVX_ERR_ARG;
    nvx_rs_plan &p = d->p;
    std::lock_guard<std::mutex> lk(p.mu);
    nvx_rs_call c;
    int rc;
    if ((rc = nvx_rs_push_open(p, what, input, in, n_in, out_iq, cap_samples, &c)) != NVX_OK) return rc;
    size_t all_words;
    if (c.outs > cap_samples || c.outs > 0x7fffffffu || __builtin_mul_overflow(cap_samples, (size_t)d->n_slices * 4, &all_words)) {
        set_error("%s: %zu samples give %zu outputs per slice, a slice's row holds %zu: nothing consumed", what, n_in, c.outs, cap_samples);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) { if (n_out) *n_out = 0; return NVX_OK; }
    const size_t row_words = c.outs ? c.outs : 1;
    if ((rc = nvx_rs_push_stage(p, what, in, n_in, row_words * d->n_slices)) != NVX_OK) return rc;
    if ((rc = launch(d, input, 1, c, p.push.d_in, n_in, n_in, p.push.d_out, row_words, 0, nullptr)) != NVX_OK) return rc;
    if (c.outs) HIP_TRY(hipMemcpy2D(out_iq, cap_samples * 4, p.push.d_out, row_words * 4, c.outs * 4, (size_t)d->n_slices, hipMemcpyDeviceToHost));     // waits for the null stream
    else HIP_TRY(hipStreamSynchronize(nullptr));
    if (n_out) *n_out = c.outs;
    return NVX_OK;
}
