// nvx_ddc_host.cpp -- the down-converter bank's entry points (include/navtex_amd_ddc.h): the plan, the grid rule, argument
// and span checks, the carried positions and shifts, the choice of launch shape, HIP-event timing.  The library stands
// alone: it shares no state with the other three, and takes the resampler's design (nvx_resample_design.c) as compiled-in
// code, not as a library.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "nvx_ddc_plan.h"
#include "nvx_ddc_table.h"

static thread_local char g_err[512] = "";

static void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

extern "C" const char *nvx_ddc_last_error(void) { return g_err; }

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? NVX_ERR_NODEV : NVX_ERR_HIP; \
        }                                                                                  \
    } while (0)

static const uint32_t MAGIC = 0x4e444431u;      // "NDD1"
static const int BPS[4] = { 4, 2, 2, 8 };
static const int TARGET_WORKGROUPS = 2048;      // few rows: a row's tiles are spread until the grid has about this many
static const int MANY_ROWS = 1024;              // from here on a workgroup per output row fills the chip

struct nvx_ddc {
    uint32_t magic = MAGIC;
    std::mutex mu;
    int device = 0, n_inputs = 0, n_slices = 0, format = 0;
    uint32_t rate = 0;
    int L = 0, M = 0, T = 0, Tp = 0, row_dw = 0, tap_dw = 0, K = 0, hist_pitch = 0;
    bool taps_in_lds = false;
    uint32_t dq = 0, dr = 0;
    uint32_t *d_taps = nullptr, *d_table = nullptr, *d_hist[2] = { nullptr, nullptr };
    int *d_k = nullptr, *h_k = nullptr;          // the shifts on the device, and the pinned row they are uploaded from
    hipEvent_t k_uploaded = nullptr;             // recorded behind the last upload: h_k is not rewritten before it
    bool k_dirty = false;
    std::vector<int> k;                          // [n_inputs][n_slices]
    std::vector<uint64_t> consumed;
    std::vector<uint8_t> parity;                 // which history row the input's next launch reads
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool, pending;
    double sum_ms = 0.0; uint64_t launches = 0;
    void *d_push_in = nullptr; uint32_t *d_push_out = nullptr;     // nvx_ddc_push's staging, grown on demand
    size_t push_in_cap = 0, push_out_cap = 0;
    struct { int K, tiles, tiles_per_chunk, chunks, slices, inputs, taps_in_lds; size_t lds_bytes; } last = {};
    int64_t kernel_launches = 0;
};

static bool valid(const nvx_ddc *d, const char *what)
{
    if (!d || d->magic != MAGIC) { set_error("%s: not a down-converter bank", what); return false; }
    return true;
}

static int select_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        set_error("no HIP device available (%s); the down-converter bank has no CPU path", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return NVX_ERR_NODEV;
    }
    if (device < 0 || device >= n) { set_error("device %d out of range (0..%d)", device, n - 1); return NVX_ERR_ARG; }
    HIP_TRY(hipSetDevice(device));
    return NVX_OK;
}

// [p, p + bytes) against the allocation the runtime knows p to lie in; no verdict (NVX_OK) for a pointer it does not know
static int check_device_span(const void *p, size_t bytes, const char *what)
{
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return NVX_OK; }
    const size_t off = (size_t)((const char *)p - (const char *)base);
    if (off > size || bytes > size - off) {
        set_error("%s: %zu bytes from %p leave the allocation they lie in (%zu bytes from %p): the launch would fault", what, bytes, p, size, (void *)base);
        return NVX_ERR_ARG;
    }
    return NVX_OK;
}

// (a * b + c) * d without wrapping; false on overflow
static bool span_bytes(size_t a, size_t b, size_t c, size_t d, size_t *out)
{
    size_t t;
    return !__builtin_mul_overflow(a, b, &t) && !__builtin_add_overflow(t, c, &t) && !__builtin_mul_overflow(t, d, out);
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
    (void)hipFree(d->d_taps); (void)hipFree(d->d_table); (void)hipFree(d->d_hist[0]); (void)hipFree(d->d_hist[1]);
    (void)hipFree(d->d_k); (void)hipHostFree(d->h_k);
    (void)hipFree(d->d_push_in); (void)hipFree(d->d_push_out);
    if (d->k_uploaded) (void)hipEventDestroy(d->k_uploaded);
    for (auto &p : d->pending) d->pool.push_back(p);
    for (auto &p : d->pool) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    d->magic = 0;
    delete d;
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
    int L, M, T;
    const char *why = "";
    if (nvx_rs_plan_numbers(cfg->input_rate_hz, &L, &M, &T, &why) != NVX_OK) { set_error("%s: %u S/s: %s", what, cfg->input_rate_hz, why); return NVX_ERR_ARG; }
    std::vector<int16_t> taps((size_t)L * T);
    int rc = nvx_rs_plan_taps(cfg->input_rate_hz, L, T, taps.data(), &why);
    if (rc != NVX_OK) { set_error("%s: %u S/s: %s", what, cfg->input_rate_hz, why); return rc; }
    if ((rc = select_device(cfg->device)) != NVX_OK) return rc;
    HIP_TRY(nvx_ddc_prepare());

    nvx_ddc *d = new (std::nothrow) nvx_ddc;
    if (!d) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    d->device = cfg->device; d->n_inputs = cfg->n_inputs; d->n_slices = cfg->n_slices; d->format = cfg->format; d->rate = cfg->input_rate_hz;
    d->L = L; d->M = M; d->T = T;
    // the resampler's tap table and tile (nvx_resample_plan.h)
    d->Tp = (T + NVX_RS_ALIGN - 1 + 3) & ~3;
    d->row_dw = d->Tp / 2 + ((d->Tp / 4) % 2 == 0 ? 2 : 0);
    d->tap_dw = (NVX_RS_ALIGN * L * d->row_dw + 3) & ~3;
    d->taps_in_lds = (size_t)d->tap_dw * 4 <= NVX_RS_TAPS_LDS_MAX;
    d->dq = (uint32_t)(NVX_RS_THREADS * (uint64_t)M / L); d->dr = (uint32_t)(NVX_RS_THREADS * (uint64_t)M % L);
    for (d->K = NVX_RS_MAX_K; d->K > 1; d->K--)
        if (((uint64_t)(NVX_RS_THREADS * d->K - 1) * M) / L + 2 + T + 24 <= NVX_RS_PLANE) break;
    if (((uint64_t)(NVX_RS_THREADS * d->K - 1) * M) / L + 2 + T + 24 > NVX_RS_PLANE) {
        set_error("%s: %u S/s: one tile's input does not fit the kernel's staging area", what, cfg->input_rate_hz);
        release(d); return NVX_ERR_ARG;
    }
    d->hist_pitch = (T - 1 + 3) & ~3;
    d->consumed.assign(d->n_inputs, 0);
    d->parity.assign(d->n_inputs, 0);
    const size_t rows = (size_t)d->n_inputs * d->n_slices;
    d->k.assign(rows, 0);

    std::vector<uint16_t> table((size_t)d->tap_dw * 2, 0);
    for (int sh = 0; sh < NVX_RS_ALIGN; sh++)
        for (int ph = 0; ph < L; ph++)
            for (int i = 0; i < T; i++)
                table[((size_t)(sh * L + ph) * d->row_dw) * 2 + sh + i] = (uint16_t)taps[(size_t)ph * T + (T - 1 - i)];
    std::vector<uint32_t> half(NVX_DDC_TAB_DW, 0);
    for (int j = 0; j < NVX_DDC_HALF; j++) {
        int16_t c, s;
        nvx_ddc_w(j, &c, &s);
        half[NVX_DDC_SLOT(j)] = (uint32_t)(uint16_t)c | ((uint32_t)(uint16_t)s << 16);
    }
    const size_t hist_bytes = (size_t)d->n_inputs * d->hist_pitch * 4;
    hipError_t e = hipMalloc((void **)&d->d_taps, (size_t)d->tap_dw * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d->d_table, half.size() * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d->d_hist[0], hist_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&d->d_hist[1], hist_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&d->d_k, rows * sizeof(int));
    if (e == hipSuccess) e = hipHostMalloc((void **)&d->h_k, rows * sizeof(int), hipHostMallocDefault);
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); release(d); return NVX_ERR_NOMEM; }
    e = hipEventCreateWithFlags(&d->k_uploaded, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemcpy(d->d_taps, table.data(), (size_t)d->tap_dw * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d->d_table, half.data(), half.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d->d_hist[0], 0, hist_bytes);
    if (e == hipSuccess) e = hipMemset(d->d_hist[1], 0, hist_bytes);
    if (e == hipSuccess) e = hipMemset(d->d_k, 0, rows * sizeof(int));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: filling the tables failed: %s", what, hipGetErrorString(e)); release(d); return NVX_ERR_HIP; }
    *out = d;
    return NVX_OK;
}

extern "C" void nvx_ddc_destroy(nvx_ddc *d)
{
    if (!d || d->magic != MAGIC) return;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    release(d);
}

extern "C" int nvx_ddc_plan(nvx_ddc *d, int *L, int *M, int *T, int *n_inputs, int *n_slices, int *format)
{
    if (!valid(d, "nvx_ddc_plan")) return NVX_ERR_ARG;
    if (L) *L = d->L;
    if (M) *M = d->M;
    if (T) *T = d->T;
    if (n_inputs) *n_inputs = d->n_inputs;
    if (n_slices) *n_slices = d->n_slices;
    if (format) *format = d->format;
    return NVX_OK;
}

extern "C" int nvx_ddc_set_shift(nvx_ddc *d, int input, int slice, double hz, double *applied_hz)
{
    const char *what = "nvx_ddc_set_shift";
    if (!valid(d, what)) return NVX_ERR_ARG;
    if (input < -1 || input >= d->n_inputs || slice < 0 || slice >= d->n_slices) {
        set_error("%s: input %d of %d, slice %d of %d", what, input, d->n_inputs, slice, d->n_slices); return NVX_ERR_ARG;
    }
    int k;
    const int rc = grid_k(d->rate, hz, &k, what);
    if (rc != NVX_OK) return rc;
    std::lock_guard<std::mutex> lk(d->mu);
    for (int i = input < 0 ? 0 : input; i < (input < 0 ? d->n_inputs : input + 1); i++) d->k[(size_t)i * d->n_slices + slice] = k;
    d->k_dirty = true;
    if (applied_hz) *applied_hz = (double)k * d->rate / NVX_DDC_GRID;
    return NVX_OK;
}

extern "C" int nvx_ddc_get_shift(nvx_ddc *d, int input, int slice, int *k, double *applied_hz)
{
    const char *what = "nvx_ddc_get_shift";
    if (!valid(d, what)) return NVX_ERR_ARG;
    if (input < 0 || input >= d->n_inputs || slice < 0 || slice >= d->n_slices) {
        set_error("%s: input %d of %d, slice %d of %d", what, input, d->n_inputs, slice, d->n_slices); return NVX_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(d->mu);
    const int kk = d->k[(size_t)input * d->n_slices + slice];
    if (k) *k = kk;
    if (applied_hz) *applied_hz = (double)kk * d->rate / NVX_DDC_GRID;
    return NVX_OK;
}

extern "C" int nvx_ddc_reset(nvx_ddc *d, int input)
{
    if (!valid(d, "nvx_ddc_reset")) return NVX_ERR_ARG;
    if (input < -1 || input >= d->n_inputs) { set_error("nvx_ddc_reset: input %d of %d", input, d->n_inputs); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(d->mu);
    // an input at position 0 has silence in front: its history rows are not read before they are written again
    for (int i = input < 0 ? 0 : input; i < (input < 0 ? d->n_inputs : input + 1); i++) d->consumed[i] = 0;
    return NVX_OK;
}

extern "C" int nvx_ddc_debug_set_position(nvx_ddc *d, int input, uint64_t consumed)
{
    const char *what = "nvx_ddc_debug_set_position";
    if (!valid(d, what)) return NVX_ERR_ARG;
    if (input < -1 || input >= d->n_inputs || consumed >> 62) { set_error("%s: input %d of %d, position %llu (below 2^62)", what, input, d->n_inputs, (unsigned long long)consumed); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(d->mu);
    int rc;
    if ((rc = select_device(d->device)) != NVX_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    for (int i = input < 0 ? 0 : input; i < (input < 0 ? d->n_inputs : input + 1); i++) {
        for (int p = 0; p < 2; p++) HIP_TRY(hipMemset(d->d_hist[p] + (size_t)i * d->hist_pitch, 0, (size_t)d->hist_pitch * 4));     // silence in front
        d->consumed[i] = consumed;
    }
    HIP_TRY(hipDeviceSynchronize());
    return NVX_OK;
}

extern "C" int nvx_ddc_position(nvx_ddc *d, int input, uint64_t *consumed, uint64_t *produced)
{
    if (!valid(d, "nvx_ddc_position")) return NVX_ERR_ARG;
    if (input < 0 || input >= d->n_inputs) { set_error("nvx_ddc_position: input %d of %d", input, d->n_inputs); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(d->mu);
    if (consumed) *consumed = d->consumed[input];
    if (produced) *produced = nvx_rs_outputs_after(d->consumed[input], d->L, d->M);
    return NVX_OK;
}

extern "C" int nvx_ddc_timing(nvx_ddc *d, int enable)
{
    if (!valid(d, "nvx_ddc_timing")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(d->mu);
    d->timing = enable != 0;
    return NVX_OK;
}

extern "C" int nvx_ddc_time_stats(nvx_ddc *d, double *sum_ms, uint64_t *launches, int reset)
{
    if (!valid(d, "nvx_ddc_time_stats")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(d->mu);
    for (auto &p : d->pending) {
        HIP_TRY(hipEventSynchronize(p.second));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
        d->sum_ms += ms; d->launches++;
        d->pool.push_back(p);
    }
    d->pending.clear();
    if (sum_ms) *sum_ms = d->sum_ms;
    if (launches) *launches = d->launches;
    if (reset) { d->sum_ms = 0.0; d->launches = 0; }
    return NVX_OK;
}

extern "C" int64_t nvx_ddc_debug_last_launch(nvx_ddc *d, int *K, int *tiles, int *tiles_per_chunk, int *chunks, int *slices,
                                             int *inputs, int *taps_in_lds, size_t *lds_bytes)
{
    if (!valid(d, "nvx_ddc_debug_last_launch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(d->mu);
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

// One launch over inputs [first_input, first_input + n_inputs) of the plan, every slice of each, which stand at `consumed`
// and read history row `parity`; the caller holds d->mu and has checked every span.
static int launch(nvx_ddc *d, int first_input, int n_inputs, uint64_t consumed, int parity, const void *d_in, size_t pitch_in,
                  size_t n_in, uint32_t *d_out, size_t pitch_out, size_t out_first, size_t n_out, hipStream_t s)
{
    nvx_ddc_args da{};
    nvx_rs_args &a = da.rs;
    a.in = d_in; a.pitch_in = pitch_in; a.out = d_out; a.pitch_out = pitch_out; a.out_first = out_first;
    a.hist_in = d->d_hist[parity] + (size_t)first_input * d->hist_pitch;
    a.hist_out = d->d_hist[parity ^ 1] + (size_t)first_input * d->hist_pitch;
    a.taps = d->d_taps;
    a.hist_pitch = d->hist_pitch; a.hist_valid = consumed > 0;
    a.n_in = (int)n_in; a.n_out = (int)n_out;
    a.L = d->L; a.M = d->M; a.T = d->T; a.Tp = d->Tp; a.row_dw = d->row_dw; a.tap_dw = d->tap_dw; a.K = d->K;
    a.dq = d->dq; a.dr = d->dr;
    da.k = d->d_k + (size_t)first_input * d->n_slices; da.table = d->d_table; da.n_slices = d->n_slices;
    da.n0 = (uint32_t)(consumed % NVX_DDC_GRID);
    // output 0 of the call is the input's output n0 = ceil(consumed L / M): n0 M = Q0 L + r0, and Q0 >= consumed
    const uint64_t n0 = nvx_rs_outputs_after(consumed, d->L, d->M);
    const unsigned __int128 pos = (unsigned __int128)n0 * (unsigned)d->M;
    a.r0 = (uint32_t)(pos % (unsigned)d->L);
    a.qoff = (int)((uint64_t)(pos / (unsigned)d->L) - consumed);
    const int tile_out = NVX_RS_THREADS * d->K;
    a.tiles = (int)((n_out + tile_out - 1) / tile_out);
    // a workgroup per output row fills the chip from a few workgroups per CU on; below that a row's tiles are spread out
    const int rows = n_inputs * d->n_slices;
    int chunks = 1;
    if (rows < MANY_ROWS && a.tiles > 1) {
        chunks = (TARGET_WORKGROUPS + rows - 1) / rows;
        if (chunks > a.tiles) chunks = a.tiles;
    }
    a.tiles_per_chunk = a.tiles ? (a.tiles + chunks - 1) / chunks : 1;
    chunks = a.tiles ? (a.tiles + a.tiles_per_chunk - 1) / a.tiles_per_chunk : 1;
    // the steps the kernel advances its positions by, as (div L, mod L)
    const uint64_t uL = (uint64_t)d->L, tile_pos = (uint64_t)tile_out * d->M, chunk_pos = tile_pos * (uint64_t)a.tiles_per_chunk;
    a.tile_dq = (uint32_t)(tile_pos / uL); a.tile_dr = (uint32_t)(tile_pos % uL);
    a.chunk_dq = (uint32_t)(chunk_pos / uL); a.chunk_dr = (uint32_t)(chunk_pos % uL);
    a.span_q = (uint32_t)((tile_pos - d->M) / uL); a.span_r = (uint32_t)((tile_pos - d->M) % uL);
    a.m_div = (uint32_t)(d->M / d->L); a.m_mod = (uint32_t)(d->M % d->L);

    int rc;
    if ((rc = upload_shifts(d, s)) != NVX_OK) return rc;
    std::pair<hipEvent_t, hipEvent_t> ev{ nullptr, nullptr };
    const bool timed = d->timing;
    if (timed) {
        if (d->pool.empty()) { HIP_TRY(hipEventCreate(&ev.first)); HIP_TRY(hipEventCreate(&ev.second)); }
        else { ev = d->pool.back(); d->pool.pop_back(); }
        HIP_TRY(hipEventRecord(ev.first, s));
    }
    HIP_TRY(nvx_ddc_launch(&da, d->format, n_inputs, chunks, d->taps_in_lds, s));
    d->last = { a.K, a.tiles, a.tiles_per_chunk, chunks, d->n_slices, n_inputs, d->taps_in_lds ? 1 : 0, nvx_ddc_lds_bytes(&da, d->taps_in_lds) };
    d->kernel_launches++;
    if (timed) { HIP_TRY(hipEventRecord(ev.second, s)); d->pending.push_back(ev); }
    return NVX_OK;
}

extern "C" int nvx_ddc_resident(nvx_ddc *d, const void *d_in, size_t pitch_in, size_t n_in, void *d_out, size_t pitch_out,
                                size_t out_first, size_t *n_out, void *hip_stream)
{
    const char *what = "nvx_ddc_resident";
    if (!valid(d, what)) return NVX_ERR_ARG;
    const size_t bps = (size_t)BPS[d->format];
    if (!d_in || !d_out || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 3) || n_in > NVX_RS_MAX_IN) {
        set_error("%s: bad argument (null pointer, input not 16-byte aligned, output not 4-byte aligned, or more than 2^30 samples)", what);
        return NVX_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(d->mu);
    const uint64_t consumed = d->consumed[0];
    for (int i = 1; i < d->n_inputs; i++)
        if (d->consumed[i] != consumed) {
            set_error("%s: input %d stands at %llu, input 0 at %llu: all inputs of a call stand at the same position", what, i,
                      (unsigned long long)d->consumed[i], (unsigned long long)consumed);
            return NVX_ERR_STATE;
        }
    if ((consumed + n_in) >> 62) { set_error("%s: the position passes 2^62", what); return NVX_ERR_ARG; }
    const size_t outs = (size_t)(nvx_rs_outputs_after(consumed + n_in, d->L, d->M) - nvx_rs_outputs_after(consumed, d->L, d->M));
    const size_t rows = (size_t)d->n_inputs * d->n_slices;
    // every row's last sample read and last word written, in samples of its row and in bytes of the whole operand
    size_t out_end, in_bytes, out_bytes;
    if (__builtin_add_overflow(out_first, outs, &out_end) || outs > 0x7fffffffu ||
        !span_bytes((size_t)(d->n_inputs - 1), pitch_in, n_in, bps, &in_bytes) ||
        !span_bytes(rows - 1, pitch_out, out_end, 4, &out_bytes)) {
        set_error("%s: the span of %zu samples of %d inputs at pitch %zu, or of %zu outputs from %zu of %zu rows at pitch %zu, overflows", what, n_in,
                  d->n_inputs, pitch_in, outs, out_first, rows, pitch_out);
        return NVX_ERR_ARG;
    }
    if ((d->n_inputs > 1 && (n_in > pitch_in || ((pitch_in * bps) & 15))) || (rows > 1 && out_end > pitch_out)) {
        set_error("%s: %zu samples per input at pitch %zu, outputs up to %zu at pitch %zu (a row must hold them, and input rows are 16-byte aligned)",
                  what, n_in, pitch_in, out_end, pitch_out);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) { if (n_out) *n_out = 0; return NVX_OK; }
    int rc;
    if ((rc = select_device(d->device)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_in, in_bytes, "nvx_ddc_resident: input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out, out_bytes, "nvx_ddc_resident: output")) != NVX_OK) return rc;

    hipStream_t s = (hipStream_t)hip_stream;
    // inputs pushed one by one may read different history rows: bring them to input 0's
    const int parity = d->parity[0];
    for (int i = 1; i < d->n_inputs; i++)
        if (d->parity[i] != parity) {
            HIP_TRY(hipMemcpyAsync(d->d_hist[parity] + (size_t)i * d->hist_pitch, d->d_hist[parity ^ 1] + (size_t)i * d->hist_pitch,
                                   (size_t)d->hist_pitch * 4, hipMemcpyDeviceToDevice, s));
            d->parity[i] = (uint8_t)parity;
        }
    if ((rc = launch(d, 0, d->n_inputs, consumed, parity, d_in, pitch_in, n_in, (uint32_t *)d_out, pitch_out, out_first, outs, s)) != NVX_OK) return rc;
    for (int i = 0; i < d->n_inputs; i++) { d->consumed[i] = consumed + n_in; d->parity[i] = (uint8_t)(parity ^ 1); }
    if (n_out) *n_out = outs;
    return NVX_OK;
}

extern "C" int nvx_ddc_push(nvx_ddc *d, int input, const void *in, size_t n_in, int16_t *out_iq, size_t cap_samples, size_t *n_out)
{
    const char *what = "nvx_ddc_push";
    if (!valid(d, what)) return NVX_ERR_ARG;
    if (input < 0 || input >= d->n_inputs || !in || (!out_iq && cap_samples) || n_in > NVX_RS_MAX_IN) {
        set_error("%s: bad argument (input %d of %d, null pointer, or more than 2^30 samples)", what, input, d->n_inputs);
        return NVX_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(d->mu);
    const uint64_t consumed = d->consumed[input];
    if ((consumed + n_in) >> 62) { set_error("%s: the position passes 2^62", what); return NVX_ERR_ARG; }
    const size_t outs = (size_t)(nvx_rs_outputs_after(consumed + n_in, d->L, d->M) - nvx_rs_outputs_after(consumed, d->L, d->M));
    size_t all_words;
    if (outs > cap_samples || outs > 0x7fffffffu || __builtin_mul_overflow(cap_samples, (size_t)d->n_slices * 4, &all_words)) {
        set_error("%s: %zu samples give %zu outputs per slice, a slice's row holds %zu: nothing consumed", what, n_in, outs, cap_samples);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) { if (n_out) *n_out = 0; return NVX_OK; }
    int rc;
    if ((rc = select_device(d->device)) != NVX_OK) return rc;
    const size_t in_bytes = n_in * (size_t)BPS[d->format], row_words = outs ? outs : 1, out_words = row_words * d->n_slices;
    if (in_bytes > d->push_in_cap) {
        (void)hipFree(d->d_push_in); d->d_push_in = nullptr; d->push_in_cap = 0;
        if (hipMalloc(&d->d_push_in, in_bytes) != hipSuccess) { set_error("%s: hipMalloc of %zu bytes failed", what, in_bytes); return NVX_ERR_NOMEM; }
        d->push_in_cap = in_bytes;
    }
    if (out_words > d->push_out_cap) {
        (void)hipFree(d->d_push_out); d->d_push_out = nullptr; d->push_out_cap = 0;
        if (hipMalloc((void **)&d->d_push_out, out_words * 4) != hipSuccess) { set_error("%s: hipMalloc of %zu bytes failed", what, out_words * 4); return NVX_ERR_NOMEM; }
        d->push_out_cap = out_words;
    }
    HIP_TRY(hipMemcpy(d->d_push_in, in, in_bytes, hipMemcpyHostToDevice));
    const int parity = d->parity[input];
    if ((rc = launch(d, input, 1, consumed, parity, d->d_push_in, n_in, n_in, d->d_push_out, row_words, 0, outs, nullptr)) != NVX_OK) return rc;
    d->consumed[input] = consumed + n_in; d->parity[input] = (uint8_t)(parity ^ 1);
    if (outs) HIP_TRY(hipMemcpy2D(out_iq, cap_samples * 4, d->d_push_out, row_words * 4, outs * 4, (size_t)d->n_slices, hipMemcpyDeviceToHost));     // waits for the null stream
    else HIP_TRY(hipStreamSynchronize(nullptr));
    if (n_out) *n_out = outs;
    return NVX_OK;
}
