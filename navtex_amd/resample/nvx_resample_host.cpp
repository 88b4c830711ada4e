// nvx_resample_host.cpp -- the resampler's entry points (include/navtex_amd_resample.h): the plan, argument and span
// checks, the carried positions, the choice of kernel form, HIP-event timing.  The library stands alone: it shares no
// state with libnavtex_amd.so.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "nvx_resample_plan.h"

static thread_local char g_err[512] = "";

static void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

extern "C" const char *nvx_resample_last_error(void) { return g_err; }

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? NVX_ERR_NODEV : NVX_ERR_HIP; \
        }                                                                                  \
    } while (0)

static const uint32_t MAGIC = 0x4e525331u;      // "NRS1"
static const int BPS[4] = { 4, 2, 2, 8 };
static const int TARGET_WORKGROUPS = 2048;      // form 2 spreads a stream's tiles until the grid has about this many

struct nvx_resampler {
    uint32_t magic = MAGIC;
    std::mutex mu;
    int device = 0, n_streams = 0, format = 0;
    uint32_t rate = 0;
    int L = 0, M = 0, T = 0, Tp = 0, row_dw = 0, tap_dw = 0, K = 0, hist_pitch = 0;
    bool taps_in_lds = false;
    uint32_t dq = 0, dr = 0;
    uint32_t *d_taps = nullptr, *d_hist[2] = { nullptr, nullptr };
    std::vector<uint64_t> consumed;
    std::vector<uint8_t> parity;                 // which history row the stream's next launch reads
    int form = 0;
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool, pending;
    double sum_ms = 0.0; uint64_t launches = 0;
    void *d_push_in = nullptr; uint32_t *d_push_out = nullptr;     // nvx_resample_push's staging, grown on demand
    size_t push_in_cap = 0, push_out_cap = 0;
    struct { int K, tiles, tiles_per_chunk, chunks, taps_in_lds; size_t lds_bytes; } last = {};      // nvx_resample_debug_last_launch
    int64_t kernel_launches = 0;
};

static bool valid(const nvx_resampler *r, const char *what)
{
    if (!r || r->magic != MAGIC) { set_error("%s: not a resampler", what); return false; }
    return true;
}

static int select_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        set_error("no HIP device available (%s); the resampler has no CPU path", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
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
    (void)hipFree(r->d_taps); (void)hipFree(r->d_hist[0]); (void)hipFree(r->d_hist[1]);
    (void)hipFree(r->d_push_in); (void)hipFree(r->d_push_out);
    for (auto &p : r->pending) r->pool.push_back(p);
    for (auto &p : r->pool) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
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
    int L, M, T;
    const char *why = "";
    if (nvx_rs_plan_numbers(cfg->input_rate_hz, &L, &M, &T, &why) != NVX_OK) { set_error("%s: %u S/s: %s", what, cfg->input_rate_hz, why); return NVX_ERR_ARG; }
    std::vector<int16_t> taps((size_t)L * T);
    int rc = nvx_rs_plan_taps(cfg->input_rate_hz, L, T, taps.data(), &why);
    if (rc != NVX_OK) { set_error("%s: %u S/s: %s", what, cfg->input_rate_hz, why); return rc; }
    if ((rc = select_device(cfg->device)) != NVX_OK) return rc;
    HIP_TRY(nvx_rs_prepare());

    nvx_resampler *r = new (std::nothrow) nvx_resampler;
    if (!r) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    r->device = cfg->device; r->n_streams = cfg->n_streams; r->format = cfg->format; r->rate = cfg->input_rate_hz;
    r->L = L; r->M = M; r->T = T;
    r->Tp = (T + NVX_RS_ALIGN - 1 + 3) & ~3;
    r->row_dw = r->Tp / 2 + ((r->Tp / 4) % 2 == 0 ? 2 : 0);      // an odd number of 8-byte words: 32 consecutive phases, 32 bank pairs
    r->tap_dw = (NVX_RS_ALIGN * L * r->row_dw + 3) & ~3;
    r->taps_in_lds = (size_t)r->tap_dw * 4 <= NVX_RS_TAPS_LDS_MAX;
    r->dq = (uint32_t)(NVX_RS_THREADS * (uint64_t)M / L); r->dr = (uint32_t)(NVX_RS_THREADS * (uint64_t)M % L);
    // the largest tile whose input span fits the planes: (256 K - 1) M / L + 1 samples between its first and last window
    // end, T - 1 in front, up to 7 + 15 of rounding to groups
    for (r->K = NVX_RS_MAX_K; r->K > 1; r->K--)
        if (((uint64_t)(NVX_RS_THREADS * r->K - 1) * M) / L + 2 + T + 24 <= NVX_RS_PLANE) break;
    if (((uint64_t)(NVX_RS_THREADS * r->K - 1) * M) / L + 2 + T + 24 > NVX_RS_PLANE) {
        set_error("%s: %u S/s: one tile's input does not fit the kernel's staging area", what, cfg->input_rate_hz);
        release(r); return NVX_ERR_ARG;
    }
    r->hist_pitch = (T - 1 + 3) & ~3;
    r->consumed.assign(r->n_streams, 0);
    r->parity.assign(r->n_streams, 0);

    // the table the kernel reads: copy `shift` of phase r holds h[r][T-1-i] at position shift + i
    std::vector<uint16_t> table((size_t)r->tap_dw * 2, 0);
    for (int sh = 0; sh < NVX_RS_ALIGN; sh++)
        for (int ph = 0; ph < L; ph++)
            for (int i = 0; i < T; i++)
                table[((size_t)(sh * L + ph) * r->row_dw) * 2 + sh + i] = (uint16_t)taps[(size_t)ph * T + (T - 1 - i)];
    const size_t hist_bytes = (size_t)r->n_streams * r->hist_pitch * 4;
    hipError_t e = hipMalloc((void **)&r->d_taps, (size_t)r->tap_dw * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&r->d_hist[0], hist_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&r->d_hist[1], hist_bytes);
    if (e != hipSuccess) { set_error("%s: hipMalloc failed: %s", what, hipGetErrorString(e)); release(r); return NVX_ERR_NOMEM; }
    e = hipMemcpy(r->d_taps, table.data(), (size_t)r->tap_dw * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(r->d_hist[0], 0, hist_bytes);
    if (e == hipSuccess) e = hipMemset(r->d_hist[1], 0, hist_bytes);
    if (e != hipSuccess) { set_error("%s: filling the tables failed: %s", what, hipGetErrorString(e)); release(r); return NVX_ERR_HIP; }
    *out = r;
    return NVX_OK;
}

extern "C" void nvx_resample_destroy(nvx_resampler *r)
{
    if (!r || r->magic != MAGIC) return;
    (void)hipSetDevice(r->device);
    (void)hipDeviceSynchronize();
    release(r);
}

extern "C" int nvx_resample_plan(nvx_resampler *r, int *L, int *M, int *T, int *n_streams, int *format)
{
    if (!valid(r, "nvx_resample_plan")) return NVX_ERR_ARG;
    if (L) *L = r->L;
    if (M) *M = r->M;
    if (T) *T = r->T;
    if (n_streams) *n_streams = r->n_streams;
    if (format) *format = r->format;
    return NVX_OK;
}

extern "C" int nvx_resample_reset(nvx_resampler *r, int stream)
{
    if (!valid(r, "nvx_resample_reset")) return NVX_ERR_ARG;
    if (stream < -1 || stream >= r->n_streams) { set_error("nvx_resample_reset: stream %d of %d", stream, r->n_streams); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(r->mu);
    // a stream at position 0 has silence in front: its history rows are not read before they are written again
    for (int s = stream < 0 ? 0 : stream; s < (stream < 0 ? r->n_streams : stream + 1); s++) r->consumed[s] = 0;
    return NVX_OK;
}

extern "C" int nvx_resample_position(nvx_resampler *r, int stream, uint64_t *consumed, uint64_t *produced)
{
    if (!valid(r, "nvx_resample_position")) return NVX_ERR_ARG;
    if (stream < 0 || stream >= r->n_streams) { set_error("nvx_resample_position: stream %d of %d", stream, r->n_streams); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(r->mu);
    if (consumed) *consumed = r->consumed[stream];
    if (produced) *produced = nvx_rs_outputs_after(r->consumed[stream], r->L, r->M);
    return NVX_OK;
}

extern "C" int nvx_resample_set_form(nvx_resampler *r, int form)
{
    if (!valid(r, "nvx_resample_set_form")) return NVX_ERR_ARG;
    if (form < 0 || form > 2) { set_error("nvx_resample_set_form: form %d (0, 1 or 2)", form); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(r->mu);
    r->form = form;
    return NVX_OK;
}

extern "C" int nvx_resample_timing(nvx_resampler *r, int enable)
{
    if (!valid(r, "nvx_resample_timing")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(r->mu);
    r->timing = enable != 0;
    return NVX_OK;
}

extern "C" int nvx_resample_time_stats(nvx_resampler *r, double *sum_ms, uint64_t *launches, int reset)
{
    if (!valid(r, "nvx_resample_time_stats")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(r->mu);
    for (auto &p : r->pending) {
        HIP_TRY(hipEventSynchronize(p.second));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
        r->sum_ms += ms; r->launches++;
        r->pool.push_back(p);
    }
    r->pending.clear();
    if (sum_ms) *sum_ms = r->sum_ms;
    if (launches) *launches = r->launches;
    if (reset) { r->sum_ms = 0.0; r->launches = 0; }
    return NVX_OK;
}

extern "C" int64_t nvx_resample_debug_last_launch(nvx_resampler *r, int *K, int *tiles, int *tiles_per_chunk, int *chunks,
                                                  int *taps_in_lds, size_t *lds_bytes)
{
    if (!valid(r, "nvx_resample_debug_last_launch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(r->mu);
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
// One launch over streams [first_stream, first_stream + n_streams) of the plan, which stand at `consumed` and read history
// row `parity`; the caller holds r->mu and has checked every span.
static int launch(nvx_resampler *r, int first_stream, int n_streams, uint64_t consumed, int parity, const void *d_in, size_t pitch_in,
                  size_t n_in, uint32_t *d_out, size_t pitch_out, size_t out_first, size_t n_out, hipStream_t s)
{
    nvx_rs_args a{};
    a.in = d_in; a.pitch_in = pitch_in; a.out = d_out; a.pitch_out = pitch_out; a.out_first = out_first;
    a.hist_in = r->d_hist[parity] + (size_t)first_stream * r->hist_pitch;
    a.hist_out = r->d_hist[parity ^ 1] + (size_t)first_stream * r->hist_pitch;
    a.taps = r->d_taps;
    a.hist_pitch = r->hist_pitch; a.hist_valid = consumed > 0;
    a.n_in = (int)n_in; a.n_out = (int)n_out;
    a.L = r->L; a.M = r->M; a.T = r->T; a.Tp = r->Tp; a.row_dw = r->row_dw; a.tap_dw = r->tap_dw; a.K = r->K;
    a.dq = r->dq; a.dr = r->dr;
    // output 0 of the call is the stream's output n0 = ceil(consumed L / M): n0 M = Q0 L + r0, and Q0 >= consumed
    const uint64_t n0 = nvx_rs_outputs_after(consumed, r->L, r->M);
    const unsigned __int128 pos = (unsigned __int128)n0 * (unsigned)r->M;
    a.r0 = (uint32_t)(pos % (unsigned)r->L);
    a.qoff = (int)((uint64_t)(pos / (unsigned)r->L) - consumed);
    const int tile_out = NVX_RS_THREADS * r->K;
    a.tiles = (int)((n_out + tile_out - 1) / tile_out);
    // a workgroup per stream fills the chip from a few workgroups per CU on; below that a stream's tiles are spread out
    int form = r->form ? r->form : (n_streams >= 1024 ? 1 : 2);
    int chunks = 1;
    if (form == 2 && a.tiles > 1) {
        chunks = (TARGET_WORKGROUPS + n_streams - 1) / n_streams;
        if (chunks > a.tiles) chunks = a.tiles;
    }
    a.tiles_per_chunk = a.tiles ? (a.tiles + chunks - 1) / chunks : 1;
    chunks = a.tiles ? (a.tiles + a.tiles_per_chunk - 1) / a.tiles_per_chunk : 1;
    // the steps the kernel advances its positions by, as (div L, mod L)
    const uint64_t uL = (uint64_t)r->L, tile_pos = (uint64_t)tile_out * r->M, chunk_pos = tile_pos * (uint64_t)a.tiles_per_chunk;
    a.tile_dq = (uint32_t)(tile_pos / uL); a.tile_dr = (uint32_t)(tile_pos % uL);
    a.chunk_dq = (uint32_t)(chunk_pos / uL); a.chunk_dr = (uint32_t)(chunk_pos % uL);
    a.span_q = (uint32_t)((tile_pos - r->M) / uL); a.span_r = (uint32_t)((tile_pos - r->M) % uL);
    a.m_div = (uint32_t)(r->M / r->L); a.m_mod = (uint32_t)(r->M % r->L);

    std::pair<hipEvent_t, hipEvent_t> ev{ nullptr, nullptr };
    const bool timed = r->timing;
    if (timed) {
        if (r->pool.empty()) { HIP_TRY(hipEventCreate(&ev.first)); HIP_TRY(hipEventCreate(&ev.second)); }
        else { ev = r->pool.back(); r->pool.pop_back(); }
        HIP_TRY(hipEventRecord(ev.first, s));
    }
    HIP_TRY(nvx_rs_launch(&a, r->format, n_streams, chunks, r->taps_in_lds, s));
    r->last = { a.K, a.tiles, a.tiles_per_chunk, chunks, r->taps_in_lds ? 1 : 0, nvx_rs_lds_bytes(&a, r->taps_in_lds) };
    r->kernel_launches++;
    if (timed) { HIP_TRY(hipEventRecord(ev.second, s)); r->pending.push_back(ev); }
    return NVX_OK;
}

extern "C" int nvx_resample_resident(nvx_resampler *r, const void *d_in, size_t pitch_in, size_t n_in, void *d_out,
                                     size_t pitch_out, size_t out_first, size_t *n_out, void *hip_stream)
{
    const char *what = "nvx_resample_resident";
    if (!valid(r, what)) return NVX_ERR_ARG;
    const size_t bps = (size_t)BPS[r->format];
    if (!d_in || !d_out || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 3) || n_in > NVX_RS_MAX_IN) {
        set_error("%s: bad argument (null pointer, input not 16-byte aligned, output not 4-byte aligned, or more than 2^30 samples)", what);
        return NVX_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(r->mu);
    const uint64_t consumed = r->consumed[0];
    for (int s = 1; s < r->n_streams; s++)
        if (r->consumed[s] != consumed) {
            set_error("%s: stream %d stands at %llu, stream 0 at %llu: all streams of a call stand at the same position", what, s,
                      (unsigned long long)r->consumed[s], (unsigned long long)consumed);
            return NVX_ERR_STATE;
        }
    if ((consumed + n_in) >> 62) { set_error("%s: the position passes 2^62", what); return NVX_ERR_ARG; }
    const size_t outs = (size_t)(nvx_rs_outputs_after(consumed + n_in, r->L, r->M) - nvx_rs_outputs_after(consumed, r->L, r->M));
    // every stream's last sample read and last word written, in samples of its row and in bytes of the whole operand
    size_t out_end, in_bytes, out_bytes;
    if (__builtin_add_overflow(out_first, outs, &out_end) || outs > 0x7fffffffu ||
        !span_bytes((size_t)(r->n_streams - 1), pitch_in, n_in, bps, &in_bytes) ||
        !span_bytes((size_t)(r->n_streams - 1), pitch_out, out_end, 4, &out_bytes)) {
        set_error("%s: the span of %zu samples of %d streams at pitch %zu, or of %zu outputs from %zu at pitch %zu, overflows", what, n_in,
                  r->n_streams, pitch_in, outs, out_first, pitch_out);
        return NVX_ERR_ARG;
    }
    if (r->n_streams > 1 && (n_in > pitch_in || out_end > pitch_out || ((pitch_in * bps) & 15))) {
        set_error("%s: %zu samples per stream at pitch %zu, outputs up to %zu at pitch %zu (a row must hold them, and input rows are 16-byte aligned)",
                  what, n_in, pitch_in, out_end, pitch_out);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) { if (n_out) *n_out = 0; return NVX_OK; }
    int rc;
    if ((rc = select_device(r->device)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_in, in_bytes, "nvx_resample_resident: input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out, out_bytes, "nvx_resample_resident: output")) != NVX_OK) return rc;

    hipStream_t s = (hipStream_t)hip_stream;
    // streams pushed one by one may read different history rows: bring them to stream 0's
    const int parity = r->parity[0];
    for (int k = 1; k < r->n_streams; k++)
        if (r->parity[k] != parity) {
            HIP_TRY(hipMemcpyAsync(r->d_hist[parity] + (size_t)k * r->hist_pitch, r->d_hist[parity ^ 1] + (size_t)k * r->hist_pitch,
                                   (size_t)r->hist_pitch * 4, hipMemcpyDeviceToDevice, s));
            r->parity[k] = (uint8_t)parity;
        }
    if ((rc = launch(r, 0, r->n_streams, consumed, parity, d_in, pitch_in, n_in, (uint32_t *)d_out, pitch_out, out_first, outs, s)) != NVX_OK) return rc;
    for (int k = 0; k < r->n_streams; k++) { r->consumed[k] = consumed + n_in; r->parity[k] = (uint8_t)(parity ^ 1); }
    if (n_out) *n_out = outs;
    return NVX_OK;
}

extern "C" int nvx_resample_push(nvx_resampler *r, int stream, const void *in, size_t n_in, int16_t *out_iq, size_t cap_samples, size_t *n_out)
{
    const char *what = "nvx_resample_push";
    if (!valid(r, what)) return NVX_ERR_ARG;
    if (stream < 0 || stream >= r->n_streams || !in || (!out_iq && cap_samples) || n_in > NVX_RS_MAX_IN) {
        set_error("%s: bad argument (stream %d of %d, null pointer, or more than 2^30 samples)", what, stream, r->n_streams);
        return NVX_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(r->mu);
    const uint64_t consumed = r->consumed[stream];
    if ((consumed + n_in) >> 62) { set_error("%s: the position passes 2^62", what); return NVX_ERR_ARG; }
    const size_t outs = (size_t)(nvx_rs_outputs_after(consumed + n_in, r->L, r->M) - nvx_rs_outputs_after(consumed, r->L, r->M));
    if (outs > cap_samples || outs > 0x7fffffffu) {
        set_error("%s: %zu samples give %zu outputs, the buffer holds %zu: nothing consumed", what, n_in, outs, cap_samples);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) { if (n_out) *n_out = 0; return NVX_OK; }
    int rc;
    if ((rc = select_device(r->device)) != NVX_OK) return rc;
    const size_t in_bytes = n_in * (size_t)BPS[r->format], out_words = outs ? outs : 1;
    if (in_bytes > r->push_in_cap) {
        (void)hipFree(r->d_push_in); r->d_push_in = nullptr; r->push_in_cap = 0;
        if (hipMalloc(&r->d_push_in, in_bytes) != hipSuccess) { set_error("%s: hipMalloc of %zu bytes failed", what, in_bytes); return NVX_ERR_NOMEM; }
        r->push_in_cap = in_bytes;
    }
    if (out_words > r->push_out_cap) {
        (void)hipFree(r->d_push_out); r->d_push_out = nullptr; r->push_out_cap = 0;
        if (hipMalloc((void **)&r->d_push_out, out_words * 4) != hipSuccess) { set_error("%s: hipMalloc of %zu bytes failed", what, out_words * 4); return NVX_ERR_NOMEM; }
        r->push_out_cap = out_words;
    }
    HIP_TRY(hipMemcpy(r->d_push_in, in, in_bytes, hipMemcpyHostToDevice));
    const int parity = r->parity[stream];
    if ((rc = launch(r, stream, 1, consumed, parity, r->d_push_in, n_in, n_in, r->d_push_out, out_words, 0, outs, nullptr)) != NVX_OK) return rc;
    r->consumed[stream] = consumed + n_in; r->parity[stream] = (uint8_t)(parity ^ 1);
    if (outs) HIP_TRY(hipMemcpy(out_iq, r->d_push_out, outs * 4, hipMemcpyDeviceToHost));     // waits for the null stream
    else HIP_TRY(hipStreamSynchronize(nullptr));
    if (n_out) *n_out = outs;
    return NVX_OK;
}
