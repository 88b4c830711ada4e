// nvx_zoom_host.cpp -- the zoom bank's entry points (include/navtex_amd_zoom.h): the grid rule, the config checks, the plan
// with its carried positions, state rows, shifts and held samples, the checks of a call, and a push's staging.  The launch
// arithmetic is nvx_zoom_plan.h's.  The library stands alone: it shares no state with any other.
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "nvx_companion.h"
#include "nvx_ddc_table.h"
#include "nvx_zoom_plan.h"

extern "C" const char *nvx_zoom_last_error(void) { return nvx_error_text(); }

static const uint32_t MAGIC = 0x4e5a4d31u;      // "NZM1"
static const int BPS[4] = { 4, 2, 2, 8 };       // bytes per input sample, by format
static const char *const NOUN = "the zoom bank";
static const int MAX_HELD = (1 << NVX_ZOOM_MAX_LOG2) - 1;

struct nvx_zoom {
    uint32_t magic = MAGIC;
    std::mutex mu;
    int device = 0, n_inputs = 0, n_zooms = 0, k = 0, format = 0;
    nvx_state_rows<uint32_t> state;                         // [n_inputs][NVX_ZOOM_STATE_WORDS(k)]
    std::vector<int> kz;                                    // [n_inputs][n_zooms]: the host's copy, the master
    int *d_kz = nullptr;
    bool kz_dirty = false;
    uint32_t *d_table = nullptr;                            // [NVX_ZOOM_GRID]
    std::vector<uint64_t> consumed;                         // samples the kernel has taken: multiples of D
    std::vector<uint8_t> held;                              // samples a push left, fewer than D ...
    std::vector<uint64_t> samples;                          // ... [n_inputs][MAX_HELD] of 8 bytes: their bytes
    nvx_event_timer timer;
    nvx_push_staging push;
    struct { int chunks, tiles_per_chunk, warm_tiles, form; size_t lds_bytes; } last = {};
    int64_t kernel_launches = 0;

    char *held_bytes(int input) { return (char *)&samples[(size_t)input * MAX_HELD]; }
};

static bool valid(const nvx_zoom *z, const char *what)
{
    if (!z || z->magic != MAGIC) { set_error("%s: not a zoom bank", what); return false; }
    return true;
}

// ------------------------------------------------------------------------------------------------------ without a device
// kz = rint(hz N / rate), ties to even, decided on the exact remainder hz N - kz rate where the quotient lands on a half
extern "C" int nvx_zoom_grid(double rate_hz, double hz, int *kz, double *applied_hz)
{
    const char *what = "nvx_zoom_grid";
    if (!std::isfinite(rate_hz) || !(rate_hz > 0.0)) { set_error("%s: a rate of %g S/s", what, rate_hz); return NVX_ERR_ARG; }
    if (!std::isfinite(hz) || std::fabs(hz) > rate_hz) { set_error("%s: a shift of %g Hz at %g S/s", what, hz, rate_hz); return NVX_ERR_ARG; }
    const double num = hz * NVX_ZOOM_GRID, half = rate_hz / 2.0;
    long k = std::lrint(num / rate_hz);
    const double rem = std::fma(-(double)k, rate_hz, num);
    if (rem > half || (rem == half && (k & 1))) k++;
    else if (rem < -half || (rem == -half && (k & 1))) k--;
    if (k < NVX_ZOOM_KZ_MIN || k > NVX_ZOOM_KZ_MAX) {
        set_error("%s: %g Hz at %g S/s is table step %ld (%d .. %d)", what, hz, rate_hz, k, NVX_ZOOM_KZ_MIN, NVX_ZOOM_KZ_MAX);
        return NVX_ERR_ARG;
    }
    if (kz) *kz = (int)k;
    if (applied_hz) *applied_hz = (double)k * rate_hz / NVX_ZOOM_GRID;
    return NVX_OK;
}

extern "C" int nvx_zoom_taps(int16_t *taps, int cap, int *reach, int *shift)
{
    if (taps && cap < NVX_REAL_NTAPS) { set_error("nvx_zoom_taps: room for %d taps, there are %d", cap, NVX_REAL_NTAPS); return NVX_ERR_ARG; }
    if (taps) memcpy(taps, NVX_REAL_TAPS, sizeof NVX_REAL_TAPS);
    if (reach) *reach = NVX_ZOOM_STAGE_REACH;
    if (shift) *shift = 15;
    return NVX_REAL_NTAPS;
}

extern "C" void nvx_zoom_config_default(nvx_zoom_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0; cfg->n_inputs = 1; cfg->n_zooms = 1; cfg->log2_decim = 1; cfg->format = NVX_ZOOM_CS16;
}

// --------------------------------------------------------------------------------------------------------------- plans
static void release(nvx_zoom *z)
{
    z->state.release(); (void)hipFree(z->d_kz); (void)hipFree(z->d_table); z->push.release();
    z->timer.destroy();
    z->magic = 0;
    delete z;
}

extern "C" int nvx_zoom_create(const nvx_zoom_config *cfg, nvx_zoom **out)
{
    const char *what = "nvx_zoom_create";
    if (!cfg || !out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    *out = nullptr;
    if (cfg->struct_size != sizeof *cfg) { set_error("%s: struct_size %u, this library's nvx_zoom_config has %zu bytes", what, cfg->struct_size, sizeof *cfg); return NVX_ERR_ARG; }
    if (cfg->n_zooms < 1 || cfg->n_zooms > NVX_ZOOM_MAX_ZOOMS) { set_error("%s: n_zooms %d (1 .. %d)", what, cfg->n_zooms, NVX_ZOOM_MAX_ZOOMS); return NVX_ERR_ARG; }
    if (cfg->n_inputs < 1 || (int64_t)cfg->n_inputs * cfg->n_zooms > 65535) {
        set_error("%s: %d inputs of %d zooms (at least 1 input, 65535 rows at most)", what, cfg->n_inputs, cfg->n_zooms); return NVX_ERR_ARG;
    }
    if (cfg->log2_decim < NVX_ZOOM_MIN_LOG2 || cfg->log2_decim > NVX_ZOOM_MAX_LOG2) {
        set_error("%s: log2_decim %d (%d .. %d)", what, cfg->log2_decim, NVX_ZOOM_MIN_LOG2, NVX_ZOOM_MAX_LOG2); return NVX_ERR_ARG;
    }
    if (cfg->format < NVX_ZOOM_CS16 || cfg->format > NVX_ZOOM_CF32) { set_error("%s: format %d (NVX_ZOOM_CS16 .. NVX_ZOOM_CF32)", what, cfg->format); return NVX_ERR_ARG; }
    if (cfg->device < 0) { set_error("%s: device %d", what, cfg->device); return NVX_ERR_ARG; }
    nvx_zoom *z = new (std::nothrow) nvx_zoom;
    if (!z) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    int rc = select_device(cfg->device, NOUN);
    if (rc != NVX_OK) { release(z); return rc; }
    z->device = cfg->device; z->n_inputs = cfg->n_inputs; z->n_zooms = cfg->n_zooms; z->k = cfg->log2_decim; z->format = cfg->format;
    const size_t rows = (size_t)cfg->n_inputs * cfg->n_zooms;
    z->kz.assign(rows, 0);
    z->consumed.assign(cfg->n_inputs, 0); z->held.assign(cfg->n_inputs, 0); z->samples.assign((size_t)cfg->n_inputs * MAX_HELD, 0);
    // the bank's table, packed: c in the low half, s in the high half
    std::vector<uint32_t> table(NVX_ZOOM_GRID);
    static_assert(NVX_ZOOM_GRID == NVX_DDC_TAB_N, "the zoom's mixer reads the bank's table");
    for (int j = 0; j < NVX_ZOOM_GRID; j++) {
        int16_t c, s;
        nvx_ddc_w(j, &c, &s);
        table[j] = (uint32_t)(uint16_t)c | ((uint32_t)(uint16_t)s << 16);
    }
    hipError_t e = z->state.allocate(cfg->n_inputs, NVX_ZOOM_STATE_WORDS(z->k));
    if (e == hipSuccess) e = hipMalloc((void **)&z->d_kz, rows * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&z->d_table, table.size() * sizeof(uint32_t));
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); release(z); return NVX_ERR_NOMEM; }
    e = hipMemset(z->state.d[0], 0, z->state.bytes(cfg->n_inputs));
    if (e == hipSuccess) e = hipMemset(z->state.d[1], 0, z->state.bytes(cfg->n_inputs));
    if (e == hipSuccess) e = hipMemset(z->d_kz, 0, rows * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(z->d_table, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: clearing the state failed: %s", what, hipGetErrorString(e)); release(z); return NVX_ERR_HIP; }
    nvx_zoom_prepare();
    *out = z;
    return NVX_OK;
}

extern "C" void nvx_zoom_destroy(nvx_zoom *z)
{
    if (!z || z->magic != MAGIC) return;
    (void)hipSetDevice(z->device);
    (void)hipDeviceSynchronize();
    release(z);
}

extern "C" int nvx_zoom_plan(nvx_zoom *z, int *format, int *n_inputs, int *n_zooms, int *log2_decim, int *history)
{
    if (!valid(z, "nvx_zoom_plan")) return NVX_ERR_ARG;
    if (format) *format = z->format;
    if (n_inputs) *n_inputs = z->n_inputs;
    if (n_zooms) *n_zooms = z->n_zooms;
    if (log2_decim) *log2_decim = z->k;
    if (history) *history = NVX_ZOOM_HISTORY(z->k);
    return NVX_OK;
}

extern "C" int nvx_zoom_set_shift(nvx_zoom *z, int input, int zoom, int kz)
{
    const char *what = "nvx_zoom_set_shift";
    if (!valid(z, what) || !row_ok(what, "input", input, -1, z->n_inputs) || !row_ok(what, "zoom", zoom, 0, z->n_zooms)) return NVX_ERR_ARG;
    if (kz < NVX_ZOOM_KZ_MIN || kz > NVX_ZOOM_KZ_MAX) { set_error("%s: table step %d (%d .. %d)", what, kz, NVX_ZOOM_KZ_MIN, NVX_ZOOM_KZ_MAX); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(z->mu);
    for (int i = input < 0 ? 0 : input; i < (input < 0 ? z->n_inputs : input + 1); i++) z->kz[(size_t)i * z->n_zooms + zoom] = kz;
    z->kz_dirty = true;
    return NVX_OK;
}

extern "C" int nvx_zoom_get_shift(nvx_zoom *z, int input, int zoom, int *kz)
{
    const char *what = "nvx_zoom_get_shift";
    if (!valid(z, what) || !row_ok(what, "input", input, 0, z->n_inputs) || !row_ok(what, "zoom", zoom, 0, z->n_zooms)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(z->mu);
    if (kz) *kz = z->kz[(size_t)input * z->n_zooms + zoom];
    return NVX_OK;
}

// `input` (-1: all) stands at sample `position` with silence in front of it and no sample held
static int restart(nvx_zoom *z, const char *what, int input, uint64_t position)
{
    if (!row_ok(what, "input", input, -1, z->n_inputs)) return NVX_ERR_ARG;
    if ((position >> 62) || (position & (((uint64_t)1 << z->k) - 1))) {
        set_error("%s: position %llu (a multiple of %d, below 2^62)", what, (unsigned long long)position, 1 << z->k); return NVX_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(z->mu);
    int rc;
    if ((rc = select_device(z->device, NOUN)) != NVX_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const int first = input < 0 ? 0 : input, n = input < 0 ? z->n_inputs : 1;
    for (int i = first, j; i < first + n; i = j) {          // runs of inputs whose rows lie side by side
        j = z->state.run_end(i, first + n);
        HIP_TRY(hipMemset(z->state.row(i), 0, z->state.bytes(j - i)));
    }
    HIP_TRY(hipDeviceSynchronize());
    for (int i = first; i < first + n; i++) { z->consumed[i] = position; z->held[i] = 0; }
    return NVX_OK;
}

extern "C" int nvx_zoom_reset(nvx_zoom *z, int input)
{
    return valid(z, "nvx_zoom_reset") ? restart(z, "nvx_zoom_reset", input, 0) : NVX_ERR_ARG;
}

extern "C" int nvx_zoom_debug_set_position(nvx_zoom *z, int input, uint64_t position)
{
    return valid(z, "nvx_zoom_debug_set_position") ? restart(z, "nvx_zoom_debug_set_position", input, position) : NVX_ERR_ARG;
}

extern "C" int nvx_zoom_position(nvx_zoom *z, int input, uint64_t *consumed, uint64_t *produced)
{
    const char *what = "nvx_zoom_position";
    if (!valid(z, what) || !row_ok(what, "input", input, 0, z->n_inputs)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(z->mu);
    if (consumed) *consumed = z->consumed[input] + z->held[input];
    if (produced) *produced = z->consumed[input] >> z->k;
    return NVX_OK;
}

extern "C" int nvx_zoom_timing(nvx_zoom *z, int enable)
{
    return valid(z, "nvx_zoom_timing") ? timing_enable(z->mu, z->timer, enable) : NVX_ERR_ARG;
}

extern "C" int nvx_zoom_time_stats(nvx_zoom *z, double *sum_ms, uint64_t *calls, int reset)
{
    return valid(z, "nvx_zoom_time_stats") ? timing_collect(z->mu, z->timer, sum_ms, calls, reset) : NVX_ERR_ARG;
}

extern "C" int64_t nvx_zoom_debug_last_launch(nvx_zoom *z, int *chunks, int *tiles_per_chunk, int *warm_tiles, int *form, size_t *lds_bytes)
{
    if (!valid(z, "nvx_zoom_debug_last_launch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(z->mu);
    if (z->kernel_launches) {
        if (chunks) *chunks = z->last.chunks;
        if (tiles_per_chunk) *tiles_per_chunk = z->last.tiles_per_chunk;
        if (warm_tiles) *warm_tiles = z->last.warm_tiles;
        if (form) *form = z->last.form;
        if (lds_bytes) *lds_bytes = z->last.lds_bytes;
    }
    return z->kernel_launches;
}

// ------------------------------------------------------------------------------------------------------------ launches
// One call over inputs [first, first + n) of the plan, every zoom of each, which stand at `consumed` and read state row
// `parity`; the caller holds the plan's lock and has checked every span.  n_in is a multiple of D and not zero.
static int launch(nvx_zoom *z, int first, int n, uint64_t consumed, int parity, const void *d_in, size_t pitch_in, size_t n_in, uint32_t *d_out,
                  size_t pitch_out, size_t out_first, hipStream_t s)
{
    nvx_zoom_args a;
    const int chunks = nvx_zoom_fill_args(consumed, d_in, pitch_in, n_in, d_out, pitch_out, out_first, n, z->n_zooms, z->k, z->state.in(first, parity),
                                          z->state.out(first, parity), z->d_kz + (size_t)first * z->n_zooms, z->d_table,
                                          nvx_stream_wanted(n, NVX_ZOOM_TARGET_WORKGROUPS), &a);
    // the shifts, where they changed since the last call: pageable memory, staged by the runtime before it returns
    if (z->kz_dirty) {
        HIP_TRY(hipMemcpyAsync(z->d_kz, z->kz.data(), z->kz.size() * sizeof(int), hipMemcpyHostToDevice, s));
        z->kz_dirty = false;
    }
    nvx_event_timer::events ev;
    int rc;
    if ((rc = z->timer.begin(s, ev)) != NVX_OK) return rc;
    HIP_TRY(nvx_zoom_launch(&a, z->format, n, chunks, s));
    z->last = { chunks, a.tiles_per_chunk, a.warm_tiles, chunks > 1 ? 2 : 1, NVX_ZOOM_LDS_STATIC + NVX_ZOOM_LDS_DYNAMIC(z->k, z->n_zooms) };
    z->kernel_launches += 1;
    if ((rc = z->timer.end(s, ev)) != NVX_OK) return rc;
    for (int i = first; i < first + n; i++) z->consumed[i] = consumed + n_in;
    z->state.flip(first, n, parity);
    return NVX_OK;
}

extern "C" int nvx_zoom_resident(nvx_zoom *z, const void *d_in, size_t pitch_in, size_t n_in, void *d_out, size_t pitch_out, size_t out_first,
                                 size_t *n_out, void *hip_stream)
{
    const char *what = "nvx_zoom_resident";
    if (!valid(z, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(z->mu);
    const size_t D = (size_t)1 << z->k;
    if (!d_in || !d_out || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 3) || n_in > NVX_ZOOM_MAX_IN || (n_in & (D - 1))) {
        set_error("%s: bad argument (null pointer, input not 16-byte aligned, output not 4-byte aligned, a number of samples that is no multiple of %zu, or "
                  "more than 2^30)", what, D);
        return NVX_ERR_ARG;
    }
    for (int i = 0; i < z->n_inputs; i++) {
        if (z->held[i]) {
            set_error("%s: input %d holds %d samples of a push: push until none is left, or reset it", what, i, (int)z->held[i]);
            return NVX_ERR_STATE;
        }
        if (!stands_with_first(what, "input", z->consumed, i)) return NVX_ERR_STATE;
    }
    const uint64_t consumed = z->consumed[0];
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    const size_t outs = n_in >> z->k, rows_in = (size_t)z->n_inputs, rows_out = rows_in * z->n_zooms, bps = (size_t)BPS[z->format];
    size_t in_bytes, out_bytes, out_end;
    if (__builtin_add_overflow(out_first, outs, &out_end) || !span_bytes(rows_in - 1, pitch_in, n_in, bps, &in_bytes) ||
        !span_bytes(rows_out - 1, pitch_out, out_end, 4, &out_bytes) || (uintptr_t)d_in + in_bytes < in_bytes || (uintptr_t)d_out + out_bytes < out_bytes) {
        set_error("%s: the span of %zu samples of %d inputs at pitch %zu, or of %zu words from %zu of %zu rows at pitch %zu, overflows", what, n_in,
                  z->n_inputs, pitch_in, outs, out_first, rows_out, pitch_out);
        return NVX_ERR_ARG;
    }
    if ((rows_in > 1 && (n_in > pitch_in || ((pitch_in * bps) & 15))) || (rows_out > 1 && out_end > pitch_out)) {
        set_error("%s: %zu samples per input at pitch %zu, words up to %zu at pitch %zu (a row must hold them, and input rows are 16-byte aligned)", what,
                  n_in, pitch_in, out_end, pitch_out);
        return NVX_ERR_ARG;
    }
    if (n_out) *n_out = outs;
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(z->device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_in, in_bytes, what, "input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out, out_bytes, what, "output")) != NVX_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    if ((rc = z->state.align(nullptr, s)) != NVX_OK) return rc;
    return launch(z, 0, z->n_inputs, consumed, z->state.parity[0], d_in, pitch_in, n_in, (uint32_t *)d_out, pitch_out, out_first, s);
}

extern "C" int nvx_zoom_push(nvx_zoom *z, int input, const void *in, size_t n_in, int16_t *out_iq, size_t cap_samples, size_t *n_out)
{
    const char *what = "nvx_zoom_push";
    if (!valid(z, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(z->mu);
    if (input < 0 || input >= z->n_inputs || !in || !out_iq || n_in > NVX_ZOOM_MAX_IN) {
        set_error("%s: bad argument (input %d of %d, null pointer, or more than 2^30 samples)", what, input, z->n_inputs);
        return NVX_ERR_ARG;
    }
    const size_t D = (size_t)1 << z->k, bps = (size_t)BPS[z->format], front = z->held[input], have = n_in + front, use = have & ~(D - 1), words = use >> z->k;
    size_t all_words;
    if (words > cap_samples || __builtin_mul_overflow(cap_samples, (size_t)z->n_zooms * 4, &all_words)) {
        set_error("%s: %zu outputs per zoom, a zoom's row holds %zu: nothing consumed", what, words, cap_samples); return NVX_ERR_ARG;
    }
    const uint64_t consumed = z->consumed[input];
    if (!position_ok(what, consumed + have)) return NVX_ERR_ARG;
    char *const held = z->held_bytes(input);
    if (use) {
        int rc;
        if ((rc = select_device(z->device, NOUN)) != NVX_OK) return rc;
        if ((rc = z->push.reserve(what, use * bps, words * z->n_zooms)) != NVX_OK) return rc;
        // the held samples go in front
        if (front) HIP_TRY(hipMemcpy(z->push.d_in, held, front * bps, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy((char *)z->push.d_in + front * bps, in, (use - front) * bps, hipMemcpyHostToDevice));
        if ((rc = launch(z, input, 1, consumed, z->state.parity[input], z->push.d_in, use, use, z->push.d_out, words, 0, nullptr)) != NVX_OK) return rc;
        HIP_TRY(hipMemcpy2D(out_iq, cap_samples * 4, z->push.d_out, words * 4, words * 4, (size_t)z->n_zooms, hipMemcpyDeviceToHost));    // waits for the null stream
        // the samples behind the last whole group wait for the rest of theirs
        memcpy(held, (const char *)in + (use - front) * bps, (have - use) * bps);
    } else memcpy(held + front * bps, in, n_in * bps);
    z->held[input] = (uint8_t)(have - use);
    if (n_out) *n_out = words;
    return NVX_OK;
}
