// nvx_tap_host.cpp -- the channel tap's entry points (include/navtex_amd_tap.h): the design, grid and table without a device,
// the config checks, the plan with its tap table, shifts, pitches and carried positions, and the checks of a call.  The state
// rows, a push's staging, the row and position checks and the timing bodies are nvx_companion.h's, the launch arithmetic
// nvx_tap_plan.h's.  The library stands alone: it shares no state with any other.
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "nvx_companion.h"
#include "nvx_ddc_table.h"
#include "nvx_tap_plan.h"

static_assert(NVX_TAP_GRID == NVX_DDC_TAB_N, "the bank's table");

extern "C" const char *nvx_tap_last_error(void) { return nvx_error_text(); }

static const uint32_t MAGIC = 0x4e545031u;      // "NTP1"
static const char *const NOUN = "the channel tap";

struct nvx_tap {
    uint32_t magic = MAGIC;
    std::mutex mu;
    int device = 0, n_inputs = 0, n_taps = 0, kind = 0;
    uint32_t fo = 0;
    nvx_tap_args shape = {};                                // L, M, T and what follows from them
    int16_t *d_table = nullptr;
    uint32_t *d_w = nullptr;
    nvx_state_rows<uint32_t> state;                         // [n_inputs][T]
    int *d_kk = nullptr, *h_kk = nullptr;                   // [2][rows]: shifts, then pitches; the pinned row they are uploaded from
    std::vector<int> kk;
    bool kk_dirty = true;
    hipEvent_t kk_uploaded = nullptr;
    std::vector<uint64_t> consumed;
    nvx_event_timer timer;
    nvx_push_staging push;                                  // 4-byte input words; the output in words too, rounded up (audio is int16)
    struct { int tile_out, tiles, form, waves; size_t lds_bytes; } last = {};
    int64_t kernel_launches = 0;

    size_t rows() const { return (size_t)n_inputs * n_taps; }
    size_t out_size() const { return kind == NVX_TAP_IQ ? 4 : 2; }
};

static bool valid(const nvx_tap *c, const char *what)
{
    if (!c || c->magic != MAGIC) { set_error("%s: not a channel tap", what); return false; }
    return true;
}

static bool input_tap_ok(const nvx_tap *c, const char *what, int input, int lowest, int tap)
{
    if (input < lowest || input >= c->n_inputs || tap < 0 || tap >= c->n_taps) {
        set_error("%s: input %d of %d, tap %d of %d", what, input, c->n_inputs, tap, c->n_taps);
        return false;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------------ without a device
extern "C" int nvx_tap_design(uint32_t fo, int kind, int *L, int *M, int *T, int32_t *taps, int cap)
{
    int l, m, t;
    const char *why = "";
    if (nvx_tap_plan_numbers(fo, kind, &l, &m, &t, &why) != NVX_OK) { set_error("nvx_tap_design: %u S/s, kind %d: %s", fo, kind, why); return NVX_ERR_ARG; }
    if (cap < 0) { set_error("nvx_tap_design: cap %d", cap); return NVX_ERR_ARG; }
    if (L) *L = l;
    if (M) *M = m;
    if (T) *T = t;
    if (taps && cap >= l * t) {
        const int rc = nvx_tap_plan_taps(fo, kind, l, t, taps, &why);
        if (rc != NVX_OK) { set_error("nvx_tap_design: %u S/s, kind %d: %s", fo, kind, why); return rc; }
    }
    return l * t;
}

extern "C" int nvx_tap_grid(uint32_t fo, int kind, double hz, int *k, double *applied_hz)
{
    int kk;
    const char *why = "";
    if (nvx_tap_shift_k(fo, kind, hz, &kk, &why) != NVX_OK) { set_error("nvx_tap_grid: %g Hz at %u S/s, kind %d: %s", hz, fo, kind, why); return NVX_ERR_ARG; }
    if (k) *k = kk;
    if (applied_hz) *applied_hz = (double)kk * NVX_TAP_INPUT_RATE / NVX_TAP_GRID;
    return NVX_OK;
}

extern "C" int nvx_tap_table(int16_t *cs, int cap_pairs)
{
    if (cs && cap_pairs >= NVX_TAP_GRID)
        for (int j = 0; j < NVX_TAP_GRID; j++) nvx_ddc_w(j, &cs[2 * j], &cs[2 * j + 1]);
    return NVX_TAP_GRID;
}

extern "C" void nvx_tap_config_default(nvx_tap_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0; cfg->n_inputs = 1; cfg->n_taps = 1; cfg->output_rate_hz = 12000; cfg->kind = NVX_TAP_IQ;
}

// --------------------------------------------------------------------------------------------------------------- plans
static void release(nvx_tap *c)
{
    (void)hipFree(c->d_table); (void)hipFree(c->d_w); (void)hipFree(c->d_kk); (void)hipHostFree(c->h_kk);
    c->state.release(); c->push.release();
    if (c->kk_uploaded) (void)hipEventDestroy(c->kk_uploaded);
    c->timer.destroy();
    c->magic = 0;
    delete c;
}

extern "C" int nvx_tap_create(const nvx_tap_config *cfg, nvx_tap **out)
{
    const char *what = "nvx_tap_create";
    if (!cfg || !out) { set_error("%s: null argument", what); return NVX_ERR_ARG; }
    *out = nullptr;
    if (cfg->struct_size != sizeof *cfg) { set_error("%s: struct_size %u, this library's nvx_tap_config has %zu bytes", what, cfg->struct_size, sizeof *cfg); return NVX_ERR_ARG; }
    if (cfg->n_inputs < 1 || cfg->n_taps < 1 || cfg->n_inputs > 65535 || cfg->n_taps > 65535 || (int64_t)cfg->n_inputs * cfg->n_taps > 65535) {
        set_error("%s: %d inputs of %d taps (each at least 1, 65535 rows at most)", what, cfg->n_inputs, cfg->n_taps); return NVX_ERR_ARG;
    }
    if (cfg->kind != NVX_TAP_IQ && cfg->kind != NVX_TAP_REAL) { set_error("%s: kind %d (NVX_TAP_IQ or NVX_TAP_REAL)", what, cfg->kind); return NVX_ERR_ARG; }
    if (cfg->device < 0) { set_error("%s: device %d", what, cfg->device); return NVX_ERR_ARG; }
    int L, M, T;
    const char *why = "";
    if (nvx_tap_plan_numbers(cfg->output_rate_hz, cfg->kind, &L, &M, &T, &why) != NVX_OK) {
        set_error("%s: %u S/s: %s", what, cfg->output_rate_hz, why);
        return NVX_ERR_ARG;
    }
    std::vector<int32_t> taps((size_t)L * T);
    int rc = nvx_tap_plan_taps(cfg->output_rate_hz, cfg->kind, L, T, taps.data(), &why);
    if (rc != NVX_OK) { set_error("%s: %u S/s: %s", what, cfg->output_rate_hz, why); return rc; }
    int kp = 0;
    if (cfg->kind == NVX_TAP_REAL && nvx_tap_pitch_k(cfg->output_rate_hz, NVX_TAP_DEFAULT_PITCH_HZ, &kp, &why) != NVX_OK) {
        set_error("%s: %u S/s: %s", what, cfg->output_rate_hz, why);
        return NVX_ERR_ARG;
    }
    nvx_tap *c = new (std::nothrow) nvx_tap;
    if (!c) { set_error("%s: out of memory", what); return NVX_ERR_NOMEM; }
    rc = select_device(cfg->device, NOUN);
    if (rc != NVX_OK) { release(c); return rc; }
    c->device = cfg->device; c->n_inputs = cfg->n_inputs; c->n_taps = cfg->n_taps; c->kind = cfg->kind; c->fo = cfg->output_rate_hz;
    nvx_tap_fill_shape(L, M, T, &c->shape);
    c->shape.state_pitch = T; c->shape.n_taps = cfg->n_taps;
    c->consumed.assign(cfg->n_inputs, 0);
    const size_t rows = c->rows();
    c->kk.assign(2 * rows, 0);
    for (size_t i = 0; i < rows; i++) c->kk[rows + i] = kp;
    // the table as the kernel reads it (nvx_tap_plan.h)
    const int R = c->shape.R, G = c->shape.G;
    std::vector<int16_t> table((size_t)L * NVX_TAP_OFFSETS * G * 16, 0);
    for (int r = 0; r < L; r++)
        for (int e = 0; e < NVX_TAP_OFFSETS; e++)
            for (int t = 0; t < T; t++) {
                const int j = T - 1 - t + e;                                    // below R: R >= T + 3
                const int32_t h = taps[(size_t)r * T + t];
                int16_t *group = &table[(((size_t)r * NVX_TAP_OFFSETS + e) * G + j / 8) * 16];
                group[j % 8] = (int16_t)(h >> 8);
                group[8 + j % 8] = (int16_t)(h & 255);
            }
    (void)R;
    std::vector<uint32_t> w(NVX_TAP_GRID);
    for (int j = 0; j < NVX_TAP_GRID; j++) {
        int16_t cc, ss;
        nvx_ddc_w(j, &cc, &ss);
        w[j] = (uint32_t)(uint16_t)cc | ((uint32_t)(uint16_t)ss << 16);
    }
    const size_t table_bytes = table.size() * sizeof(int16_t), state_bytes = (size_t)cfg->n_inputs * T * sizeof(uint32_t);
    hipError_t e = hipMalloc((void **)&c->d_table, table_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_w, w.size() * 4);
    if (e == hipSuccess) e = c->state.allocate(cfg->n_inputs, (size_t)T);
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_kk, 2 * rows * sizeof(int));
    if (e == hipSuccess) e = hipHostMalloc((void **)&c->h_kk, 2 * rows * sizeof(int), hipHostMallocDefault);
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_NOMEM; }
    e = hipEventCreateWithFlags(&c->kk_uploaded, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemcpy(c->d_table, table.data(), table_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->d_w, w.data(), w.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(c->state.d[0], 0, state_bytes);
    if (e == hipSuccess) e = hipMemset(c->state.d[1], 0, state_bytes);
    if (e == hipSuccess) e = hipMemset(c->d_kk, 0, 2 * rows * sizeof(int));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: filling the tables and the state failed: %s", what, hipGetErrorString(e)); release(c); return NVX_ERR_HIP; }
    nvx_tap_prepare();
    *out = c;
    return NVX_OK;
}

extern "C" void nvx_tap_destroy(nvx_tap *c)
{
    if (!c || c->magic != MAGIC) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    release(c);
}

extern "C" int nvx_tap_plan(nvx_tap *c, int *L, int *M, int *T, int *n_inputs, int *n_taps, int *kind)
{
    if (!valid(c, "nvx_tap_plan")) return NVX_ERR_ARG;
    if (L) *L = c->shape.L;
    if (M) *M = c->shape.M;
    if (T) *T = c->shape.T;
    if (n_inputs) *n_inputs = c->n_inputs;
    if (n_taps) *n_taps = c->n_taps;
    if (kind) *kind = c->kind;
    return NVX_OK;
}

// ---------------------------------------------------------------------------------------------------- shifts and pitches
extern "C" int nvx_tap_set_shift(nvx_tap *c, int input, int tap, double hz, double *applied_hz)
{
    const char *what = "nvx_tap_set_shift";
    if (!valid(c, what) || !input_tap_ok(c, what, input, -1, tap)) return NVX_ERR_ARG;
    int k;
    const char *why = "";
    if (nvx_tap_shift_k(c->fo, c->kind, hz, &k, &why) != NVX_OK) { set_error("%s: %g Hz at %u S/s: %s", what, hz, c->fo, why); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    for (int i = input < 0 ? 0 : input; i < (input < 0 ? c->n_inputs : input + 1); i++) c->kk[(size_t)i * c->n_taps + tap] = k;
    c->kk_dirty = true;
    if (applied_hz) *applied_hz = (double)k * NVX_TAP_INPUT_RATE / NVX_TAP_GRID;
    return NVX_OK;
}

extern "C" int nvx_tap_get_shift(nvx_tap *c, int input, int tap, int *k, double *applied_hz)
{
    const char *what = "nvx_tap_get_shift";
    if (!valid(c, what) || !input_tap_ok(c, what, input, 0, tap)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    const int kk = c->kk[(size_t)input * c->n_taps + tap];
    if (k) *k = kk;
    if (applied_hz) *applied_hz = (double)kk * NVX_TAP_INPUT_RATE / NVX_TAP_GRID;
    return NVX_OK;
}

extern "C" int nvx_tap_set_pitch(nvx_tap *c, int input, int tap, double pitch_hz, double *applied_hz)
{
    const char *what = "nvx_tap_set_pitch";
    if (!valid(c, what) || !input_tap_ok(c, what, input, -1, tap)) return NVX_ERR_ARG;
    if (c->kind != NVX_TAP_REAL) { set_error("%s: the plan's kind is NVX_TAP_IQ: only audio has a pitch", what); return NVX_ERR_ARG; }
    int kp;
    const char *why = "";
    if (nvx_tap_pitch_k(c->fo, pitch_hz, &kp, &why) != NVX_OK) { set_error("%s: %g Hz at %u S/s: %s", what, pitch_hz, c->fo, why); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    for (int i = input < 0 ? 0 : input; i < (input < 0 ? c->n_inputs : input + 1); i++) c->kk[c->rows() + (size_t)i * c->n_taps + tap] = kp;
    c->kk_dirty = true;
    if (applied_hz) *applied_hz = (double)kp * c->fo / NVX_TAP_GRID;
    return NVX_OK;
}

extern "C" int nvx_tap_get_pitch(nvx_tap *c, int input, int tap, int *kp, double *applied_hz)
{
    const char *what = "nvx_tap_get_pitch";
    if (!valid(c, what) || !input_tap_ok(c, what, input, 0, tap)) return NVX_ERR_ARG;
    if (c->kind != NVX_TAP_REAL) { set_error("%s: the plan's kind is NVX_TAP_IQ: only audio has a pitch", what); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    const int k = c->kk[c->rows() + (size_t)input * c->n_taps + tap];
    if (kp) *kp = k;
    if (applied_hz) *applied_hz = (double)k * c->fo / NVX_TAP_GRID;
    return NVX_OK;
}

// ------------------------------------------------------------------------------------------------- positions and timing
// `input` (-1: all) stands at input sample `position` with silence in front of it
static int restart(nvx_tap *c, const char *what, int input, uint64_t position)
{
    if (!row_ok(what, "input", input, -1, c->n_inputs)) return NVX_ERR_ARG;
    if (position >> 62) { set_error("%s: position %llu (below 2^62)", what, (unsigned long long)position); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const int first = input < 0 ? 0 : input, n = input < 0 ? c->n_inputs : 1;
    HIP_TRY(hipMemset(c->state.in(first, 0), 0, c->state.bytes(n)));
    HIP_TRY(hipMemset(c->state.in(first, 1), 0, c->state.bytes(n)));
    HIP_TRY(hipDeviceSynchronize());
    for (int i = first; i < first + n; i++) c->consumed[i] = position;
    return NVX_OK;
}

extern "C" int nvx_tap_reset(nvx_tap *c, int input)
{
    return valid(c, "nvx_tap_reset") ? restart(c, "nvx_tap_reset", input, 0) : NVX_ERR_ARG;
}

extern "C" int nvx_tap_debug_set_position(nvx_tap *c, int input, uint64_t position)
{
    return valid(c, "nvx_tap_debug_set_position") ? restart(c, "nvx_tap_debug_set_position", input, position) : NVX_ERR_ARG;
}

extern "C" int nvx_tap_position(nvx_tap *c, int input, uint64_t *consumed, uint64_t *produced)
{
    const char *what = "nvx_tap_position";
    if (!valid(c, what) || !row_ok(what, "input", input, 0, c->n_inputs)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (consumed) *consumed = c->consumed[input];
    if (produced) *produced = nvx_tap_outputs_after(c->consumed[input], c->shape.L, c->shape.M);
    return NVX_OK;
}

extern "C" int nvx_tap_timing(nvx_tap *c, int enable)
{
    return valid(c, "nvx_tap_timing") ? timing_enable(c->mu, c->timer, enable) : NVX_ERR_ARG;
}

extern "C" int nvx_tap_time_stats(nvx_tap *c, double *sum_ms, uint64_t *calls, int reset)
{
    return valid(c, "nvx_tap_time_stats") ? timing_collect(c->mu, c->timer, sum_ms, calls, reset) : NVX_ERR_ARG;
}

extern "C" int64_t nvx_tap_debug_last_launch(nvx_tap *c, int *tile_out, int *tiles, int *form, int *waves, size_t *lds_bytes)
{
    if (!valid(c, "nvx_tap_debug_last_launch")) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->kernel_launches) {
        if (tile_out) *tile_out = c->last.tile_out;
        if (tiles) *tiles = c->last.tiles;
        if (form) *form = c->last.form;
        if (waves) *waves = c->last.waves;
        if (lds_bytes) *lds_bytes = c->last.lds_bytes;
    }
    return c->kernel_launches;
}

// ------------------------------------------------------------------------------------------------------------ launches
// The outputs of a call of n_in samples on an input at `consumed`; false where the position passes 2^62.
static bool call_outputs(const nvx_tap *c, const char *what, uint64_t consumed, size_t n_in, size_t *outs)
{
    if (n_in > NVX_TAP_MAX_IN) { set_error("%s: %zu samples (at most 2^30 per call)", what, n_in); return false; }
    if (!position_ok(what, consumed + n_in)) return false;
    *outs = (size_t)(nvx_tap_outputs_after_wide(consumed + n_in, c->shape.L, c->shape.M) - nvx_tap_outputs_after_wide(consumed, c->shape.L, c->shape.M));
    return true;                                            // L / M < 1: fewer outputs than samples
}

// The shifts and pitches as they stand go to the device in front of the launch, on its stream, from the pinned row; the row is
// not rewritten while an earlier upload may still read it.
static int upload_steps(nvx_tap *c, hipStream_t s)
{
    if (!c->kk_dirty) return NVX_OK;
    HIP_TRY(hipEventSynchronize(c->kk_uploaded));
    memcpy(c->h_kk, c->kk.data(), c->kk.size() * sizeof(int));
    HIP_TRY(hipMemcpyAsync(c->d_kk, c->h_kk, c->kk.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->kk_uploaded, s));
    c->kk_dirty = false;
    return NVX_OK;
}

// One call over inputs [first, first + n) of the plan, every tap of each, which stand at `consumed` and read state row
// `parity`; the caller holds the plan's lock and has checked every span.  n_in is not zero.
static int launch(nvx_tap *c, int first, int n, uint64_t consumed, int parity, const uint32_t *d_in, size_t pitch_in, size_t n_in, void *d_out,
                  size_t pitch_out, size_t out_first, hipStream_t s)
{
    nvx_tap_args a = c->shape;
    const size_t row0 = (size_t)first * c->n_taps;
    a.in = d_in; a.pitch_in = pitch_in; a.out = d_out; a.pitch_out = pitch_out; a.out_first = out_first;
    a.state_in = c->state.in(first, parity); a.state_out = c->state.out(first, parity);
    a.table = c->d_table; a.w = c->d_w; a.k = c->d_kk + row0; a.kp = c->d_kk + c->rows() + row0;
    nvx_tap_fill_args(consumed, n_in, &a);
    int rc;
    if ((rc = upload_steps(c, s)) != NVX_OK) return rc;
    nvx_event_timer::events ev;
    if ((rc = c->timer.begin(s, ev)) != NVX_OK) return rc;
    HIP_TRY(nvx_tap_launch(&a, c->kind, n, s));
    c->last = { a.tile_out, a.tiles, a.uniform ? 1 : 2, a.tile_out >> 6, nvx_tap_lds_bytes(&a) };
    c->kernel_launches += 1;
    if ((rc = c->timer.end(s, ev)) != NVX_OK) return rc;
    for (int i = first; i < first + n; i++) c->consumed[i] = consumed + n_in;
    c->state.flip(first, n, parity);
    return NVX_OK;
}

extern "C" int nvx_tap_resident(nvx_tap *c, const void *d_in, size_t pitch_in, size_t n_in, void *d_out, size_t pitch_out, size_t out_first,
                                size_t *n_out, void *hip_stream)
{
    const char *what = "nvx_tap_resident";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t osize = c->out_size();
    if (!d_in || !d_out || ((uintptr_t)d_in & 3) || ((uintptr_t)d_out & (osize - 1))) {
        set_error("%s: bad argument (null pointer, input not 4-byte aligned, or output not aligned to its sample)", what);
        return NVX_ERR_ARG;
    }
    if (!all_stand_together(what, "input", c->consumed)) return NVX_ERR_STATE;
    const uint64_t consumed = c->consumed[0];
    size_t outs;
    if (!call_outputs(c, what, consumed, n_in, &outs)) return NVX_ERR_ARG;
    // every row's last sample read and last sample written, in samples of its row (out_end) and in bytes of the whole operand
    const size_t in_rows = (size_t)c->n_inputs, out_rows = c->rows();
    size_t out_end, in_bytes, out_bytes;
    if (__builtin_add_overflow(out_first, outs, &out_end) || !span_bytes(in_rows - 1, pitch_in, n_in, 4, &in_bytes) ||
        !span_bytes(out_rows - 1, pitch_out, out_end, osize, &out_bytes)) {
        set_error("%s: the span of %zu samples of %d inputs at pitch %zu, or of %zu outputs from %zu of %zu rows at pitch %zu, overflows", what, n_in,
                  c->n_inputs, pitch_in, outs, out_first, out_rows, pitch_out);
        return NVX_ERR_ARG;
    }
    if ((in_rows > 1 && n_in > pitch_in) || (out_rows > 1 && out_end > pitch_out)) {
        set_error("%s: %zu samples per input at pitch %zu, outputs up to %zu at pitch %zu (a row must hold them)", what, n_in, pitch_in, out_end, pitch_out);
        return NVX_ERR_ARG;
    }
    if (n_out) *n_out = outs;
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_in, in_bytes, what, "input")) != NVX_OK) return rc;
    if (outs && (rc = check_device_span(d_out, out_bytes, what, "output")) != NVX_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    // the state rows of inputs pushed one by one are brought to input 0's parity
    if ((rc = c->state.align(nullptr, s)) != NVX_OK) return rc;
    return launch(c, 0, c->n_inputs, consumed, c->state.parity[0], (const uint32_t *)d_in, pitch_in, n_in, d_out, pitch_out, out_first, s);
}

extern "C" int nvx_tap_push(nvx_tap *c, int input, const void *in, size_t n_in, int16_t *out, size_t cap_samples, size_t *n_out)
{
    const char *what = "nvx_tap_push";
    if (!valid(c, what)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (input < 0 || input >= c->n_inputs || !in || !out) {
        set_error("%s: bad argument (input %d of %d, or null pointer)", what, input, c->n_inputs);
        return NVX_ERR_ARG;
    }
    const uint64_t consumed = c->consumed[input];
    size_t outs, cap_bytes;
    if (!call_outputs(c, what, consumed, n_in, &outs)) return NVX_ERR_ARG;
    if (outs > cap_samples) { set_error("%s: %zu samples give %zu outputs per tap, the buffer holds %zu: nothing consumed", what, n_in, outs, cap_samples); return NVX_ERR_ARG; }
    const size_t osize = c->out_size();
    if (!span_bytes((size_t)c->n_taps - 1, cap_samples, outs, osize, &cap_bytes)) { set_error("%s: %d taps of %zu samples overflow", what, c->n_taps, cap_samples); return NVX_ERR_ARG; }
    if (n_out) *n_out = outs;
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(c->device, NOUN)) != NVX_OK) return rc;
    const size_t pitch = outs ? outs : 1, out_bytes = (size_t)c->n_taps * pitch * osize;
    if ((rc = c->push.reserve(what, n_in * 4, (out_bytes + 3) / 4)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(c->push.d_in, in, n_in * 4, hipMemcpyHostToDevice));
    if ((rc = launch(c, input, 1, consumed, c->state.parity[input], (const uint32_t *)c->push.d_in, n_in, n_in, c->push.d_out, pitch, 0, nullptr)) != NVX_OK) return rc;
    if (outs) HIP_TRY(hipMemcpy2D(out, cap_samples * osize, c->push.d_out, pitch * osize, outs * osize, (size_t)c->n_taps, hipMemcpyDeviceToHost));
    else HIP_TRY(hipStreamSynchronize(nullptr));
    return NVX_OK;
}
