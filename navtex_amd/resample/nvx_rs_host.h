// nvx_rs_host.h -- the polyphase plan the resampler (nvx_resample_host.cpp) and the down-converter bank
// (navtex_amd/ddc/nvx_ddc_host.cpp) both run: the plan's numbers and tap table, its carried positions and history rows,
// the launch arithmetic of nvx_rs_args, the checks of a resident call and the staging of a push.  The rows, the staging, the
// row and position checks and the timing bodies are nvx_companion.h's, the chunk split nvx_stream_plan.h's.  Internal, and all
// of it static: each library compiles its own copy and they share no state.
//
// A plan has `n_inputs` input rows (the resampler's streams, the bank's inputs).  A call writes `out_rows` output rows:
// one per input row in the resampler, one per slice of each in the bank.
#ifndef NVX_RS_HOST_H
#define NVX_RS_HOST_H

#include <mutex>
#include <vector>

#include "nvx_companion.h"
#include "nvx_resample_plan.h"
#include "nvx_stream_plan.h"

static const int NVX_RS_BPS[4] = { 4, 2, 2, 8 };          // bytes per input sample, by format
static const int NVX_RS_TARGET_WORKGROUPS = 2048;         // a row's tiles are spread over chunks until the grid has about this many

struct nvx_rs_plan {
    const char *const library, *const noun;      // for the sentences: "the resampler" and "stream", "the down-converter bank" and "input"
    nvx_rs_plan(const char *library_, const char *noun_) : library(library_), noun(noun_) {}
    std::mutex mu;
    int device = 0, n_inputs = 0, format = 0;
    uint32_t rate = 0;
    int L = 0, M = 0, T = 0, Tp = 0, row_dw = 0, tap_dw = 0, K = 0;
    bool taps_in_lds = false;
    uint32_t dq = 0, dr = 0;
    uint32_t *d_taps = nullptr;
    nvx_state_rows<uint32_t> hist;               // [n_inputs][words]: the T - 1 converted samples in front of an input's next call
    std::vector<uint64_t> consumed;
    nvx_event_timer timer;
    nvx_push_staging push;
};

// ------------------------------------------------------------------------------------------------------ without a device
// The numbers that follow from L, M, T; false where one tile's input does not fit the kernel's staging area.
static inline bool nvx_rs_plan_shape(nvx_rs_plan &p, int L, int M, int T)
{
    p.L = L; p.M = M; p.T = T;
    p.Tp = (T + NVX_RS_ALIGN - 1 + 3) & ~3;
    p.row_dw = p.Tp / 2 + ((p.Tp / 4) % 2 == 0 ? 2 : 0);      // an odd number of 8-byte words: 32 consecutive phases, 32 bank pairs
    p.tap_dw = (NVX_RS_ALIGN * L * p.row_dw + 3) & ~3;
    p.taps_in_lds = (size_t)p.tap_dw * 4 <= NVX_RS_TAPS_LDS_MAX;
    p.dq = (uint32_t)(NVX_RS_THREADS * (uint64_t)M / L); p.dr = (uint32_t)(NVX_RS_THREADS * (uint64_t)M % L);
    p.hist.words = (size_t)((T - 1 + 3) & ~3);
    // the largest tile whose input span fits the planes: (256 K - 1) M / L + 1 samples between its first and last window
    // end, T - 1 in front, up to 7 + 15 of rounding to groups
    for (p.K = NVX_RS_MAX_K; p.K > 1; p.K--)
        if (((uint64_t)(NVX_RS_THREADS * p.K - 1) * M) / L + 2 + T + 24 <= NVX_RS_PLANE) break;
    return ((uint64_t)(NVX_RS_THREADS * p.K - 1) * M) / L + 2 + T + 24 <= NVX_RS_PLANE;
}

// The arguments of one launch over input rows [first_input, ...) of the plan, which stand at `consumed` and read history
// row `parity`.  `chunks` is how many workgroups the caller would spread a row's tiles over; the number the grid gets is
// returned: at most one per tile, and equal shares.
static inline int nvx_rs_fill_args(const nvx_rs_plan &p, int first_input, uint64_t consumed, int parity, const void *d_in, size_t pitch_in,
                                   size_t n_in, uint32_t *d_out, size_t pitch_out, size_t out_first, size_t n_out, int chunks, nvx_rs_args *out)
{
    nvx_rs_args a{};
    a.in = d_in; a.pitch_in = pitch_in; a.out = d_out; a.pitch_out = pitch_out; a.out_first = out_first;
    a.hist_in = p.hist.in(first_input, parity); a.hist_out = p.hist.out(first_input, parity);
    a.taps = p.d_taps;
    a.hist_pitch = (int)p.hist.words; a.hist_valid = consumed > 0;
    a.n_in = (int)n_in; a.n_out = (int)n_out;
    a.L = p.L; a.M = p.M; a.T = p.T; a.Tp = p.Tp; a.row_dw = p.row_dw; a.tap_dw = p.tap_dw; a.K = p.K;
    a.dq = p.dq; a.dr = p.dr;
    // output 0 of the call is the row's output n0 = ceil(consumed L / M): n0 M = Q0 L + r0, and Q0 >= consumed
    const uint64_t n0 = nvx_rs_outputs_after(consumed, p.L, p.M);
    const unsigned __int128 pos = (unsigned __int128)n0 * (unsigned)p.M;
    a.r0 = (uint32_t)(pos % (unsigned)p.L);
    a.qoff = (int)((uint64_t)(pos / (unsigned)p.L) - consumed);
    const int tile_out = NVX_RS_THREADS * p.K;
    a.tiles = (int)((n_out + tile_out - 1) / tile_out);
    chunks = nvx_stream_chunks(a.tiles, chunks, 1, &a.tiles_per_chunk);
    // the steps the kernel advances its positions by, as (div L, mod L)
    const uint64_t uL = (uint64_t)p.L, tile_pos = (uint64_t)tile_out * p.M, chunk_pos = tile_pos * (uint64_t)a.tiles_per_chunk;
    a.tile_dq = (uint32_t)(tile_pos / uL); a.tile_dr = (uint32_t)(tile_pos % uL);
    a.chunk_dq = (uint32_t)(chunk_pos / uL); a.chunk_dr = (uint32_t)(chunk_pos % uL);
    a.span_q = (uint32_t)((tile_pos - p.M) / uL); a.span_r = (uint32_t)((tile_pos - p.M) % uL);
    a.m_div = (uint32_t)(p.M / p.L); a.m_mod = (uint32_t)(p.M % p.L);
    *out = a;
    return chunks;
}

// --------------------------------------------------------------------------------------------------------------- plans
static inline void nvx_rs_plan_release(nvx_rs_plan &p)
{
    (void)hipFree(p.d_taps);
    p.hist.release(); p.push.release();
    p.timer.destroy();
}

// The design of `rate`, the device, the tap table and the zeroed history rows.  What it allocated before a failure is the
// caller's to release (nvx_rs_plan_release).
static inline int nvx_rs_plan_create(nvx_rs_plan &p, const char *what, int device, int n_inputs, int format, uint32_t rate)
{
    int L, M, T;
    const char *why = "";
    if (nvx_rs_plan_numbers(rate, &L, &M, &T, &why) != NVX_OK) { set_error("%s: %u S/s: %s", what, rate, why); return NVX_ERR_ARG; }
    std::vector<int16_t> taps((size_t)L * T);
    int rc = nvx_rs_plan_taps(rate, L, T, taps.data(), &why);
    if (rc != NVX_OK) { set_error("%s: %u S/s: %s", what, rate, why); return rc; }
    if ((rc = select_device(device, p.library)) != NVX_OK) return rc;
    p.device = device; p.n_inputs = n_inputs; p.format = format; p.rate = rate;
    if (!nvx_rs_plan_shape(p, L, M, T)) { set_error("%s: %u S/s: one tile's input does not fit the kernel's staging area", what, rate); return NVX_ERR_ARG; }
    p.consumed.assign(n_inputs, 0);

    // the table the kernel reads: copy `shift` of phase r holds h[r][T-1-i] at position shift + i
    std::vector<uint16_t> table((size_t)p.tap_dw * 2, 0);
    for (int sh = 0; sh < NVX_RS_ALIGN; sh++)
        for (int ph = 0; ph < L; ph++)
            for (int i = 0; i < T; i++)
                table[((size_t)(sh * L + ph) * p.row_dw) * 2 + sh + i] = (uint16_t)taps[(size_t)ph * T + (T - 1 - i)];
    hipError_t e = hipMalloc((void **)&p.d_taps, (size_t)p.tap_dw * 4);
    if (e == hipSuccess) e = p.hist.allocate(n_inputs, p.hist.words);
    if (e != hipSuccess) { set_error("%s: allocation failed: %s", what, hipGetErrorString(e)); return NVX_ERR_NOMEM; }
    e = hipMemcpy(p.d_taps, table.data(), (size_t)p.tap_dw * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(p.hist.d[0], 0, p.hist.bytes(n_inputs));
    if (e == hipSuccess) e = hipMemset(p.hist.d[1], 0, p.hist.bytes(n_inputs));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: filling the tables failed: %s", what, hipGetErrorString(e)); return NVX_ERR_HIP; }
    return NVX_OK;
}

static inline int nvx_rs_reset(nvx_rs_plan &p, const char *what, int input)
{
    if (!row_ok(what, p.noun, input, -1, p.n_inputs)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(p.mu);
    // a row at position 0 has silence in front: its history rows are not read before they are written again
    for (int i = input < 0 ? 0 : input; i < (input < 0 ? p.n_inputs : input + 1); i++) p.consumed[i] = 0;
    return NVX_OK;
}

static inline int nvx_rs_position(nvx_rs_plan &p, const char *what, int input, uint64_t *consumed, uint64_t *produced)
{
    if (!row_ok(what, p.noun, input, 0, p.n_inputs)) return NVX_ERR_ARG;
    std::lock_guard<std::mutex> lk(p.mu);
    if (consumed) *consumed = p.consumed[input];
    if (produced) *produced = nvx_rs_outputs_after(p.consumed[input], p.L, p.M);
    return NVX_OK;
}

// --------------------------------------------------------------------------------------------------------------- calls
// What a call works with once its position is known.  The callers hold p.mu from here on.
struct nvx_rs_call {
    uint64_t consumed;        // where the call's input rows stand
    int parity;               // the history row they read
    size_t outs;              // outputs per output row
    size_t out_end, in_bytes, out_bytes;         // a resident call's spans: see nvx_rs_resident_spans
};

// the position's bound and the output count, for a call of n_in samples from `consumed`
static inline int nvx_rs_call_count(const nvx_rs_plan &p, const char *what, uint64_t consumed, size_t n_in, nvx_rs_call *c)
{
    if (!position_ok(what, consumed + n_in)) return NVX_ERR_ARG;
    c->consumed = consumed;
    c->outs = (size_t)(nvx_rs_outputs_after(consumed + n_in, p.L, p.M) - nvx_rs_outputs_after(consumed, p.L, p.M));
    return NVX_OK;
}

// A resident call, first step: the operands' pointers, every input row at the same position, the count.
static inline int nvx_rs_resident_open(const nvx_rs_plan &p, const char *what, const void *d_in, size_t n_in, const void *d_out,
                                       nvx_rs_call *c)
{
    if (!d_in || !d_out || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 3) || n_in > NVX_RS_MAX_IN) {
        set_error("%s: bad argument (null pointer, input not 16-byte aligned, output not 4-byte aligned, or more than 2^30 samples)", what);
        return NVX_ERR_ARG;
    }
    if (!all_stand_together(what, p.noun, p.consumed)) return NVX_ERR_STATE;
    c->parity = p.hist.parity[0];
    return nvx_rs_call_count(p, what, p.consumed[0], n_in, c);
}

// Second step: every row's last sample read and last word written, in samples of its row (out_end) and in bytes of the
// whole operand.  False where one of them overflows; the sentence is the caller's.
static inline bool nvx_rs_resident_spans(const nvx_rs_plan &p, size_t out_rows, size_t pitch_in, size_t n_in, size_t pitch_out, size_t out_first,
                                         nvx_rs_call *c)
{
    return !__builtin_add_overflow(out_first, c->outs, &c->out_end) && c->outs <= 0x7fffffffu &&
           span_bytes((size_t)(p.n_inputs - 1), pitch_in, n_in, (size_t)NVX_RS_BPS[p.format], &c->in_bytes) &&
           span_bytes(out_rows - 1, pitch_out, c->out_end, 4, &c->out_bytes);
}

// Third step: rows hold what the call puts in them, the spans lie in their allocations, and the history rows of inputs
// pushed one by one are brought to input 0's parity (on `s`).  A call of no samples passes the first of these only: it
// launches nothing.
static inline int nvx_rs_resident_ready(nvx_rs_plan &p, const char *what, size_t out_rows, const void *d_in, size_t pitch_in, size_t n_in,
                                        const void *d_out, size_t pitch_out, const nvx_rs_call &c, hipStream_t s)
{
    if ((p.n_inputs > 1 && (n_in > pitch_in || ((pitch_in * (size_t)NVX_RS_BPS[p.format]) & 15))) || (out_rows > 1 && c.out_end > pitch_out)) {
        set_error("%s: %zu samples per %s at pitch %zu, outputs up to %zu at pitch %zu (a row must hold them, and input rows are 16-byte aligned)",
                  what, n_in, p.noun, pitch_in, c.out_end, pitch_out);
        return NVX_ERR_ARG;
    }
    if (n_in == 0) return NVX_OK;
    int rc;
    if ((rc = select_device(p.device, p.library)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_in, c.in_bytes, what, "input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_out, c.out_bytes, what, "output")) != NVX_OK) return rc;
    return p.hist.align(nullptr, s);
}

// behind a launch over input rows [first_input, first_input + n): they have consumed n_in more and read the other row next
static inline void nvx_rs_advance(nvx_rs_plan &p, int first_input, int n, size_t n_in, const nvx_rs_call &c)
{
    for (int i = first_input; i < first_input + n; i++) p.consumed[i] = c.consumed + n_in;
    p.hist.flip(first_input, n, c.parity);
}

// A push, first step: the arguments and the count.  Whether the caller's buffer holds the outputs is the caller's check.
static inline int nvx_rs_push_open(const nvx_rs_plan &p, const char *what, int input, const void *in, size_t n_in, const void *out_iq,
                                   size_t cap_samples, nvx_rs_call *c)
{
    if (input < 0 || input >= p.n_inputs || !in || (!out_iq && cap_samples) || n_in > NVX_RS_MAX_IN) {
        set_error("%s: bad argument (%s %d of %d, null pointer, or more than 2^30 samples)", what, p.noun, input, p.n_inputs);
        return NVX_ERR_ARG;
    }
    c->parity = p.hist.parity[input];
    return nvx_rs_call_count(p, what, p.consumed[input], n_in, c);
}

// Second step: the device, staging for the samples and for out_words packed outputs, and the samples on the device.
static inline int nvx_rs_push_stage(nvx_rs_plan &p, const char *what, const void *in, size_t n_in, size_t out_words)
{
    int rc;
    if ((rc = select_device(p.device, p.library)) != NVX_OK) return rc;
    const size_t in_bytes = n_in * (size_t)NVX_RS_BPS[p.format];
    if ((rc = p.push.reserve(what, in_bytes, out_words)) != NVX_OK) return rc;
    HIP_TRY(hipMemcpy(p.push.d_in, in, in_bytes, hipMemcpyHostToDevice));
    return NVX_OK;
}

#endif
