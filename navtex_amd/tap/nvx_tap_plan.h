/* nvx_tap_plan.h -- what the channel tap's design (nvx_tap_design.c), its host side (nvx_tap_host.cpp) and its kernel
 * (nvx_tap.hip) share: the kernel's arguments, the tap table's layout, the launch arithmetic (pure functions that host and
 * kernel both run: tests/harness/tap_launch_args.cpp walks them without a device), and the tests' two hooks.  Internal. */
#ifndef NVX_TAP_PLAN_H
#define NVX_TAP_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_tap.h"
#include "nvx_polyphase_design.h"

#define NVX_TAP_THREADS 256                 /* a workgroup's threads at most: one output each */
#define NVX_TAP_LDS_BUDGET (80 * 1024)      /* a workgroup takes a tile of 256 outputs, or of 128 where 256 do not stage within this */
#define NVX_TAP_BLOCK_GROUPS 32             /* groups of 8 taps between two widenings: 255 * 32768 * 256 < 2^31 */
#define NVX_TAP_MAX_IN ((size_t)1 << 30)    /* input samples per call and input */

#ifdef __cplusplus
extern "C" {
#endif

/* L, M, T of a rate and kind; NVX_ERR_ARG and *why outside the supported range */
int nvx_tap_plan_numbers(uint32_t fo, int kind, int *L, int *M, int *T, const char **why);
/* the L * T taps, phase-major taps[r * T + t] */
int nvx_tap_plan_taps(uint32_t fo, int kind, int L, int T, int32_t *taps, const char **why);
/* the grid steps of a shift and of a pitch */
int nvx_tap_shift_k(uint32_t fo, int kind, double hz, int *k, const char **why);
int nvx_tap_pitch_k(uint32_t fo, double pitch_hz, int *kp, const char **why);

/* ceil(n * L / M) for n < 2^63, in full and as its low 64 bits */
static inline unsigned __int128 nvx_tap_outputs_after_wide(uint64_t n, int L, int M) { return nvx_pp_outputs_after_wide(n, L, M); }
static inline uint64_t nvx_tap_outputs_after(uint64_t n, int L, int M) { return nvx_pp_outputs_after(n, L, M); }

/* For tests: the shape of the plan's last call -- the outputs of a tile (the workgroup's threads), the tiles of a row, the
 * form (1: taps wave-uniform through the scalar cache; 2: taps per lane through the vector cache), the waves of a
 * workgroup (a wave takes every waves-th output of the tile), and the dynamic LDS bytes.  Returns the kernel launches made since creation (one per call;
 * 0: nothing was written); any pointer may be NULL. */
NVX_API int64_t nvx_tap_debug_last_launch(nvx_tap *c, int *tile_out, int *tiles, int *form, int *waves, size_t *lds_bytes);
/* For tests: `input` (-1: every input) stands at input sample `position` as after a reset there: the samples in front of it
 * count as silence. */
NVX_API int nvx_tap_debug_set_position(nvx_tap *c, int input, uint64_t position);

#ifdef __cplusplus
}

#if defined(__HIPCC__)
#define NVX_TAP_HD __host__ __device__ inline
#else
#define NVX_TAP_HD inline
#endif

/* The tap table as the kernel reads it, in global memory: per phase r and offset e = 0 .. 3 a row of G = R / 8 groups of 32
 * bytes, R = T + 3 rounded up to a multiple of 8.  Entry j of the row is the phase's tap h[r][T - 1 - (j - e)] (zero outside
 * e <= j < T + e): taps reversed, so that taps and samples both ascend, behind e zeros.  A lane whose window starts e
 * samples behind a multiple of 4 of the staged planes takes the row e and starts e samples earlier: everything it reads
 * from a plane is an aligned 8-byte word.  A group holds 8 int16 of hh = h >> 8, then 8 int16 of hl = h & 255. */
#define NVX_TAP_OFFSETS 4
struct nvx_tap_args {
    const uint32_t *in;       /* [n_inputs][pitch_in] packed words */
    size_t pitch_in;
    void *out;                /* [n_inputs * n_taps][pitch_out] words (IQ) or int16 (REAL) */
    size_t pitch_out, out_first;
    const uint32_t *state_in; /* [n_inputs][state_pitch]: the input's last T - 1 words, oldest first */
    uint32_t *state_out;
    const int16_t *table;     /* the table above */
    const uint32_t *w;        /* W[j] as (c & 0xffff) | (s << 16), j = 0 .. 4095 */
    const int *k, *kp;        /* [n_inputs * n_taps]: the rows' shifts and pitches, in grid steps */
    int state_pitch;
    int n_taps;
    int n_in, n_out;
    int L, M, T, R, G;
    int tile_out;             /* outputs of a tile = threads of a workgroup: 256 or 128 */
    int uniform;              /* L = 1 and waves * M a multiple of 4: the lanes of a wave share the row (phase 0, one e) */
    int stage_len;            /* samples of a staged plane (a multiple of 8) */
    int tiles;
    uint32_t q0, r0;          /* the call's first output: its q relative to the call's first sample, and its phase */
    uint32_t tile_dq, tile_dr;           /* a tile's step: tile_out M = tile_dq L + tile_dr */
    uint32_t n0, m0;          /* the call's first input and output index since the reset, mod 4096 */
};

/* n = quot d + rem for n < d << bits, by shifts and subtractions (the kernel has no divider, and its float one is not exact).
 * A loop, not unrolled: it runs once per workgroup. */
NVX_TAP_HD void nvx_tap_divmod64(uint64_t n, uint32_t d, int bits, uint32_t *quot, uint32_t *rem)
{
    uint64_t q = 0;
#pragma GCC unroll 1
    for (int b = bits - 1; b >= 0; b--)
        if ((n >> b) >= d) { n -= (uint64_t)d << b; q |= (uint64_t)1 << b; }
    *quot = (uint32_t)q; *rem = (uint32_t)n;
}

/* Positions are counted from the call's first input sample and first output.  The first output of tile t: its q and phase. */
NVX_TAP_HD void nvx_tap_tile_start(const nvx_tap_args &a, uint32_t t, uint32_t *q, uint32_t *r)
{
    uint32_t quot, rem;
    nvx_tap_divmod64((uint64_t)a.r0 + (uint64_t)t * a.tile_dr, (uint32_t)a.L, 36, &quot, &rem);
    *q = a.q0 + t * a.tile_dq + quot;
    *r = rem;
}

/* Which output of its tile thread tid takes: wave w of W takes outputs w, w + W, w + 2 W, ...; where L = 1 their windows
 * start W M samples apart, and with W M a multiple of 4 at one offset e. */
NVX_TAP_HD int nvx_tap_thread_output(int tile_out, int tid) { return (tile_out >> 6) * (tid & 63) + (tid >> 6); }

/* The first staged sample of a tile whose first output has q = qt, relative to the call's first sample: a multiple of 4, at
 * or below the first sample of that output's window; may be negative. */
NVX_TAP_HD int nvx_tap_stage_first(const nvx_tap_args &a, uint32_t qt) { return (int)(((int64_t)qt - a.T + 1) & ~(int64_t)3); }

static inline size_t nvx_tap_lds_bytes(const nvx_tap_args *a) { return (size_t)a->stage_len * 4; }

static inline int nvx_tap_stage_len(int L, int M, int R, int tile_out)
{
    const int span = (int)(((int64_t)(L - 1) + (int64_t)(tile_out - 1) * M) / L);
    return (span + 3 + R + 7) & ~7;
}

/* The shape of a plan: what of nvx_tap_args depends on L, M and T alone. */
static inline void nvx_tap_fill_shape(int L, int M, int T, nvx_tap_args *a)
{
    a->L = L; a->M = M; a->T = T;
    a->R = (T + 3 + 7) & ~7; a->G = a->R / 8;
    a->tile_out = NVX_TAP_THREADS;
    while (a->tile_out > 128 && (size_t)nvx_tap_stage_len(L, M, a->R, a->tile_out) * 4 > NVX_TAP_LDS_BUDGET) a->tile_out >>= 1;
    a->stage_len = nvx_tap_stage_len(L, M, a->R, a->tile_out);
    a->uniform = (L == 1 && ((a->tile_out >> 6) * M) % 4 == 0) ? 1 : 0;
    const uint64_t step = (uint64_t)a->tile_out * (uint64_t)M;
    a->tile_dq = (uint32_t)(step / (uint64_t)L); a->tile_dr = (uint32_t)(step % (uint64_t)L);
}

/* The arguments of one call of n_in > 0 samples over inputs that stand at `consumed` samples, on top of nvx_tap_fill_shape.
 * Returns the tiles of a row: the grid's x, at least 1 (a call without outputs still carries the state over). */
static inline int nvx_tap_fill_args(uint64_t consumed, size_t n_in, nvx_tap_args *a)
{
    const unsigned __int128 before = nvx_tap_outputs_after_wide(consumed, a->L, a->M);
    a->n_in = (int)n_in;
    a->n_out = (int)(nvx_tap_outputs_after_wide(consumed + n_in, a->L, a->M) - before);
    const unsigned __int128 pos0 = before * (unsigned)a->M;
    a->q0 = (uint32_t)(pos0 / (unsigned)a->L - consumed);
    a->r0 = (uint32_t)(pos0 % (unsigned)a->L);
    a->n0 = (uint32_t)(consumed % NVX_TAP_GRID);
    a->m0 = (uint32_t)(before % NVX_TAP_GRID);
    a->tiles = a->n_out ? (a->n_out + a->tile_out - 1) / a->tile_out : 1;
    return a->tiles;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
/* the kernel on s: grid (tiles, n_taps, n_inputs) */
hipError_t nvx_tap_launch(const nvx_tap_args *a, int kind, int n_inputs, hipStream_t s);
void nvx_tap_prepare(void);                 /* once per process: the kernels' LDS limit */
#endif
#endif

#endif
