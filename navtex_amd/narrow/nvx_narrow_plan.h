/* nvx_narrow_plan.h -- what the narrowband interpolator's design (nvx_narrow_design.c), its host side (nvx_narrow_host.cpp)
 * and its kernel (nvx_narrow.hip) share: the kernel's arguments, the tap table's layout, the launch arithmetic (pure
 * functions that host and kernel both run: tests/harness/nb_launch_args.cpp walks them without a device), and the tests' two
 * hooks.  Internal. */
#ifndef NVX_NARROW_PLAN_H
#define NVX_NARROW_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_narrow.h"
#include "nvx_polyphase_design.h"
#include "nvx_stream_plan.h"

#define NVX_NB_THREADS 256
#define NVX_NB_MAX_T 32                     /* taps per phase the kernel has registers for */
#define NVX_NB_STATE_WORDS 32               /* a stream's state row: its last T - 1 converted samples, oldest first, packed */
#define NVX_NB_PART_OUTPUTS 32              /* outputs of one window a thread takes at most: J */
#define NVX_NB_STAGE_WORDS 288              /* the tile's input in the LDS: at most 256 windows and 31 samples in front */
#define NVX_NB_OUT_WORDS 8200               /* the tile's outputs in the LDS: at most 8192, behind up to 3 words of alignment */
#define NVX_NB_MIN_CHUNK_TILES 2            /* a later chunk stages the table and up to 31 samples again */
#define NVX_NB_MAX_CHUNKS 4096
#define NVX_NB_TARGET_WORKGROUPS 2048       /* a stream's tiles are spread over chunks until the grid has about this many */
#define NVX_NB_MAX_IN ((size_t)1 << 30)     /* input samples per call and stream */

#ifdef __cplusplus
extern "C" {
#endif

/* L, M, T of a rate; NVX_ERR_ARG and *why for a rate outside the supported range */
int nvx_nb_plan_numbers(uint32_t num, uint32_t den, int *L, int *M, int *T, const char **why);
/* the L * T taps, phase-major taps[r * T + t] */
int nvx_nb_plan_taps(int L, int T, int16_t *taps, const char **why);
/* ceil(n * L / M) for n < 2^63, in full and as its low 64 bits (exact for n below 2^54: L / M is below 2^10) */
static inline unsigned __int128 nvx_nb_outputs_after_wide(uint64_t n, int L, int M) { return nvx_pp_outputs_after_wide(n, L, M); }
static inline uint64_t nvx_nb_outputs_after(uint64_t n, int L, int M) { return nvx_pp_outputs_after(n, L, M); }

/* For tests: the shape of the plan's last call -- workgroups per stream, tiles a full workgroup walks, the form (1: one
 * workgroup per stream, 2: a stream spread over several), the windows (input samples) of a tile, the threads that share a
 * window, and the dynamic LDS bytes.  Returns the kernel launches made since creation (one per call; 0: nothing was
 * written); any pointer may be NULL. */
NVX_API int64_t nvx_nb_debug_last_launch(nvx_nb_interpolator *c, int *chunks, int *tiles_per_chunk, int *form, int *windows, int *parts,
                                         size_t *lds_bytes);
/* For tests: `stream` (-1: every stream) stands at input sample `position` as after a reset there: the samples in front of it
 * count as silence. */
NVX_API int nvx_nb_debug_set_position(nvx_nb_interpolator *c, int stream, uint64_t position);

#ifdef __cplusplus
}

#if defined(__HIPCC__)
#define NVX_NB_HD __host__ __device__ inline
#else
#define NVX_NB_HD inline
#endif

/* The tap table as the kernel reads it: L rows of row_quads 16-byte words.  A row holds Tp = 8 tq int16 (tq = ceil(T / 8)):
 * Tp - T zeros, then the phase's taps reversed (so that taps and samples both ascend: entry j meets x[q - (Tp - 1) + j]), and,
 * where tq is even, one more 16-byte word: a row is an odd number of them, so that rows M apart start on different banks. */
struct nvx_nb_args {
    const void *in;           /* [n_streams][pitch_in] samples in the plan's format and kind */
    size_t pitch_in;          /* samples */
    uint32_t *out;            /* [n_streams][pitch_out] packed words */
    size_t pitch_out, out_first;
    const uint32_t *state_in; /* [n_streams][NVX_NB_STATE_WORDS] */
    uint32_t *state_out;
    const uint32_t *table;    /* the table above, in global memory */
    int n_in, n_out;
    int L, M, T, tq, row_quads, table_quads;
    int windows;              /* input samples of a tile: 256 >> pshift */
    int pshift;               /* 1 << pshift threads share a window, each taking up to `part` of its outputs */
    int part;
    int jlo, lr;              /* L = jlo M + lr: a window has jlo outputs, or one more where its first phase is below lr */
    int tiles, tiles_per_chunk;          /* blockIdx.x walks tiles [x * tiles_per_chunk, ...) of stream blockIdx.y */
    uint32_t e0;              /* the phase of the call's first output: below M */
    uint32_t tile_di, tile_dr;           /* a tile's step:   windows L = tile_di M + tile_dr */
    uint32_t chunk_di, chunk_dr;         /* a chunk's step:  tiles_per_chunk windows L = chunk_di M + chunk_dr */
};

/* n = quot d + rem for n < d << bits, by shifts and subtractions (the kernel has no divider, and its float one is not exact).
 * A loop, not unrolled: it runs once or twice per workgroup, and unrolled it holds every d << b in a scalar register. */
NVX_NB_HD void nvx_nb_divmod(uint32_t n, uint32_t d, int bits, uint32_t *quot, uint32_t *rem)
{
    uint32_t q = 0;
#pragma GCC unroll 1
    for (int b = bits - 1; b >= 0; b--)
        if ((n >> b) >= d) { n -= d << b; q |= 1u << b; }
    *quot = q; *rem = n;
}

/* Positions are counted from the call's first: window k is input sample k, output i the call's i-th.  Window k's first output
 * is i(k) = ceil((k L - e0) / M) and has phase r(k) = i(k) M + e0 - k L, below M.
 * The first window of chunk x: k = x tiles_per_chunk windows. */
NVX_NB_HD void nvx_nb_chunk_start(const nvx_nb_args &a, uint32_t x, uint32_t *i, uint32_t *r)
{
    const uint32_t d = x * a.chunk_dr;                  /* below 2^12 * 2^10 */
    if (d <= a.e0) { *i = x * a.chunk_di; *r = a.e0 - d; return; }
    uint32_t quot, rem;
    nvx_nb_divmod(d - a.e0 + (uint32_t)a.M - 1u, (uint32_t)a.M, 23, &quot, &rem);
    *i = x * a.chunk_di + quot;
    *r = (uint32_t)a.M - 1u - rem;
}

/* ... of the tile behind one that starts at (i, r) */
NVX_NB_HD void nvx_nb_tile_next(const nvx_nb_args &a, uint32_t i, uint32_t r, uint32_t *i2, uint32_t *r2)
{
    const bool carry = a.tile_dr > r;
    *i2 = i + a.tile_di + (carry ? 1u : 0u);
    *r2 = r - a.tile_dr + (carry ? (uint32_t)a.M : 0u);
}

/* ... of window w of a tile that starts at (i, r), where w L = aw M + bw; *count is the number of the window's outputs */
NVX_NB_HD void nvx_nb_window_first(const nvx_nb_args &a, uint32_t i, uint32_t r, uint32_t aw, uint32_t bw, uint32_t *i0, uint32_t *r0, int *count)
{
    const bool carry = bw > r;
    *i0 = i + aw + (carry ? 1u : 0u);
    *r0 = r - bw + (carry ? (uint32_t)a.M : 0u);
    *count = a.jlo + (*r0 < (uint32_t)a.lr ? 1 : 0);
}

static inline size_t nvx_nb_lds_bytes(const nvx_nb_args *a)
{
    return (size_t)a->table_quads * 16 + (NVX_NB_STAGE_WORDS + NVX_NB_OUT_WORDS) * sizeof(uint32_t);
}

/* The shape of a plan: what of nvx_nb_args depends on L, M and T alone. */
static inline void nvx_nb_fill_shape(int L, int M, int T, nvx_nb_args *a)
{
    a->L = L; a->M = M; a->T = T;
    a->tq = (T + 7) / 8;
    a->row_quads = a->tq | 1;
    a->table_quads = L * a->row_quads;
    a->jlo = L / M; a->lr = L % M;
    const int jmax = a->jlo + (a->lr ? 1 : 0);
    a->pshift = jmax <= NVX_NB_PART_OUTPUTS ? 0 : (jmax <= 2 * NVX_NB_PART_OUTPUTS ? 1 : 2);
    a->part = (jmax + (1 << a->pshift) - 1) >> a->pshift;
    a->windows = NVX_NB_THREADS >> a->pshift;
    const uint64_t step = (uint64_t)a->windows * (uint64_t)L;
    a->tile_di = (uint32_t)(step / (uint64_t)M); a->tile_dr = (uint32_t)(step % (uint64_t)M);
}

/* The arguments of one call of n_in > 0 samples over rows that stand at `consumed` samples, on top of nvx_nb_fill_shape.
 * `wanted` is how many workgroups the caller would spread a row over; the number the grid gets is returned: every chunk but
 * the last has tiles_per_chunk tiles, at least NVX_NB_MIN_CHUNK_TILES where there is more than one chunk. */
static inline int nvx_nb_fill_args(uint64_t consumed, const void *d_in, size_t pitch_in, size_t n_in, uint32_t *d_out, size_t pitch_out,
                                   size_t out_first, const uint32_t *state_in, uint32_t *state_out, const uint32_t *table, int wanted,
                                   nvx_nb_args *a)
{
    a->in = d_in; a->pitch_in = pitch_in; a->out = d_out; a->pitch_out = pitch_out; a->out_first = out_first;
    a->state_in = state_in; a->state_out = state_out; a->table = table;
    const unsigned __int128 before = nvx_nb_outputs_after_wide(consumed, a->L, a->M);
    a->n_in = (int)n_in;
    a->n_out = (int)(nvx_nb_outputs_after_wide(consumed + n_in, a->L, a->M) - before);
    a->e0 = (uint32_t)(before * (unsigned)a->M - (unsigned __int128)consumed * (unsigned)a->L);
    a->tiles = (int)((n_in + (size_t)a->windows - 1) / (size_t)a->windows);
    if (wanted > NVX_NB_MAX_CHUNKS) wanted = NVX_NB_MAX_CHUNKS;
    const int chunks = nvx_stream_chunks(a->tiles, wanted, NVX_NB_MIN_CHUNK_TILES, &a->tiles_per_chunk);
    const uint64_t step = (uint64_t)a->tiles_per_chunk * (uint64_t)a->windows * (uint64_t)a->L;
    a->chunk_di = (uint32_t)(step / (uint64_t)a->M); a->chunk_dr = (uint32_t)(step % (uint64_t)a->M);
    return chunks;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
/* the kernel on s: grid (chunks, n_streams) */
hipError_t nvx_nb_launch(const nvx_nb_args *a, int format, int kind, int n_streams, int chunks, hipStream_t s);
void nvx_nb_prepare(void);                  /* once per process: the kernels' LDS limit */
#endif
#endif

#endif
