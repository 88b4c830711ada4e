/* nvx_align_plan.h -- what the row aligner's host side (nvx_align_host.cpp), its host-only parts (nvx_align_find.c) and its
 * kernels (nvx_align.hip) share: the kernels' arguments, the layout of a pair's state row, the launch arithmetic
 * (nvx_align_fill_args and nvx_align_fill_measure_args, pure functions: tests/harness/align_launch_args.cpp walks them without
 * a device), and the tests' two hooks.  Internal. */
#ifndef NVX_ALIGN_PLAN_H
#define NVX_ALIGN_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_align.h"
#include "nvx_stream_plan.h"

#define NVX_ALIGN_THREADS 256
#define NVX_ALIGN_WAVES 4
#define NVX_ALIGN_REGION 1024               /* outputs of a tile a wave takes */
#define NVX_ALIGN_TILE (NVX_ALIGN_WAVES * NVX_ALIGN_REGION)     /* outputs a workgroup takes per step */
#define NVX_ALIGN_MIN_CHUNK_TILES 4
#define NVX_ALIGN_TARGET_WORKGROUPS 2048    /* a pair's tiles are spread over chunks until the grid has about this many */
#define NVX_ALIGN_MAX_IN (1u << 30)         /* samples per call and pair */
/* A pair's state row, in 32-bit words: the last H = max_delay + T converted samples of the main row (sample consumed - H + j
 * in word j; zero in front of the reset), then those of the sense row. */
#define NVX_ALIGN_HISTORY(max_delay) ((max_delay) + NVX_ALIGN_TAPS)
#define NVX_ALIGN_STATE_WORDS(max_delay) (2 * NVX_ALIGN_HISTORY(max_delay))
/* the measure kernel: a workgroup takes 64 lags and tiles of 1024 main samples, a wave 256 of them, 128 per 32-bit partial */
#define NVX_ALIGN_M_LAGS 64
#define NVX_ALIGN_M_TILE 1024
#define NVX_ALIGN_M_FOLD 128
#define NVX_ALIGN_M_TARGET_WORKGROUPS 2048

#ifdef __cplusplus
extern "C" {
#endif

/* the shipped taps (nvx_align_find.c): h_f[k] at taps[f * NVX_ALIGN_TAPS + k] */
int nvx_align_design_taps(int16_t *taps);

/* For tests: the shape of the plan's last nvx_align_resident or nvx_align_push -- workgroups per pair, tiles of 4096 outputs
 * a full workgroup walks, and the form (1: one workgroup per pair, 2: a pair spread over several).  Returns the kernel
 * launches made since creation (0: nothing was written); any pointer may be NULL. */
NVX_API int64_t nvx_align_debug_last_launch(nvx_row_aligner *al, int *chunks, int *tiles_per_chunk, int *form);
/* For tests: `pair` (-1: every pair) stands at `position` as after a reset there: the samples in front of it count as zero. */
NVX_API int nvx_align_debug_set_position(nvx_row_aligner *al, int pair, uint64_t position);

#ifdef __cplusplus
}

struct nvx_align_args {
    const void *in_main;       /* [n_pairs][pitch_main] samples in the plan's format */
    const void *in_sense;      /* [n_pairs][pitch_sense] */
    size_t pitch_main, pitch_sense;      /* samples */
    uint32_t *out_main, *out_sense;      /* [n_pairs][pitch_out_*] packed words */
    size_t pitch_out_main, pitch_out_sense, out_first;
    const uint32_t *state_in;  /* [n_pairs][state_words] */
    uint32_t *state_out;
    const int32_t *delays;     /* [n_pairs] delay_q5 */
    const uint32_t *taps;      /* [32][8] words: (h_f[15 - 2q] & 0xffff) | (h_f[14 - 2q] << 16) */
    int n_in;
    int tiles, tiles_per_chunk;          /* blockIdx.x walks tiles [x * tiles_per_chunk, ...) of pair blockIdx.y */
    int history, state_words;            /* H, 2 H */
    int history_per_chunk;               /* words of each row's carried samples blockIdx.x writes: [x * this, ...) */
    int vec_main, vec_sense;             /* every row of that output is 16-byte aligned */
};

/* the delays of part 3 from delay_q5; the kernel calls it too */
#ifdef __HIP__
__host__ __device__
#endif
static inline void nvx_align_split_delay(int d, int *dm, int *ds, int *f)
{
    if (d >= 0) { *dm = (d + 31) >> 5; *ds = 0; *f = 32 * *dm - d; }
    else { *dm = 0; *ds = (-d) >> 5; *f = (-d) & 31; }
}

/* The arguments of one call over n_pairs pairs.  `wanted` is how many workgroups the caller would spread a pair over; the
 * number the grid gets is returned. */
static inline int nvx_align_fill_args(const void *d_main, size_t pitch_main, const void *d_sense, size_t pitch_sense, size_t n_in, uint32_t *d_out_main,
                                      size_t pitch_out_main, uint32_t *d_out_sense, size_t pitch_out_sense, size_t out_first, int n_pairs,
                                      const uint32_t *state_in, uint32_t *state_out, const int32_t *delays, const uint32_t *taps, int max_delay,
                                      int wanted, nvx_align_args *out)
{
    nvx_align_args a = {};
    a.in_main = d_main; a.pitch_main = pitch_main; a.in_sense = d_sense; a.pitch_sense = pitch_sense;
    a.out_main = d_out_main; a.pitch_out_main = pitch_out_main; a.out_sense = d_out_sense; a.pitch_out_sense = pitch_out_sense; a.out_first = out_first;
    a.state_in = state_in; a.state_out = state_out; a.delays = delays; a.taps = taps;
    a.n_in = (int)n_in;
    a.tiles = (int)((n_in + NVX_ALIGN_TILE - 1) / NVX_ALIGN_TILE);
    const int chunks = nvx_stream_chunks(a.tiles, wanted, NVX_ALIGN_MIN_CHUNK_TILES, &a.tiles_per_chunk);
    a.history = NVX_ALIGN_HISTORY(max_delay); a.state_words = NVX_ALIGN_STATE_WORDS(max_delay);
    a.history_per_chunk = (a.history + chunks - 1) / chunks;
    a.vec_main = nvx_stream_rows_aligned16(d_out_main, pitch_out_main, out_first, n_pairs);
    a.vec_sense = nvx_stream_rows_aligned16(d_out_sense, pitch_out_sense, out_first, n_pairs);
    *out = a;
    return chunks;
}

struct nvx_align_measure_args {
    const void *in_main, *in_sense;
    size_t pitch_main, pitch_sense;      /* samples */
    unsigned long long *table;           /* [n_pairs][n_lags][2], from zero */
    unsigned long long *power;           /* [n_pairs][2], from zero */
    int n_in, lag_first, n_lags;
    int n0, window;                      /* the main row's first sample, N */
    int tiles, tiles_per_chunk;          /* blockIdx.y walks tiles of 1024 main samples [y * tiles_per_chunk, ...) */
};

/* The arguments of one measurement; returns the chunks (gridDim.y), 0 where the call is refused.  The grid is
 * (n_lags / 64, chunks, n_pairs). */
static inline int nvx_align_fill_measure_args(const void *d_main, size_t pitch_main, const void *d_sense, size_t pitch_sense, size_t n_in, int lag_first,
                                              int n_lags, int n_pairs, unsigned long long *table, unsigned long long *power, nvx_align_measure_args *out)
{
    nvx_align_measure_args a = {};
    const uint64_t window = nvx_align_window(n_in, lag_first, n_lags);
    if (!window) return 0;
    a.in_main = d_main; a.pitch_main = pitch_main; a.in_sense = d_sense; a.pitch_sense = pitch_sense; a.table = table; a.power = power;
    a.n_in = (int)n_in; a.lag_first = lag_first; a.n_lags = n_lags;
    a.n0 = lag_first < 0 ? -lag_first : 0; a.window = (int)window;
    a.tiles = (a.window + NVX_ALIGN_M_TILE - 1) / NVX_ALIGN_M_TILE;
    const int groups = n_lags / NVX_ALIGN_M_LAGS;
    int wanted = NVX_ALIGN_M_TARGET_WORKGROUPS / (groups * n_pairs);
    const int chunks = nvx_stream_chunks(a.tiles, wanted, 1, &a.tiles_per_chunk);
    *out = a;
    return chunks;
}

#include <hip/hip_runtime.h>
/* the apply kernel on s: grid (chunks, n_pairs) */
hipError_t nvx_align_launch(const nvx_align_args *a, int format, int n_pairs, int chunks, hipStream_t s);
/* the measure kernel on s: grid (n_lags / 64, chunks, n_pairs); the table and the power sums are zeroed by the caller, on s, in front */
hipError_t nvx_align_measure_launch(const nvx_align_measure_args *a, int format, int n_pairs, int chunks, hipStream_t s);
#endif

#endif
