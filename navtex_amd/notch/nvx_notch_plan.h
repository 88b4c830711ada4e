/* nvx_notch_plan.h -- what the tone notch's host side (nvx_notch_host.cpp) and its kernels (nvx_notch.hip) share: the kernels'
 * arguments, the layout of a row's state and of its configuration words, the launch arithmetic (nvx_notch_fill_args, a pure
 * function: tests/harness/notch_launch_args.cpp walks it without a device), and the tests' two hooks.  Internal. */
#ifndef NVX_NOTCH_PLAN_H
#define NVX_NOTCH_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_notch.h"
#include "nvx_stream_plan.h"

#define NVX_NOTCH_THREADS 256
#define NVX_NOTCH_WAVES 4
#define NVX_NOTCH_REGION 1024               /* samples of a tile a wave takes */
#define NVX_NOTCH_TILE (NVX_NOTCH_WAVES * NVX_NOTCH_REGION)     /* samples a workgroup takes per step: sixteen blocks */
#define NVX_NOTCH_TILE_M 18                 /* the values of M a tile's words touch */
#define NVX_NOTCH_MIN_CHUNK_TILES 8         /* a workgroup fills its table once: it takes at least this many tiles */
#define NVX_NOTCH_TARGET_WORKGROUPS 2048    /* a row's tiles are spread over chunks until the grid has about this many */
#define NVX_NOTCH_MAX_IN (1u << 30)         /* samples per call and row */
#define NVX_NOTCH_TABLE 4096                /* packed (c, s) words of the NCO table */

/* A row's state, in int64 words: NVX_NOTCH_ROW_SCALARS words (the reset position, one spare), then per notch
 * NVX_NOTCH_NOTCH_WORDS(r) words -- the last H = 2R + 2 complete block sums (re, im), oldest first, the open block's partial
 * sums (re, im), X (re, im), the pair count and the first block behind the last restart --, then the delay line: D packed
 * words, two to an int64.  Every part starts 16-byte aligned. */
#define NVX_NOTCH_ROW_SCALARS 2
#define NVX_NOTCH_HIST(r) (2 * (1 << (r)) + 2)
#define NVX_NOTCH_NOTCH_WORDS(r) (2 * NVX_NOTCH_HIST(r) + 6)
#define NVX_NOTCH_DELAY(r) (((1 << (r)) + 1) * NVX_NOTCH_BLOCK)
#define NVX_NOTCH_DELAY_AT(r, k) (NVX_NOTCH_ROW_SCALARS + (k) * NVX_NOTCH_NOTCH_WORDS(r))
#define NVX_NOTCH_STATE_WORDS(r, k) (NVX_NOTCH_DELAY_AT(r, k) + NVX_NOTCH_DELAY(r) / 2)
enum { NVX_NOTCH_ST_PARTIAL = 0, NVX_NOTCH_ST_X = 2, NVX_NOTCH_ST_PAIRS = 4, NVX_NOTCH_ST_FROM = 5 };       /* behind the H sums */
/* A row's configuration, in uint32 words: the row's flags, one spare, then (step, flags) per notch.  The host keeps them and
 * copies them to the device in front of a call where they changed; RESET, RESTART and MEASURE hold for one call. */
#define NVX_NOTCH_CFG_WORDS(k) (2 + 2 * (k))
#define NVX_NOTCH_ROW_RESET 1u              /* the row starts anew at the call's position */
#define NVX_NOTCH_ENABLED 1u
#define NVX_NOTCH_RESTART 2u                /* set_freq: the sums and the readout start anew */
#define NVX_NOTCH_MEASURE 4u                /* the readout starts anew */

#ifdef __cplusplus
extern "C" {
#endif

/* For tests: the shape of the plan's last call -- workgroups per row (the same in the sums and the apply kernels), tiles of
 * 4096 samples a full workgroup walks, block records per row and notch, and the form (1: one workgroup per row, 2: a row
 * spread over several).  Returns the kernel launches made since creation (three per call; 0: nothing was written); any pointer
 * may be NULL. */
NVX_API int64_t nvx_notch_debug_last_launch(nvx_tone_notch *n, int *chunks, int *tiles_per_chunk, int *records, int *form);
/* For tests: `row` (-1: every row) stands at `position` as after a reset there: the samples in front of it count as silence
 * and the words for them are (0, 0). */
NVX_API int nvx_notch_debug_set_position(nvx_tone_notch *n, int row, uint64_t position);

#ifdef __cplusplus
}

struct nvx_notch_args {
    const void *in;           /* [n_rows][pitch_in] samples in the plan's format */
    size_t pitch_in;          /* samples */
    uint32_t *out;            /* [n_rows][pitch_out] packed words */
    size_t pitch_out, out_first;
    const int64_t *state_in;  /* [n_rows][state_words] */
    int64_t *state_out;
    const uint32_t *cfg;      /* [n_rows][cfg_words] */
    const uint32_t *table;    /* [NVX_NOTCH_TABLE]: c in the low half, s in the high half */
    unsigned long long *records;         /* [n_rows][blocks][n_notches][2]: the sums of the call's samples per block, from zero */
    int64_t position;         /* of the call's first sample */
    uint32_t in_lo, out_lo;   /* the low 32 bits of position and of position - D: what the NCOs of the two kernels count from */
    int n_in, n_rows;
    int tiles, tiles_per_chunk;          /* blockIdx.x walks tiles [x * tiles_per_chunk, ...) of row blockIdx.y */
    int off0;                 /* 0 .. 255: the call's first sample is sample off0 of its block */
    int blocks;               /* the blocks the call touches: record j holds block (position div 256) + j */
    int done;                 /* ... of which so many end inside the call */
    int g0;                   /* off0 - D - 128: word i of the call interpolates at (g0 + i) div 256 and (g0 + i) mod 256, in
                               * blocks counted from the call's first */
    int n_notches, width_log2, delay, hist, notch_words, state_words, cfg_words;
    int out_vec;              /* every row of the output is 16-byte aligned */
};

/* The arguments of one call over n_rows rows that stand at `consumed`.  `wanted` is how many workgroups the caller would
 * spread a row over; the number the grid gets is returned: every chunk but the last has tiles_per_chunk tiles, at least
 * NVX_NOTCH_MIN_CHUNK_TILES where there is more than one chunk. */
static inline int nvx_notch_fill_args(uint64_t consumed, const void *d_in, size_t pitch_in, size_t n_in, uint32_t *d_out, size_t pitch_out,
                                      size_t out_first, int n_rows, const int64_t *state_in, int64_t *state_out, const uint32_t *cfg,
                                      const uint32_t *table, unsigned long long *records, int n_notches, int width_log2, int wanted,
                                      nvx_notch_args *out)
{
    nvx_notch_args a = {};
    a.in = d_in; a.pitch_in = pitch_in; a.out = d_out; a.pitch_out = pitch_out; a.out_first = out_first;
    a.state_in = state_in; a.state_out = state_out; a.cfg = cfg; a.table = table; a.records = records;
    a.n_notches = n_notches; a.width_log2 = width_log2; a.delay = NVX_NOTCH_DELAY(width_log2); a.hist = NVX_NOTCH_HIST(width_log2);
    a.notch_words = NVX_NOTCH_NOTCH_WORDS(width_log2); a.state_words = NVX_NOTCH_STATE_WORDS(width_log2, n_notches);
    a.cfg_words = NVX_NOTCH_CFG_WORDS(n_notches);
    a.position = (int64_t)consumed; a.in_lo = (uint32_t)consumed; a.out_lo = (uint32_t)(consumed - (uint64_t)a.delay);
    a.n_in = (int)n_in; a.n_rows = n_rows;
    a.tiles = (int)((n_in + NVX_NOTCH_TILE - 1) / NVX_NOTCH_TILE);
    const int chunks = nvx_stream_chunks(a.tiles, wanted, NVX_NOTCH_MIN_CHUNK_TILES, &a.tiles_per_chunk);
    a.off0 = (int)(consumed % NVX_NOTCH_BLOCK);
    a.blocks = n_in ? (int)(((uint64_t)a.off0 + n_in - 1) / NVX_NOTCH_BLOCK) + 1 : 0;
    a.done = (int)(((uint64_t)a.off0 + n_in) / NVX_NOTCH_BLOCK);
    a.g0 = a.off0 - a.delay - NVX_NOTCH_BLOCK / 2;
    a.out_vec = nvx_stream_rows_aligned16(d_out, pitch_out, out_first, n_rows);
    *out = a;
    return chunks;
}

#include <hip/hip_runtime.h>
/* the three kernels, in order, on s: sums and apply with the grid (chunks, n_rows), the readout's update with a lane per (row,
 * notch) between them; the records are zeroed by the caller, on s, in front */
hipError_t nvx_notch_launch(const nvx_notch_args *a, int format, int n_rows, int chunks, hipStream_t s);
#endif

#endif
