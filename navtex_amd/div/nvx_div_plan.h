/* nvx_div_plan.h -- what the diversity combiner's host side (nvx_div_host.cpp) and its kernels (nvx_div.hip) share: the kernels'
 * arguments, the layout of a target's state row and of a pair's configuration words, the launch arithmetic (nvx_div_fill_args,
 * a pure function: tests/harness/div_launch_args.cpp walks it without a device), and the tests' two hooks.  Internal. */
#ifndef NVX_DIV_PLAN_H
#define NVX_DIV_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_div.h"
#include "nvx_stream_plan.h"

#define NVX_DIV_THREADS 256
#define NVX_DIV_WAVES 4
#define NVX_DIV_REGION 1024                 /* samples of a tile a wave takes */
#define NVX_DIV_TILE (NVX_DIV_WAVES * NVX_DIV_REGION)       /* samples a workgroup takes per step: sixteen blocks; at most one cell ends inside */
#define NVX_DIV_MIN_CHUNK_TILES 8           /* a workgroup of the sums kernel fills its table once: it takes at least this many tiles */
#define NVX_DIV_TARGET_WORKGROUPS 2048      /* a pair's tiles are spread over chunks until the grid has about this many */
#define NVX_DIV_MAX_IN (1u << 30)           /* samples per call and pair */
#define NVX_DIV_TABLE 4096                  /* packed (c, s) words of the NCO table */
#define NVX_DIV_SUMS 4                      /* SAA, SBB, SRE, SIM of a cell; A re, A im, B re, B im of a block */

/* The state row of one target of one pair, in int64 words: the ring of W cell sums (cell k in slot k mod W), the open cell's
 * partial sums, the open block's partial A and B, then NVX_DIV_STATE_SCALARS words.  A pair's targets lie side by side. */
#define NVX_DIV_STATE_SCALARS 8
#define NVX_DIV_STATE_WORDS(window_log2) (NVX_DIV_SUMS * (1 << (window_log2)) + 2 * NVX_DIV_SUMS + NVX_DIV_STATE_SCALARS)
enum { NVX_DIV_ST_FIRST = 0,                /* F: the first counted cell */
       NVX_DIV_ST_COMPLETE,                 /* cells complete since the restart, saturated at W */
       NVX_DIV_ST_LEAD, NVX_DIV_ST_WRE, NVX_DIV_ST_WIM, NVX_DIV_ST_COHERENCE, NVX_DIV_ST_MODE, NVX_DIV_ST_REASON };
/* A pair's configuration, in uint32 words: the pair's flags, one spare, then NVX_DIV_CFG_TARGET words per target: step, flags,
 * the lead and weight of a pending set, one spare.  The host keeps them and copies them to the device in front of a call
 * where they changed; RESET, RESTART and SET hold for one call. */
#define NVX_DIV_CFG_TARGET 6
#define NVX_DIV_CFG_WORDS(t) (2 + NVX_DIV_CFG_TARGET * (t))
enum { NVX_DIV_CFG_STEP = 0, NVX_DIV_CFG_FLAGS, NVX_DIV_CFG_LEAD, NVX_DIV_CFG_WRE, NVX_DIV_CFG_WIM };
#define NVX_DIV_PAIR_RESET 1u               /* the pair starts anew at the call's position */
#define NVX_DIV_HELD 1u                     /* NVX_DIV_HOLD */
#define NVX_DIV_RESTART 2u                  /* set_freq: the target starts anew at the call's position */
#define NVX_DIV_SET 4u                      /* lead and weight are replaced at the call's first sample */

#ifdef __cplusplus
extern "C" {
#endif

/* For tests: the shape of the plan's last call -- workgroups per pair (the same in the sums and the apply kernels), tiles of
 * 4096 samples a full workgroup walks, block records per pair and target, and the form (1: one workgroup per pair, 2: a pair
 * spread over several).  Returns the kernel launches made since creation (three per call; 0: nothing was written); any
 * pointer may be NULL. */
NVX_API int64_t nvx_div_debug_last_launch(nvx_diversity_combiner *c, int *chunks, int *tiles_per_chunk, int *records, int *form);
/* For tests: `pair` (-1: every pair) stands at `position` as after a reset there: every target's first counted cell is the
 * first whose first sample is at or behind `position`. */
NVX_API int nvx_div_debug_set_position(nvx_diversity_combiner *c, int pair, uint64_t position);

#ifdef __cplusplus
}

struct nvx_div_weight { int32_t lead, w_re, w_im, spare; };

struct nvx_div_args {
    const void *in_main;      /* [n_pairs][pitch_main] samples in the plan's format */
    const void *in_second;    /* [n_pairs][pitch_second] */
    size_t pitch_main, pitch_second;     /* samples */
    uint32_t *out;            /* [n_pairs * n_targets][pitch_out] packed words */
    size_t pitch_out, out_first;
    const int64_t *state_in;  /* [n_pairs][n_targets][state_words] */
    int64_t *state_out;
    const uint32_t *cfg;      /* [n_pairs][cfg_words] */
    const uint32_t *table;    /* [NVX_DIV_TABLE]: c in the low half, s in the high half */
    unsigned long long *records;         /* [n_pairs][blocks][n_targets][NVX_DIV_SUMS]: A and B of the call's samples per block, from zero */
    nvx_div_weight *weights;  /* [n_pairs][cells][n_targets]: lead and weight of every cell the call touches */
    unsigned long long *counters;        /* [n_pairs][n_targets][2]: cells solved, cells rejected */
    int64_t position;         /* of the call's first sample */
    uint32_t in_lo;           /* its low 32 bits: what the NCOs count from */
    int n_in, n_pairs, n_targets;
    int tiles, tiles_per_chunk;          /* blockIdx.x walks tiles [x * tiles_per_chunk, ...) of pair blockIdx.y */
    int off0;                 /* 0 .. 255: the call's first sample is sample off0 of its block */
    int blocks;               /* the blocks the call touches: record j holds block (position div 256) + j */
    int done;                 /* ... of which so many end inside the call */
    int cell_off;             /* 0 .. 65535: the call's first sample is sample cell_off of its cell */
    int cells;                /* the cells the call touches: weight j is that of cell (position div 65536) + j */
    int cells_done;           /* ... of which so many end inside the call */
    int window_log2, state_words, cfg_words;
    int out_vec;              /* every row of the output is 16-byte aligned */
};

/* The arguments of one call over n_pairs pairs that stand at `consumed`.  `wanted` is how many workgroups the caller would
 * spread a pair over; the number the grid gets is returned: every chunk but the last has tiles_per_chunk tiles, at least
 * NVX_DIV_MIN_CHUNK_TILES where there is more than one chunk. */
static inline int nvx_div_fill_args(uint64_t consumed, const void *d_main, size_t pitch_main, const void *d_second, size_t pitch_second, size_t n_in,
                                    uint32_t *d_out, size_t pitch_out, size_t out_first, int n_pairs, int n_targets, const int64_t *state_in,
                                    int64_t *state_out, const uint32_t *cfg, const uint32_t *table, unsigned long long *records, nvx_div_weight *weights,
                                    unsigned long long *counters, int window_log2, int wanted, nvx_div_args *out)
{
    nvx_div_args a = {};
    a.in_main = d_main; a.pitch_main = pitch_main; a.in_second = d_second; a.pitch_second = pitch_second;
    a.out = d_out; a.pitch_out = pitch_out; a.out_first = out_first;
    a.state_in = state_in; a.state_out = state_out; a.cfg = cfg; a.table = table; a.records = records; a.weights = weights; a.counters = counters;
    a.position = (int64_t)consumed; a.in_lo = (uint32_t)consumed;
    a.n_in = (int)n_in; a.n_pairs = n_pairs; a.n_targets = n_targets;
    a.tiles = (int)((n_in + NVX_DIV_TILE - 1) / NVX_DIV_TILE);
    const int chunks = nvx_stream_chunks(a.tiles, wanted, NVX_DIV_MIN_CHUNK_TILES, &a.tiles_per_chunk);
    a.off0 = (int)(consumed % NVX_DIV_BLOCK);
    a.blocks = n_in ? (int)(((uint64_t)a.off0 + n_in - 1) / NVX_DIV_BLOCK) + 1 : 0;
    a.done = (int)(((uint64_t)a.off0 + n_in) / NVX_DIV_BLOCK);
    a.cell_off = (int)(consumed % NVX_DIV_CELL);
    a.cells = n_in ? (int)(((uint64_t)a.cell_off + n_in - 1) / NVX_DIV_CELL) + 1 : 0;
    a.cells_done = (int)(((uint64_t)a.cell_off + n_in) / NVX_DIV_CELL);
    a.window_log2 = window_log2; a.state_words = NVX_DIV_STATE_WORDS(window_log2); a.cfg_words = NVX_DIV_CFG_WORDS(n_targets);
    a.out_vec = nvx_stream_rows_aligned16(d_out, pitch_out, out_first, n_pairs * n_targets);
    *out = a;
    return chunks;
}

#include <hip/hip_runtime.h>
/* the three kernels, in order, on s: sums and apply with the grid (chunks, n_pairs), the fold with a wave per (pair, target)
 * between them; the records are zeroed by the caller, on s, in front, where the call starts inside a block */
hipError_t nvx_div_launch(const nvx_div_args *a, int format, int n_pairs, int chunks, hipStream_t s);
#endif

#endif
