/* nvx_blank_plan.h -- what the blanker's host side (nvx_blank_host.cpp) and its kernel (nvx_blank.hip) share: the
 * kernel's arguments, the launch arithmetic (nvx_blank_fill_args, a pure function: tests/harness/blank_launch_args.cpp walks
 * it without a device), and the tests' two hooks.  Internal. */
#ifndef NVX_BLANK_PLAN_H
#define NVX_BLANK_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_blank.h"
#include "nvx_stream_plan.h"

#define NVX_BLANK_THREADS 256
#define NVX_BLANK_WAVES 4
#define NVX_BLANK_TILE (NVX_BLANK_WAVES * NVX_BLANK_BLOCK)      /* samples a workgroup takes per step: a block-long region per wave */
#define NVX_BLANK_PREROLL_TILES 2           /* tiles a later chunk reads in front of its own: 8 blocks */
#define NVX_BLANK_MIN_CHUNK_TILES 32        /* a chunk is at least this long, so that the pre-roll stays below 1/16 of it */
#define NVX_BLANK_TARGET_WORKGROUPS 2048    /* a stream's tiles are spread over chunks until the grid has about this many */
#define NVX_BLANK_STATE_WORDS 8             /* a stream's state row: S[b-4] .. S[b-1], the partial sum, the blocks complete since the
                                               reset (saturated at 4), hold + 1 - the distance to the last detection (0: none in
                                               reach), one spare */
#define NVX_BLANK_MAX_IN (1u << 30)         /* samples per call and stream */
#define NVX_BLANK_LDS_BYTES 84              /* per wave two sums and the latest detection; five levels; four fronts */

#ifdef __cplusplus
extern "C" {
#endif

/* For tests: the shape of the plan's last kernel launch -- workgroups per stream, blocks a full workgroup walks, blocks a
 * later workgroup reads in front of its own, and the form (1: one workgroup per stream, 2: a stream spread over several).
 * Returns the launches made since creation (0: nothing was written); any pointer may be NULL. */
NVX_API int64_t nvx_blank_debug_last_launch(nvx_blanker *b, int *chunks, int *blocks_per_chunk, int *preroll_blocks, int *form);
/* For tests: `stream` (-1: every stream) stands at `position` as after a reset there: the samples in front of it count as
 * silence, and nothing is detected until four blocks are complete, the one `position` lies in included. */
NVX_API int nvx_blank_debug_set_position(nvx_blanker *b, int stream, uint64_t position);

#ifdef __cplusplus
}

struct nvx_blank_args {
    const void *in;           /* [n_streams][pitch_in] samples in the plan's format */
    size_t pitch_in;          /* samples */
    uint32_t *out;            /* [n_streams][pitch_out] packed words */
    size_t pitch_out, out_first;
    const uint32_t *state_in; /* [n_streams][NVX_BLANK_STATE_WORDS] */
    uint32_t *state_out;
    unsigned long long *counters;        /* [n_streams][2]: detections, blanked */
    int n_in;
    int tiles, tiles_per_chunk;          /* blockIdx.x walks tiles [x * tiles_per_chunk, ...) of stream blockIdx.y */
    int off;                  /* 1 .. 1024: a wave's region [1024 w, 1024 w + 1024) of a tile ends a block behind its sample off - 1 */
    int hold;
    uint32_t thr_q8, floor;
    int out_vec;              /* every row of the output is 16-byte aligned */
};

/* The arguments of one launch over n_streams rows that stand at `consumed`.  `wanted` is how many workgroups the caller
 * would spread a row over; the number the grid gets is returned: every chunk but the last has tiles_per_chunk tiles, at
 * least NVX_BLANK_MIN_CHUNK_TILES where there is more than one chunk. */
static inline int nvx_blank_fill_args(uint64_t consumed, const void *d_in, size_t pitch_in, size_t n_in, uint32_t *d_out, size_t pitch_out,
                                      size_t out_first, int n_streams, const uint32_t *state_in, uint32_t *state_out,
                                      unsigned long long *counters, uint32_t thr_q8, uint32_t hold, uint32_t floor, int wanted, nvx_blank_args *out)
{
    nvx_blank_args a = {};
    a.in = d_in; a.pitch_in = pitch_in; a.out = d_out; a.pitch_out = pitch_out; a.out_first = out_first;
    a.state_in = state_in; a.state_out = state_out; a.counters = counters;
    a.n_in = (int)n_in;
    a.tiles = (int)((n_in + NVX_BLANK_TILE - 1) / NVX_BLANK_TILE);
    const int chunks = nvx_stream_chunks(a.tiles, wanted, NVX_BLANK_MIN_CHUNK_TILES, &a.tiles_per_chunk);
    a.off = NVX_BLANK_BLOCK - (int)(consumed % NVX_BLANK_BLOCK);
    a.hold = (int)hold; a.thr_q8 = thr_q8; a.floor = floor;
    a.out_vec = nvx_stream_rows_aligned16(d_out, pitch_out, out_first, n_streams);
    *out = a;
    return chunks;
}

#include <hip/hip_runtime.h>
/* grid (chunks, n_streams) */
hipError_t nvx_blank_launch(const nvx_blank_args *a, int format, int n_streams, int chunks, hipStream_t s);
#endif

#endif
