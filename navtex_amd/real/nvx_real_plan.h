/* nvx_real_plan.h -- what the real-input converter's host side (nvx_real_host.cpp) and its kernel (nvx_real.hip) share: the
 * kernel's arguments, the layout of a stream's state row, the launch arithmetic (nvx_real_fill_args, a pure function:
 * tests/harness/real_launch_args.cpp walks it without a device), and the tests' two hooks.  Internal. */
#ifndef NVX_REAL_PLAN_H
#define NVX_REAL_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_real.h"
#include "nvx_real_taps.h"
#include "nvx_stream_plan.h"

#define NVX_REAL_THREADS 256
#define NVX_REAL_WAVES 4
#define NVX_REAL_REGION 1024                /* outputs of a tile a wave loads the sample pairs of */
#define NVX_REAL_TILE (NVX_REAL_WAVES * NVX_REAL_REGION)   /* outputs a workgroup takes per step: T */
#define NVX_REAL_MIN_CHUNK_TILES 4          /* a later chunk reads 28 pairs twice: 0.2 % of four tiles */
#define NVX_REAL_TARGET_WORKGROUPS 2048     /* a stream's tiles are spread over chunks until the grid has about this many */
#define NVX_REAL_MAX_IN ((size_t)1 << 31)   /* samples per call and stream */
/* A stream's state row: the last NVX_REAL_HISTORY converted sample pairs, oldest first, e in the low half of a word and o in
 * the high half. */
#define NVX_REAL_STATE_WORDS NVX_REAL_HISTORY
/* The tile's LDS image: e and o as int16, NVX_REAL_HALO_AT - NVX_REAL_HISTORY unused entries, the halo, the tile. */
#define NVX_REAL_HALO_AT 32
#define NVX_REAL_LDS_ENTRIES (NVX_REAL_HALO_AT + NVX_REAL_TILE)

#ifdef __cplusplus
extern "C" {
#endif

/* For tests: the shape of the plan's last call -- workgroups per stream, tiles of 4096 outputs a full workgroup walks, and
 * the form (1: one workgroup per stream, 2: a stream spread over several).  Returns the kernel launches made since creation
 * (one per call; 0: nothing was written); any pointer may be NULL. */
NVX_API int64_t nvx_real_debug_last_launch(nvx_real_converter *c, int *chunks, int *tiles_per_chunk, int *form);
/* For tests: `stream` (-1: every stream) stands at sample `position` (even) as after a reset there: the samples in front of
 * it count as silence. */
NVX_API int nvx_real_debug_set_position(nvx_real_converter *c, int stream, uint64_t position);

#ifdef __cplusplus
}

struct nvx_real_args {
    const void *in;           /* [n_streams][pitch_in] samples in the plan's format */
    size_t pitch_in;          /* samples */
    uint32_t *out;            /* [n_streams][pitch_out] packed words */
    size_t pitch_out, out_first;
    const uint32_t *state_in; /* [n_streams][NVX_REAL_STATE_WORDS] */
    uint32_t *state_out;
    int n;                    /* outputs of the call = sample pairs = n_in / 2 */
    int tiles, tiles_per_chunk;          /* blockIdx.x walks tiles [x * tiles_per_chunk, ...) of stream blockIdx.y */
    int par;                  /* the parity of m - K of the call's first output: output i of the call has s = +1 where par + i is even */
    int invert;
    int out_vec;              /* every row of the output is 16-byte aligned */
};

/* The arguments of one call over n_streams rows that stand at `consumed` samples (even).  `wanted` is how many workgroups the
 * caller would spread a row over; the number the grid gets is returned: every chunk but the last has tiles_per_chunk tiles,
 * at least NVX_REAL_MIN_CHUNK_TILES where there is more than one chunk. */
static inline int nvx_real_fill_args(uint64_t consumed, const void *d_in, size_t pitch_in, size_t n_in, uint32_t *d_out, size_t pitch_out,
                                     size_t out_first, int n_streams, const uint32_t *state_in, uint32_t *state_out, int invert, int wanted,
                                     nvx_real_args *out)
{
    nvx_real_args a = {};
    a.in = d_in; a.pitch_in = pitch_in; a.out = d_out; a.pitch_out = pitch_out; a.out_first = out_first;
    a.state_in = state_in; a.state_out = state_out;
    a.n = (int)(n_in / 2);
    a.tiles = (int)((n_in / 2 + NVX_REAL_TILE - 1) / NVX_REAL_TILE);
    const int chunks = nvx_stream_chunks(a.tiles, wanted, NVX_REAL_MIN_CHUNK_TILES, &a.tiles_per_chunk);
    /* output i of the call is the stream's m = consumed / 2 + i, and m - K has the parity of m + K */
    a.par = (int)((consumed / 2 + NVX_REAL_K) & 1);
    a.invert = invert;
    a.out_vec = nvx_stream_rows_aligned16(d_out, pitch_out, out_first, n_streams);
    *out = a;
    return chunks;
}

#include <hip/hip_runtime.h>
/* the kernel on s: grid (chunks, n_streams) */
hipError_t nvx_real_launch(const nvx_real_args *a, int format, int n_streams, int chunks, hipStream_t s);
#endif

#endif
