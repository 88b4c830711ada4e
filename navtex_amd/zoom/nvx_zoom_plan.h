/* nvx_zoom_plan.h -- what the zoom bank's host side (nvx_zoom_host.cpp) and its kernel (nvx_zoom.hip) share: the kernel's
 * arguments, the layout of an input's state row and of the LDS, the launch arithmetic (nvx_zoom_fill_args, a pure function:
 * tests/harness/zoom_launch_args.cpp walks it without a device), and the tests' two hooks.  Internal. */
#ifndef NVX_ZOOM_PLAN_H
#define NVX_ZOOM_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_zoom.h"
#include "nvx_real_taps.h"
#include "nvx_stream_plan.h"

#define NVX_ZOOM_THREADS 256
#define NVX_ZOOM_BLOCK 1024                 /* input samples a workgroup takes per step: a tile is BLOCK >> k outputs */
#define NVX_ZOOM_TILE(k) (NVX_ZOOM_BLOCK >> (k))            /* T: 512 (k = 1) .. 16 (k = 6) */
#define NVX_ZOOM_HISTORY(k) (NVX_ZOOM_STAGE_REACH * ((1 << (k)) - 1))       /* H */
/* A chunk starts with every stage's line empty and walks WARM(k) tiles in front of its first without storing: they fill the
 * lines.  WARM * BLOCK >= H. */
#define NVX_ZOOM_WARM(k) ((NVX_ZOOM_HISTORY(k) + NVX_ZOOM_BLOCK - 1) / NVX_ZOOM_BLOCK)       /* 1, 1, 1, 1, 2, 4 */
#define NVX_ZOOM_MIN_CHUNK_WARMS 8          /* a chunk has at least this many times its warm-up: the halo is 12.5 % at most */
#define NVX_ZOOM_TARGET_WORKGROUPS 1024     /* an input's tiles are spread over chunks until the grid has about this many */
#define NVX_ZOOM_MAX_IN ((size_t)1 << 30)   /* samples per call and input */
/* An input's state row: the last H converted, unmixed samples, oldest first, I in the low half of a word. */
#define NVX_ZOOM_STATE_WORDS(k) NVX_ZOOM_HISTORY(k)
/* The LDS.  Static: the table as 4096 packed (c, s) words and the block's converted samples, 16384 + 4096 bytes.  Dynamic:
 * per zoom and stage s = 1 .. k four planes of int16 -- the even and the odd samples of I, then of Q, of the stage's input --
 * each NVX_ZOOM_LINE_AT - NVX_REAL_HISTORY unused entries, the 28 carried ones, and the block's BLOCK >> s. */
#define NVX_ZOOM_LINE_AT 32
#define NVX_ZOOM_PLANE(s) (NVX_ZOOM_LINE_AT + (NVX_ZOOM_BLOCK >> (s)))                       /* entries of a plane of stage s */
#define NVX_ZOOM_STAGE_AT(s) (4 * NVX_ZOOM_LINE_AT * ((s) - 1) + 4 * (NVX_ZOOM_BLOCK - (NVX_ZOOM_BLOCK >> ((s) - 1))))   /* entries in front of stage s */
#define NVX_ZOOM_ZOOM_ENTRIES(k) NVX_ZOOM_STAGE_AT((k) + 1)
#define NVX_ZOOM_LDS_STATIC (NVX_ZOOM_GRID * 4 + NVX_ZOOM_BLOCK * 4)
#define NVX_ZOOM_LDS_DYNAMIC(k, zooms) ((size_t)(zooms) * NVX_ZOOM_ZOOM_ENTRIES(k) * 2)
#define NVX_ZOOM_LDS_MAX 163840             /* of a gfx950 workgroup */

#ifdef __cplusplus
extern "C" {
#endif

/* For tests: the shape of the plan's last call -- workgroups per input, tiles a full workgroup stores, the tiles it walks in
 * front of them, the form (1: one workgroup per input, 2: an input spread over several) and the LDS bytes of a workgroup.
 * Returns the kernel launches made since creation (one per call; 0: nothing was written); any pointer may be NULL. */
NVX_API int64_t nvx_zoom_debug_last_launch(nvx_zoom *z, int *chunks, int *tiles_per_chunk, int *warm_tiles, int *form, size_t *lds_bytes);
/* For tests: `input` (-1: every input) stands at sample `position` (a multiple of D) as after a reset there: the samples in
 * front of it count as silence. */
NVX_API int nvx_zoom_debug_set_position(nvx_zoom *z, int input, uint64_t position);

#ifdef __cplusplus
}

struct nvx_zoom_args {
    const void *in;           /* [n_inputs][pitch_in] samples in the plan's format */
    size_t pitch_in;          /* samples */
    uint32_t *out;            /* [n_inputs * n_zooms][pitch_out] packed words */
    size_t pitch_out, out_first;
    const uint32_t *state_in; /* [n_inputs][hist] */
    uint32_t *state_out;
    const int *kz;            /* [n_inputs][n_zooms] */
    const uint32_t *table;    /* [4096] packed (c, s) */
    int n_in, n_out;          /* samples and outputs of the call, per input and zoom */
    int tiles, tiles_per_chunk;          /* blockIdx.x stores tiles [x * tiles_per_chunk, ...) of input blockIdx.y ... */
    int warm_tiles;           /* ... behind this many it walks without storing */
    int log2_decim, n_zooms, hist;
    uint32_t n0;              /* the position of the call's first sample, mod 4096 */
    int out_vec;              /* every row of the output is 16-byte aligned */
};

/* The arguments of one call over n_inputs inputs that stand at `consumed` samples.  `wanted` is how many workgroups the
 * caller would spread an input over; the number the grid gets is returned: every chunk but the last has tiles_per_chunk
 * tiles, at least NVX_ZOOM_MIN_CHUNK_WARMS * NVX_ZOOM_WARM(k) where there is more than one chunk.  n_in is a multiple of D. */
static inline int nvx_zoom_fill_args(uint64_t consumed, const void *d_in, size_t pitch_in, size_t n_in, uint32_t *d_out, size_t pitch_out,
                                     size_t out_first, int n_inputs, int n_zooms, int log2_decim, const uint32_t *state_in, uint32_t *state_out,
                                     const int *kz, const uint32_t *table, int wanted, nvx_zoom_args *out)
{
    nvx_zoom_args a = {};
    const int k = log2_decim;
    a.in = d_in; a.pitch_in = pitch_in; a.out = d_out; a.pitch_out = pitch_out; a.out_first = out_first;
    a.state_in = state_in; a.state_out = state_out; a.kz = kz; a.table = table;
    a.n_in = (int)n_in; a.n_out = (int)(n_in >> k);
    a.tiles = (int)((n_in + NVX_ZOOM_BLOCK - 1) / NVX_ZOOM_BLOCK);
    a.warm_tiles = NVX_ZOOM_WARM(k);
    const int chunks = nvx_stream_chunks(a.tiles, wanted, NVX_ZOOM_MIN_CHUNK_WARMS * a.warm_tiles, &a.tiles_per_chunk);
    a.log2_decim = k; a.n_zooms = n_zooms; a.hist = NVX_ZOOM_HISTORY(k);
    a.n0 = (uint32_t)(consumed % NVX_ZOOM_GRID);
    a.out_vec = nvx_stream_rows_aligned16(d_out, pitch_out, out_first, n_inputs * n_zooms);
    *out = a;
    return chunks;
}

#include <hip/hip_runtime.h>
/* once per process: the kernels may take the dynamic LDS of the largest plan */
void nvx_zoom_prepare(void);
/* the kernel on s: grid (chunks, n_inputs) */
hipError_t nvx_zoom_launch(const nvx_zoom_args *a, int format, int n_inputs, int chunks, hipStream_t s);
#endif

#endif
