/* nvx_iqc_plan.h -- what the IQ corrector's host side (nvx_iqc_host.cpp) and its kernels (nvx_iqc.hip) share: the kernels'
 * arguments, the layout of a stream's state row, the launch arithmetic (nvx_iqc_fill_args, a pure function:
 * tests/harness/iqc_launch_args.cpp walks it without a device), and the tests' two hooks.  Internal. */
#ifndef NVX_IQC_PLAN_H
#define NVX_IQC_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_iqc.h"
#include "nvx_stream_plan.h"

#define NVX_IQC_THREADS 256
#define NVX_IQC_WAVES 4
#define NVX_IQC_REGION 1024                 /* samples of a tile a wave takes */
#define NVX_IQC_TILE (NVX_IQC_WAVES * NVX_IQC_REGION)   /* samples a workgroup takes per step; at most one block ends inside */
#define NVX_IQC_MIN_CHUNK_TILES 32          /* a chunk is at least two blocks long where a stream has more than one */
#define NVX_IQC_TARGET_WORKGROUPS 2048      /* a stream's tiles are spread over chunks until the grid has about this many */
#define NVX_IQC_MAX_IN (1u << 30)           /* samples per call and stream */
#define NVX_IQC_SUMS 5                      /* SI, SQ, SII, SQQ, SIQ */
/* A stream's state row, in int64 words: the ring of W block sums (block b in slot b mod W), the open block's partial sums,
 * then NVX_IQC_STATE_SCALARS words: the blocks complete since the reset (saturated at W), dI, dQ, c_i, c_q, the mode, the
 * last reason, one spare. */
#define NVX_IQC_STATE_SCALARS 8
#define NVX_IQC_STATE_WORDS(window_log2) (NVX_IQC_SUMS * (1 << (window_log2)) + NVX_IQC_SUMS + NVX_IQC_STATE_SCALARS)
enum { NVX_IQC_ST_COMPLETE = 0, NVX_IQC_ST_DI, NVX_IQC_ST_DQ, NVX_IQC_ST_CI, NVX_IQC_ST_CQ, NVX_IQC_ST_MODE, NVX_IQC_ST_REASON };

#ifdef __cplusplus
extern "C" {
#endif

/* For tests: the shape of the plan's last call -- workgroups per stream (the same in both kernels), tiles of 4096 samples a
 * full workgroup walks, block records per stream, and the form (1: one workgroup per stream, 2: a stream spread over
 * several).  Returns the kernel launches made since creation (two per call; 0: nothing was written); any pointer may be NULL. */
NVX_API int64_t nvx_iqc_debug_last_launch(nvx_iq_corrector *c, int *chunks, int *tiles_per_chunk, int *records, int *form);
/* For tests: `stream` (-1: every stream) stands at `position` as after a reset there: the samples in front of it count as
 * silence, and nothing is solved until W blocks are complete, the one `position` lies in included. */
NVX_API int nvx_iqc_debug_set_position(nvx_iq_corrector *c, int stream, uint64_t position);

#ifdef __cplusplus
}

struct nvx_iqc_args {
    const void *in;           /* [n_streams][pitch_in] samples in the plan's format */
    size_t pitch_in;          /* samples */
    uint32_t *out;            /* [n_streams][pitch_out] packed words */
    size_t pitch_out, out_first;
    const int64_t *state_in;  /* [n_streams][state_words] */
    int64_t *state_out;
    unsigned long long *records;         /* [n_streams][blocks][NVX_IQC_SUMS]: the sums of the call's samples per block, from zero */
    unsigned long long *counters;        /* [n_streams][2]: blocks solved, blocks rejected */
    int n_in;
    int tiles, tiles_per_chunk;          /* blockIdx.x walks tiles [x * tiles_per_chunk, ...) of stream blockIdx.y */
    int off0;                 /* 0 .. 65535: the call's first sample is sample off0 of its block */
    int blocks;               /* the blocks the call touches: record r holds block (position div 65536) + r */
    int slot0;                /* the ring slot of the call's first block */
    int window_log2, state_words;
    int out_vec;              /* every row of the output is 16-byte aligned */
};

/* The arguments of one call over n_streams rows that stand at `consumed`.  `wanted` is how many workgroups the caller would
 * spread a row over; the number the grid gets is returned: every chunk but the last has tiles_per_chunk tiles, at least
 * NVX_IQC_MIN_CHUNK_TILES where there is more than one chunk. */
static inline int nvx_iqc_fill_args(uint64_t consumed, const void *d_in, size_t pitch_in, size_t n_in, uint32_t *d_out, size_t pitch_out,
                                    size_t out_first, int n_streams, const int64_t *state_in, int64_t *state_out, unsigned long long *records,
                                    unsigned long long *counters, int window_log2, int wanted, nvx_iqc_args *out)
{
    nvx_iqc_args a = {};
    a.in = d_in; a.pitch_in = pitch_in; a.out = d_out; a.pitch_out = pitch_out; a.out_first = out_first;
    a.state_in = state_in; a.state_out = state_out; a.records = records; a.counters = counters;
    a.n_in = (int)n_in;
    a.tiles = (int)((n_in + NVX_IQC_TILE - 1) / NVX_IQC_TILE);
    const int chunks = nvx_stream_chunks(a.tiles, wanted, NVX_IQC_MIN_CHUNK_TILES, &a.tiles_per_chunk);
    a.off0 = (int)(consumed % NVX_IQC_BLOCK);
    a.blocks = n_in ? (int)(((uint64_t)a.off0 + n_in - 1) / NVX_IQC_BLOCK) + 1 : 0;
    a.slot0 = (int)((consumed / NVX_IQC_BLOCK) & ((1u << window_log2) - 1));
    a.window_log2 = window_log2; a.state_words = NVX_IQC_STATE_WORDS(window_log2);
    a.out_vec = nvx_stream_rows_aligned16(d_out, pitch_out, out_first, n_streams);
    *out = a;
    return chunks;
}

#include <hip/hip_runtime.h>
/* both kernels, in order, on s: grid (chunks, n_streams) each; the records are zeroed by the caller, on s, in front */
hipError_t nvx_iqc_launch(const nvx_iqc_args *a, int format, int n_streams, int chunks, hipStream_t s);
#endif

#endif
