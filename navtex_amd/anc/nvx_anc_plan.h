/* nvx_anc_plan.h -- what the noise canceller's host side (nvx_anc_host.cpp) and its kernels (nvx_anc.hip) share: the kernels'
 * arguments, the layout of a pair's state row, the launch arithmetic (nvx_anc_fill_args, a pure function:
 * tests/harness/anc_launch_args.cpp walks it without a device), and the tests' two hooks.  Internal. */
#ifndef NVX_ANC_PLAN_H
#define NVX_ANC_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_anc.h"
#include "nvx_stream_plan.h"

#define NVX_ANC_THREADS 256
#define NVX_ANC_WAVES 4
#define NVX_ANC_REGION 1024                 /* samples of a tile a wave takes */
#define NVX_ANC_TILE (NVX_ANC_WAVES * NVX_ANC_REGION)   /* samples a workgroup takes per step; at most one block ends inside */
#define NVX_ANC_MIN_CHUNK_TILES 32          /* a chunk is at least two blocks long where a pair has more than one */
#define NVX_ANC_TARGET_WORKGROUPS 2048      /* a pair's tiles are spread over chunks until the grid has about this many */
#define NVX_ANC_MAX_IN (1u << 30)           /* samples per call and pair */
#define NVX_ANC_SUMS 4                      /* SAA, SBB, SRE, SIM */
/* A pair's state row, in int64 words: the ring of W block sums (block b in slot b mod W), the open block's partial sums,
 * then NVX_ANC_STATE_SCALARS words: the blocks complete since the reset (saturated at W), c_re, c_im, the coherence of the
 * last solve, the mode, the last reason, two spare. */
#define NVX_ANC_STATE_SCALARS 8
#define NVX_ANC_STATE_WORDS(window_log2) (NVX_ANC_SUMS * (1 << (window_log2)) + NVX_ANC_SUMS + NVX_ANC_STATE_SCALARS)
enum { NVX_ANC_ST_COMPLETE = 0, NVX_ANC_ST_CRE, NVX_ANC_ST_CIM, NVX_ANC_ST_COHERENCE, NVX_ANC_ST_MODE, NVX_ANC_ST_REASON };

#ifdef __cplusplus
extern "C" {
#endif

/* For tests: the shape of the plan's last call -- workgroups per pair (the same in both kernels), tiles of 4096 samples a
 * full workgroup walks, block records per pair, and the form (1: one workgroup per pair, 2: a pair spread over several).
 * Returns the kernel launches made since creation (two per call; 0: nothing was written); any pointer may be NULL. */
NVX_API int64_t nvx_anc_debug_last_launch(nvx_noise_canceller *c, int *chunks, int *tiles_per_chunk, int *records, int *form);
/* For tests: `pair` (-1: every pair) stands at `position` as after a reset there: the samples in front of it count as
 * silence, and nothing is solved until W blocks are complete, the one `position` lies in included. */
NVX_API int nvx_anc_debug_set_position(nvx_noise_canceller *c, int pair, uint64_t position);

#ifdef __cplusplus
}

struct nvx_anc_args {
    const void *in_main;       /* [n_pairs][pitch_main] samples in the plan's format */
    const void *in_sense;      /* [n_pairs][pitch_sense] */
    size_t pitch_main, pitch_sense;      /* samples */
    uint32_t *out;            /* [n_pairs][pitch_out] packed words */
    size_t pitch_out, out_first;
    const int64_t *state_in;  /* [n_pairs][state_words] */
    int64_t *state_out;
    unsigned long long *records;         /* [n_pairs][blocks][NVX_ANC_SUMS]: the sums of the call's samples per block, from zero */
    unsigned long long *counters;        /* [n_pairs][2]: blocks solved, blocks rejected */
    int n_in;
    int tiles, tiles_per_chunk;          /* blockIdx.x walks tiles [x * tiles_per_chunk, ...) of pair blockIdx.y */
    int off0;                 /* 0 .. 65535: the call's first sample is sample off0 of its block */
    int blocks;               /* the blocks the call touches: record r holds block (position div 65536) + r */
    int slot0;                /* the ring slot of the call's first block */
    int window_log2, state_words;
    int out_vec;              /* every row of the output is 16-byte aligned */
};

/* The arguments of one call over n_pairs pairs that stand at `consumed`.  `wanted` is how many workgroups the caller would
 * spread a pair over; the number the grid gets is returned: every chunk but the last has tiles_per_chunk tiles, at least
 * NVX_ANC_MIN_CHUNK_TILES where there is more than one chunk. */
static inline int nvx_anc_fill_args(uint64_t consumed, const void *d_main, size_t pitch_main, const void *d_sense, size_t pitch_sense, size_t n_in,
                                    uint32_t *d_out, size_t pitch_out, size_t out_first, int n_pairs, const int64_t *state_in, int64_t *state_out,
                                    unsigned long long *records, unsigned long long *counters, int window_log2, int wanted, nvx_anc_args *out)
{
    nvx_anc_args a = {};
    a.in_main = d_main; a.pitch_main = pitch_main; a.in_sense = d_sense; a.pitch_sense = pitch_sense;
    a.out = d_out; a.pitch_out = pitch_out; a.out_first = out_first;
    a.state_in = state_in; a.state_out = state_out; a.records = records; a.counters = counters;
    a.n_in = (int)n_in;
    a.tiles = (int)((n_in + NVX_ANC_TILE - 1) / NVX_ANC_TILE);
    const int chunks = nvx_stream_chunks(a.tiles, wanted, NVX_ANC_MIN_CHUNK_TILES, &a.tiles_per_chunk);
    a.off0 = (int)(consumed % NVX_ANC_BLOCK);
    a.blocks = n_in ? (int)(((uint64_t)a.off0 + n_in - 1) / NVX_ANC_BLOCK) + 1 : 0;
    a.slot0 = (int)((consumed / NVX_ANC_BLOCK) & ((1u << window_log2) - 1));
    a.window_log2 = window_log2; a.state_words = NVX_ANC_STATE_WORDS(window_log2);
    a.out_vec = nvx_stream_rows_aligned16(d_out, pitch_out, out_first, n_pairs);
    *out = a;
    return chunks;
}

#include <hip/hip_runtime.h>
/* both kernels, in order, on s: grid (chunks, n_pairs) each; the records are zeroed by the caller, on s, in front */
hipError_t nvx_anc_launch(const nvx_anc_args *a, int format, int n_pairs, int chunks, hipStream_t s);
#endif

#endif
