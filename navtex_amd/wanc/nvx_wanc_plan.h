/* nvx_wanc_plan.h -- what the multi-tap canceller's host side (nvx_wanc_host.cpp) and its kernels (nvx_wanc.hip) share: the
 * kernels' arguments, the layout of a pair's state row and of a block's weight record, the launch arithmetic
 * (nvx_wanc_fill_args, a pure function: tests/harness/wanc_launch_args.cpp walks it without a device), and the tests' two
 * hooks.  Internal. */
#ifndef NVX_WANC_PLAN_H
#define NVX_WANC_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_wanc.h"
#include "nvx_stream_plan.h"

#define NVX_WANC_THREADS 256
#define NVX_WANC_WAVES 4
#define NVX_WANC_REGION 1024                /* samples of a tile a wave takes */
#define NVX_WANC_TILE (NVX_WANC_WAVES * NVX_WANC_REGION)  /* samples a workgroup takes per step; at most one block ends inside */
#define NVX_WANC_PAD 16                     /* sense words staged in front of a tile: K - 1 of them are the halo */
#define NVX_WANC_MIN_CHUNK_TILES 32         /* a chunk is at least two blocks long where a pair has more than one */
#define NVX_WANC_TARGET_WORKGROUPS 2048     /* a pair's tiles are spread over chunks until the grid has about this many */
#define NVX_WANC_MAX_IN (1u << 30)          /* samples per call and pair */
#define NVX_WANC_SOLVE_LANES 16             /* (pair, block) solves per workgroup of the solve kernel */
/* The sums of a block, in this order: Re r[0 .. K), Im r[0 .. K), Re q[0 .. K), Im q[0 .. K), SAA. */
#define NVX_WANC_SUMS(k) (4 * (k) + 1)
/* A pair's state row, in int64 words: the ring of W blocks' sums (block b in slot b mod W), the open block's partial sums,
 * NVX_WANC_STATE_SCALARS words (the blocks complete since the reset saturated at W, the coherence of the last solve, the
 * mode, the last reason, four spare), the weights (w_re[0 .. K), w_im[0 .. K)), the last K - 1 converted sense words (the
 * oldest first) and the last K / 2 converted main words. */
#define NVX_WANC_STATE_SCALARS 8
#define NVX_WANC_ST_SCALARS(k, wl) (NVX_WANC_SUMS(k) * ((1 << (wl)) + 1))
#define NVX_WANC_ST_WEIGHTS(k, wl) (NVX_WANC_ST_SCALARS(k, wl) + NVX_WANC_STATE_SCALARS)
#define NVX_WANC_ST_SENSE(k, wl) (NVX_WANC_ST_WEIGHTS(k, wl) + 2 * (k))
#define NVX_WANC_ST_MAIN(k, wl) (NVX_WANC_ST_SENSE(k, wl) + (k) - 1)
#define NVX_WANC_STATE_WORDS(k, wl) (NVX_WANC_ST_MAIN(k, wl) + (k) / 2)
enum { NVX_WANC_SC_COMPLETE = 0, NVX_WANC_SC_COHERENCE, NVX_WANC_SC_MODE, NVX_WANC_SC_REASON };
/* A block's weight record, in int32 words: w_re[0 .. K), w_im[0 .. K), then the coherence, the reason, whether the block's
 * start was solved (1) or the weights are the carried ones (0), one spare. */
#define NVX_WANC_WREC(k) (2 * (k) + 4)

#ifdef __cplusplus
extern "C" {
#endif

/* For tests: the shape of the plan's last call -- workgroups per pair (the same in the sums and the apply kernel), tiles of
 * 4096 samples a full workgroup walks, block records per pair, and the form (1: one workgroup per pair, 2: a pair spread
 * over several).  Returns the kernel launches made since creation (three per call; 0: nothing was written); any pointer may
 * be NULL. */
NVX_API int64_t nvx_wanc_debug_last_launch(nvx_wide_canceller *c, int *chunks, int *tiles_per_chunk, int *records, int *form);
/* For tests: `pair` (-1: every pair) stands at `position` as after a reset there: the samples in front of it count as
 * silence, and nothing is solved until W blocks are complete, the one `position` lies in included. */
NVX_API int nvx_wanc_debug_set_position(nvx_wide_canceller *c, int pair, uint64_t position);

#ifdef __cplusplus
}

struct nvx_wanc_args {
    const void *in_main;       /* [n_pairs][pitch_main] samples in the plan's format */
    const void *in_sense;      /* [n_pairs][pitch_sense] */
    size_t pitch_main, pitch_sense;      /* samples */
    uint32_t *out;            /* [n_pairs][pitch_out] packed words */
    size_t pitch_out, out_first;
    const int64_t *state_in;  /* [n_pairs][state_words] */
    int64_t *state_out;
    unsigned long long *records;         /* [n_pairs][blocks][NVX_WANC_SUMS(K)]: the sums of the call's samples per block, from zero */
    int32_t *weights;         /* [n_pairs][blocks][NVX_WANC_WREC(K)]: written by the solve kernel, read by the apply kernel */
    unsigned long long *counters;        /* [n_pairs][2]: blocks solved, blocks rejected */
    int n_in, n_pairs;
    int tiles, tiles_per_chunk;          /* blockIdx.x walks tiles [x * tiles_per_chunk, ...) of pair blockIdx.y */
    int off0;                 /* 0 .. 65535: the call's first sample is sample off0 of its block */
    int blocks;               /* the blocks the call touches: record r holds block (position div 65536) + r */
    int slot0;                /* the ring slot of the call's first block */
    int window_log2, n_taps, load_log2, state_words;
    int out_vec;              /* every row of the output is 16-byte aligned */
};

/* The arguments of one call over n_pairs pairs that stand at `consumed`.  `wanted` is how many workgroups the caller would
 * spread a pair over; the number the grid gets is returned: every chunk but the last has tiles_per_chunk tiles, at least
 * NVX_WANC_MIN_CHUNK_TILES where there is more than one chunk. */
static inline int nvx_wanc_fill_args(uint64_t consumed, const void *d_main, size_t pitch_main, const void *d_sense, size_t pitch_sense, size_t n_in,
                                     uint32_t *d_out, size_t pitch_out, size_t out_first, int n_pairs, const int64_t *state_in, int64_t *state_out,
                                     unsigned long long *records, int32_t *weights, unsigned long long *counters, int window_log2, int n_taps,
                                     int load_log2, int wanted, nvx_wanc_args *out)
{
    nvx_wanc_args a = {};
    a.in_main = d_main; a.pitch_main = pitch_main; a.in_sense = d_sense; a.pitch_sense = pitch_sense;
    a.out = d_out; a.pitch_out = pitch_out; a.out_first = out_first;
    a.state_in = state_in; a.state_out = state_out; a.records = records; a.weights = weights; a.counters = counters;
    a.n_in = (int)n_in; a.n_pairs = n_pairs;
    a.tiles = (int)((n_in + NVX_WANC_TILE - 1) / NVX_WANC_TILE);
    const int chunks = nvx_stream_chunks(a.tiles, wanted, NVX_WANC_MIN_CHUNK_TILES, &a.tiles_per_chunk);
    a.off0 = (int)(consumed % NVX_WANC_BLOCK);
    a.blocks = n_in ? (int)(((uint64_t)a.off0 + n_in - 1) / NVX_WANC_BLOCK) + 1 : 0;
    a.slot0 = (int)((consumed / NVX_WANC_BLOCK) & ((1u << window_log2) - 1));
    a.window_log2 = window_log2; a.n_taps = n_taps; a.load_log2 = load_log2;
    a.state_words = NVX_WANC_STATE_WORDS(n_taps, window_log2);
    a.out_vec = nvx_stream_rows_aligned16(d_out, pitch_out, out_first, n_pairs);
    *out = a;
    return chunks;
}

#include <hip/hip_runtime.h>
/* the three kernels, in order, on s: sums and apply on the grid (chunks, n_pairs), the solve with a lane per (pair, block);
 * the records are zeroed by the caller, on s, in front */
hipError_t nvx_wanc_launch(const nvx_wanc_args *a, int format, int n_pairs, int chunks, hipStream_t s);
#endif

#endif
