/* nvx_resample_plan.h -- what the resampler's design (nvx_resample_design.c), its host side (nvx_resample_host.cpp) and
 * its kernels (nvx_resample.hip) share.  Internal.  The plan's host code is nvx_rs_host.h, the kernels' common device code
 * nvx_rs_device.h; the down-converter bank (navtex_amd/ddc/) compiles all three too. */
#ifndef NVX_RESAMPLE_PLAN_H
#define NVX_RESAMPLE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_resample.h"

#define NVX_RS_THREADS 256
#define NVX_RS_ALIGN 4                      /* the kernel reads windows from sample indices that are multiples of 4 (8 bytes) */
#define NVX_RS_PLANE 8704                   /* samples of one component a workgroup stages in the LDS: 17 KB each */
#define NVX_RS_GROUP 8                      /* samples staged per step: 16 bytes of one plane */
#define NVX_RS_MAX_K 16                     /* outputs per thread and tile */
#define NVX_RS_TAPS_LDS_MAX (60 * 1024)     /* bytes of tap table held in the LDS; a larger one is read from global memory */
#define NVX_RS_MAX_IN (1u << 30)            /* input samples per call and stream */

#ifdef __cplusplus
extern "C" {
#endif

/* L, M, T of a rate; NVX_ERR_ARG and *why for a rate outside the supported range */
int nvx_rs_plan_numbers(uint32_t fi, int *L, int *M, int *T, const char **why);
/* the L * T taps, phase-major taps[r * T + t] */
int nvx_rs_plan_taps(uint32_t fi, int L, int T, int16_t *taps, const char **why);
uint64_t nvx_rs_outputs_after(uint64_t n, int L, int M);

/* For tests: the shape of the handle's last kernel launch, from the values handed to nvx_rs_launch -- outputs per thread
 * and tile, tiles per stream, tiles per workgroup, workgroups per stream, whether the tap table went to the LDS, and the
 * dynamic LDS bytes of the launch.  Returns the launches made since creation (0: nothing was written); any pointer may be
 * NULL. */
NVX_API int64_t nvx_resample_debug_last_launch(nvx_resampler *r, int *K, int *tiles, int *tiles_per_chunk, int *chunks,
                                               int *taps_in_lds, size_t *lds_bytes);

#ifdef __cplusplus
}

/* The tap table as the kernel reads it, as 32-bit words: NVX_RS_ALIGN copies [shift][r] of a row of row_dw words.  A row
 * holds the phase's taps reversed (so that taps and samples both ascend) behind `shift` zero taps, zeros up to Tp =
 * T + 3 rounded up to a multiple of 4, and, where Tp / 4 is even, two more words: a row is an odd number of 8-byte words, so
 * that the rows of 32 consecutive phases start on 32 different bank pairs. */
struct nvx_rs_args {
    const void *in;           /* [n_streams][pitch_in] samples in the plan's format */
    size_t pitch_in;          /* samples */
    uint32_t *out;            /* [n_streams][pitch_out] packed words */
    size_t pitch_out, out_first;
    const uint32_t *hist_in;  /* [n_streams][hist_pitch] the T-1 converted samples in front of this call, packed words */
    uint32_t *hist_out;
    const uint32_t *taps;     /* the table above, in global memory */
    int hist_pitch, hist_valid;          /* hist_valid 0: silence in front (a stream at position 0) */
    int n_in, n_out;
    int L, M, T, Tp, row_dw, tap_dw;     /* tap_dw: words of the whole table */
    int K;                    /* outputs per thread and tile: a tile is 256 K outputs */
    int tiles, tiles_per_chunk;          /* blockIdx.x walks tiles [x * tiles_per_chunk, ...) of stream blockIdx.y */
    uint32_t r0;              /* output 0 of this call stands at input position qoff + (r0 + j M) div L, phase (r0 + j M) mod L */
    int qoff;
    uint32_t dq, dr;          /* a thread's step, 256 outputs:  256 M = dq L + dr */
    uint32_t tile_dq, tile_dr;           /* a tile's step:                 256 K M = tile_dq L + tile_dr */
    uint32_t chunk_dq, chunk_dr;         /* a chunk's step:                tiles_per_chunk 256 K M = chunk_dq L + chunk_dr */
    uint32_t span_q, span_r;             /* first to last output of a full tile: (256 K - 1) M = span_q L + span_r */
    uint32_t m_div, m_mod;               /* M = m_div L + m_mod */
};

#include <hip/hip_runtime.h>
/* grid (chunks, n_streams); taps_in_lds: the table fits NVX_RS_TAPS_LDS_MAX */
hipError_t nvx_rs_launch(const nvx_rs_args *a, int format, int n_streams, int chunks, bool taps_in_lds, hipStream_t s);
size_t nvx_rs_lds_bytes(const nvx_rs_args *a, bool taps_in_lds);      /* the dynamic LDS of that launch */
void nvx_rs_prepare(void);                  /* once per process: the kernels' LDS limit */
#endif

#endif
