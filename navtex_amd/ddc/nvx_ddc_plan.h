/* nvx_ddc_plan.h -- what the down-converter bank's host side (nvx_ddc_host.cpp) and its kernels (nvx_ddc.hip) share, and
 * the tests' two hooks.  Internal.  The tile geometry, the tap table's layout and the design (L, M, T, taps) are the
 * resampler's, and so are the plan's host code and the kernels' common device code: navtex_amd/resample/nvx_resample_plan.h,
 * nvx_rs_host.h, nvx_rs_device.h and nvx_resample_design.c, compiled into this library. */
#ifndef NVX_DDC_PLAN_H
#define NVX_DDC_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_ddc.h"
#include "nvx_resample_plan.h"

#define NVX_DDC_HALF (NVX_DDC_GRID / 2)     /* the LDS holds W[0 .. N/2): the other half turn is its negative */
/* Entry j of the half turn sits at word j + (j >> 5): one word of padding per 32, so that lanes whose j differ by a
 * multiple of 32 (k a multiple of 4) fall on different banks of the 32 that serve a 4-byte LDS read. */
#define NVX_DDC_SLOT(j) ((j) + ((j) >> 5))
#define NVX_DDC_TAB_DW (NVX_DDC_HALF + NVX_DDC_HALF / 32)      /* 2112 words, 8448 bytes */

#ifdef __cplusplus
extern "C" {
#endif

/* For tests: the shape of the handle's last kernel launch, from the values handed to nvx_ddc_launch -- outputs per thread
 * and tile, tiles per row, tiles per workgroup, workgroups per row, the grid's y and z (slices, inputs), whether the tap
 * table went to the LDS, and the dynamic LDS bytes of the launch.  Returns the launches made since creation (0: nothing was
 * written); any pointer may be NULL. */
NVX_API int64_t nvx_ddc_debug_last_launch(nvx_ddc *d, int *K, int *tiles, int *tiles_per_chunk, int *chunks, int *slices,
                                          int *inputs, int *taps_in_lds, size_t *lds_bytes);
/* For tests: puts `input` (-1: every input) at position `consumed` (below 2^62) with silence in front, as if that many
 * zero samples had been consumed since its reset. */
NVX_API int nvx_ddc_debug_set_position(nvx_ddc *d, int input, uint64_t consumed);

#ifdef __cplusplus
}

struct nvx_ddc_args {
    nvx_rs_args rs;           /* the resampler's arguments, per input: in, hist_in, hist_out are [n_inputs] rows; out is
                                 [n_inputs * n_slices] rows */
    const int *k;             /* [n_inputs][n_slices] the slices' shifts, device memory */
    const uint32_t *table;    /* NVX_DDC_TAB_DW words: W[0 .. N/2) as packed (c low, s high) at NVX_DDC_SLOT(j) */
    int n_slices;
    uint32_t n0;              /* the call's first sample is the input's sample n with n mod N = n0 */
};

#include <hip/hip_runtime.h>
/* grid (chunks, n_slices, n_inputs) */
hipError_t nvx_ddc_launch(const nvx_ddc_args *a, int format, int n_inputs, int chunks, bool taps_in_lds, hipStream_t s);
size_t nvx_ddc_lds_bytes(const nvx_ddc_args *a, bool taps_in_lds);
void nvx_ddc_prepare(void);
#endif

#endif
