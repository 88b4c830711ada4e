// nvx_scan_kernels.h -- what the scan's launcher (nvx_scan_host.cpp) and its kernels (nvx_scan.hip) share.  Internal.
#ifndef NVX_SCAN_KERNELS_H
#define NVX_SCAN_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_scan.h"

#define NVX_SCAN_MODE_252K 0              // 252 kS/s input
#define NVX_SCAN_MODE_RAW1 1              // 2.016 MS/s input, integrate-and-dump stage 0
#define NVX_SCAN_MODE_RAW3 3              // 2.016 MS/s input, third-order stage 0

#define NVX_SCAN_FRAME_IN  80640          // samples per frame at 252 kS/s: 4 * 20160
#define NVX_SCAN_FRAME_RAW 645120         // ... at 2.016 MS/s
#define NVX_SCAN_SLOT_IN   (4 * NVX_SCAN_SLOT_OUTPUTS)      // 8960
#define NVX_SCAN_SLOT_RAW  (32 * NVX_SCAN_SLOT_OUTPUTS)     // 71680

struct nvx_scan_args {
    const uint32_t *iq;       // [n_streams][pitch] packed IQ
    size_t pitch;             // samples
    size_t first_frame;
    int n_frames, n_streams;
    int mode;                 // NVX_SCAN_MODE_*
    double *power;            // [n_streams][2048]
    double *rows;             // form 2: [n_streams][n_frames][2048] frame rows
};

// form 1: nvx_scan_stream; form 2: nvx_scan_frame + nvx_scan_fold (a->rows must be set).  *first_grid: the grid of the
// first kernel as it was launched
hipError_t nvx_scan_launch(const nvx_scan_args *a, int form, hipStream_t s, dim3 *first_grid);

// For tests: what the last nvx_scan_resident handed nvx_scan_launch -- the form taken (1 or 2), the grid of the first
// kernel, and the bytes of form 2's scratch (0 in form 1).  Returns the launches made by this process so far (0: nothing
// was written); any pointer may be NULL.
extern "C" NVX_API int64_t nvx_scan_debug_last_launch(int *form, int *grid_x, int *grid_y, size_t *scratch_bytes);

#endif
