/* The entry points of include/navtex_amd_scan.h called with NULL and nonsense arguments: error codes, never a crash,
 * and never a launch (every call here is refused before a device is looked for).  Linked against
 * libnavtex_amd_scan.so alone, needs no GPU (tests/test_scan.py runs it in a process of its own). */
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include "navtex_amd_scan.h"
/* the tests' hook, declared in navtex_amd/scan/nvx_scan_kernels.h (a HIP header) and not in the public one */
int64_t nvx_scan_debug_last_launch(int *form, int *grid_x, int *grid_y, size_t *scratch_bytes);
#define EXPECT(expr, want) do { int r_ = (expr); printf("%-96s -> %d\n", #expr, r_); if (r_ != (want)) bad++; } while (0)
static double row[NVX_SCAN_FFT];
static int16_t few[2 * 1024];
int main(void)
{
    int bad = 0, used = -1, form = -7, gx = -7, gy = -7;
    size_t scratch = 77;
    uint64_t n = 7;
    double ms = -1.0;
    void *in = (void *)(uintptr_t)0x100000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_scan_params p;
    nvx_scan_hit hit[4];

    EXPECT(nvx_scan_resident(0, NULL, 645120, 0, 1, 1, 1, 1, out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_scan_resident(0, in, 645120, 0, 1, 1, 1, 1, NULL, NULL), NVX_ERR_ARG);
    EXPECT(nvx_scan_resident(0, in, 645120, 0, 0, 1, 1, 1, out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_scan_resident(0, in, 645120, 0, -3, 1, 1, 1, out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_scan_resident(0, in, 645120, 0, 1, 0, 1, 1, out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_scan_resident(0, in, 645120, 0, 1, 1, 2, 1, out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_scan_resident(0, in, 645120, 0, 1, 1, 1, 2, out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_scan_resident(0, in, 80640, 0, 1, 1, 0, 3, out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_scan_resident(0, (char *)in + 4, 645120, 0, 1, 1, 1, 1, out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_scan_resident(0, in, 645122, 0, 1, 2, 1, 1, out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_scan_resident(0, in, 645120, 0, 2, 2, 1, 1, out, NULL), NVX_ERR_ARG);          /* two frames, pitch of one */
    EXPECT(nvx_scan_resident(0, in, 645120, SIZE_MAX, 1, 1, 1, 1, out, NULL), NVX_ERR_ARG);   /* first_frame + n wraps */
    EXPECT(nvx_scan_resident(0, in, 645120, SIZE_MAX / 645120, 1, 1, 1, 1, out, NULL), NVX_ERR_ARG);   /* frames * length wraps */
    EXPECT(nvx_scan_resident(0, in, SIZE_MAX & ~(size_t)3, 0, 1, 0x7fffffff, 1, 1, out, NULL), NVX_ERR_ARG);   /* streams * pitch wraps */
    EXPECT(nvx_scan_iq(0, NULL, 645120, 1, 1, row, &used), NVX_ERR_ARG);
    EXPECT(nvx_scan_iq(0, few, 1024, 1, 1, NULL, &used), NVX_ERR_ARG);
    EXPECT(nvx_scan_iq(0, few, 1024, 1, 1, row, &used), NVX_ERR_ARG);                         /* less than a frame */
    EXPECT(nvx_scan_iq(0, few, 1024, 0, 1, row, NULL), NVX_ERR_ARG);
    EXPECT(nvx_scan_iq(0, few, 1024, 5, 1, row, &used), NVX_ERR_ARG);
    EXPECT(used, -1);
    EXPECT(nvx_scan_set_form(3), NVX_ERR_ARG);
    EXPECT(nvx_scan_set_form(-1), NVX_ERR_ARG);
    EXPECT(nvx_scan_set_form(0), NVX_OK);
    nvx_scan_timing(0);
    EXPECT(nvx_scan_time_stats(NULL, NULL, 0), NVX_OK);
    EXPECT(nvx_scan_time_stats(&ms, &n, 1), NVX_OK);
    EXPECT(ms == 0.0 && n == 0, 1);
    EXPECT(nvx_scan_last_error() != NULL && nvx_scan_last_error()[0] != 0, 1);
    EXPECT((int)nvx_scan_debug_last_launch(NULL, NULL, NULL, NULL), 0);                       /* nothing was launched above */
    EXPECT((int)nvx_scan_debug_last_launch(&form, NULL, &gy, NULL), 0);
    EXPECT((int)nvx_scan_debug_last_launch(&form, &gx, &gy, &scratch), 0);
    EXPECT(form == -7 && gx == -7 && gy == -7 && scratch == 77, 1);                           /* and nothing written */

    nvx_scan_params_default(NULL);
    nvx_scan_params_default(&p);
    EXPECT(p.struct_size == sizeof p && p.band_half == 5 && p.floor_half == 32 && p.guard_bins == 13 && p.shadow_bins == 33, 1);
    EXPECT(p.min_score_db == 6.0 && p.shadow_db == 25.0 && p.max_offset_hz == 25000.0 && p.refine_half == 6 && p.refine_iters == 4, 1);
    EXPECT(nvx_scan_find(NULL, &p, hit, 4), NVX_ERR_ARG);
    EXPECT(nvx_scan_find(row, &p, NULL, 4), NVX_ERR_ARG);
    EXPECT(nvx_scan_find(row, &p, hit, -1), NVX_ERR_ARG);
    EXPECT(nvx_scan_find(row, NULL, NULL, 0), 0);                                             /* an all-zero row: no hits */
    EXPECT(nvx_scan_find(row, &p, hit, 4), 0);
    p.struct_size = 8;
    EXPECT(nvx_scan_find(row, &p, hit, 4), NVX_ERR_ARG);
    nvx_scan_params_default(&p); p.floor_half = 0;
    EXPECT(nvx_scan_find(row, &p, hit, 4), NVX_ERR_ARG);
    nvx_scan_params_default(&p); p.band_half = -1;
    EXPECT(nvx_scan_find(row, &p, hit, 4), NVX_ERR_ARG);
    row[5] = -1.0;
    EXPECT(nvx_scan_find(row, NULL, hit, 4), NVX_ERR_ARG);
    row[5] = 0.0; row[7] = NAN;
    EXPECT(nvx_scan_find(row, NULL, hit, 4), NVX_ERR_ARG);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("scan null-safety ok\n");
    return 0;
}
