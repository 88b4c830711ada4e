/* The entry points of include/navtex_amd_zoom.h called with NULL and nonsense arguments: error codes, never a crash, and
 * never a launch (every call here is refused before a device is looked for).  Linked against libnavtex_amd_zoom.so alone,
 * needs no GPU (tests/test_zoom.py runs it in a process of its own). */
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_zoom.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t few[64];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, ni = -1, nz = -1, fmt = -1, k = -1, hist = -1, kz = -7, reach = -1, shift = -1;
    uint64_t n = 7, pos = 7, made = 7;
    size_t n_out = 7;
    double ms = -1.0, applied = -1.0;
    int16_t taps[14];
    void *in = (void *)(uintptr_t)0x100000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_zoom *z = (nvx_zoom *)(uintptr_t)0x300000, *fake = (nvx_zoom *)not_a_plan;
    nvx_zoom_config cfg;

    nvx_zoom_config_default(NULL);
    nvx_zoom_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.format == NVX_ZOOM_CS16 && cfg.n_inputs == 1 && cfg.n_zooms == 1 && cfg.log2_decim == 1, 1);
    EXPECT(nvx_zoom_create(NULL, &z), NVX_ERR_ARG);
    EXPECT(nvx_zoom_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_zoom_create(&cfg, &z), NVX_ERR_ARG);
    EXPECT(z == NULL, 1);
    nvx_zoom_config_default(&cfg); cfg.n_inputs = 0;
    EXPECT(nvx_zoom_create(&cfg, &z), NVX_ERR_ARG);
    nvx_zoom_config_default(&cfg); cfg.n_inputs = 65536;
    EXPECT(nvx_zoom_create(&cfg, &z), NVX_ERR_ARG);
    nvx_zoom_config_default(&cfg); cfg.n_inputs = 8192; cfg.n_zooms = 8;
    EXPECT(nvx_zoom_create(&cfg, &z), NVX_ERR_ARG);
    nvx_zoom_config_default(&cfg); cfg.n_inputs = 0x7fffffff; cfg.n_zooms = 8;
    EXPECT(nvx_zoom_create(&cfg, &z), NVX_ERR_ARG);
    nvx_zoom_config_default(&cfg); cfg.n_zooms = 0;
    EXPECT(nvx_zoom_create(&cfg, &z), NVX_ERR_ARG);
    nvx_zoom_config_default(&cfg); cfg.n_zooms = 9;
    EXPECT(nvx_zoom_create(&cfg, &z), NVX_ERR_ARG);
    nvx_zoom_config_default(&cfg); cfg.log2_decim = 0;
    EXPECT(nvx_zoom_create(&cfg, &z), NVX_ERR_ARG);
    nvx_zoom_config_default(&cfg); cfg.log2_decim = 7;
    EXPECT(nvx_zoom_create(&cfg, &z), NVX_ERR_ARG);
    nvx_zoom_config_default(&cfg); cfg.format = 4;
    EXPECT(nvx_zoom_create(&cfg, &z), NVX_ERR_ARG);
    nvx_zoom_config_default(&cfg); cfg.format = -1;
    EXPECT(nvx_zoom_create(&cfg, &z), NVX_ERR_ARG);
    nvx_zoom_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_zoom_create(&cfg, &z), NVX_ERR_ARG);
    EXPECT(nvx_zoom_last_error() != NULL && nvx_zoom_last_error()[0] != 0, 1);
    nvx_zoom_destroy(NULL);
    nvx_zoom_destroy(fake);

    EXPECT(nvx_zoom_set_shift(NULL, 0, 0, 0), NVX_ERR_ARG);
    EXPECT(nvx_zoom_set_shift(fake, -1, 0, 100), NVX_ERR_ARG);
    EXPECT(nvx_zoom_get_shift(NULL, 0, 0, &kz), NVX_ERR_ARG);
    EXPECT(nvx_zoom_get_shift(fake, 0, 0, NULL), NVX_ERR_ARG);
    EXPECT(kz == -7, 1);
    EXPECT(nvx_zoom_resident(NULL, in, 1024, 1024, out, 1024, 0, &n_out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_zoom_resident(fake, in, 1024, 1024, out, 1024, 0, &n_out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_zoom_resident(fake, in, 1024, 1023, out, 1024, 0, NULL, NULL), NVX_ERR_ARG);
    EXPECT(nvx_zoom_resident(NULL, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, SIZE_MAX, NULL, NULL), NVX_ERR_ARG);
    EXPECT(nvx_zoom_push(NULL, 0, few, 16, few, 32, &n_out), NVX_ERR_ARG);
    EXPECT(nvx_zoom_push(fake, 0, few, 16, few, 32, &n_out), NVX_ERR_ARG);
    EXPECT(nvx_zoom_push(NULL, -1, NULL, SIZE_MAX, NULL, 0, NULL), NVX_ERR_ARG);
    EXPECT(n_out == 7, 1);
    EXPECT(nvx_zoom_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_zoom_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_zoom_position(NULL, 0, &pos, &made), NVX_ERR_ARG);
    EXPECT(nvx_zoom_position(fake, 0, &pos, &made), NVX_ERR_ARG);
    EXPECT(pos == 7 && made == 7, 1);
    EXPECT(nvx_zoom_plan(NULL, &fmt, &ni, &nz, &k, &hist), NVX_ERR_ARG);
    EXPECT(nvx_zoom_plan(fake, &fmt, &ni, &nz, &k, &hist), NVX_ERR_ARG);
    EXPECT(ni == -1 && nz == -1 && fmt == -1 && k == -1 && hist == -1, 1);
    EXPECT(nvx_zoom_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_zoom_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_zoom_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_zoom_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_zoom_last_error(), "not a zoom bank") != NULL, 1);
    /* the grid and the taps need no device and no plan */
    EXPECT(nvx_zoom_grid(0.0, 1.0, &kz, &applied), NVX_ERR_ARG);
    EXPECT(nvx_zoom_grid(-1e6, 1.0, &kz, &applied), NVX_ERR_ARG);
    EXPECT(nvx_zoom_grid(NAN, 1.0, &kz, &applied), NVX_ERR_ARG);
    EXPECT(nvx_zoom_grid(1e6, NAN, &kz, &applied), NVX_ERR_ARG);
    EXPECT(nvx_zoom_grid(1e6, INFINITY, &kz, &applied), NVX_ERR_ARG);
    EXPECT(nvx_zoom_grid(1e6, 6e5, &kz, &applied), NVX_ERR_ARG);
    EXPECT(kz == -7 && applied == -1.0, 1);
    EXPECT(nvx_zoom_grid(4096.0, 2047.0, NULL, NULL), NVX_OK);
    EXPECT(nvx_zoom_grid(4096.0, -2048.0, &kz, &applied), NVX_OK);
    EXPECT(kz == -2048 && applied == -2048.0, 1);
    EXPECT(nvx_zoom_taps(taps, 13, &reach, &shift), NVX_ERR_ARG);
    EXPECT(reach == -1 && shift == -1, 1);
    EXPECT(nvx_zoom_taps(NULL, 0, &reach, &shift), 14);
    EXPECT(reach == 53 && shift == 15, 1);
    EXPECT(nvx_zoom_taps(taps, 14, NULL, NULL), 14);
    EXPECT(taps[0] == 10376 && taps[13] == 1, 1);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("zoom null-safety ok\n");
    return 0;
}
