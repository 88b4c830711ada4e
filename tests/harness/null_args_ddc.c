/* The entry points of include/navtex_amd_ddc.h called with NULL and nonsense arguments: error codes, never a crash, and
 * never a launch (every call here is refused before a device is looked for).  Linked against libnavtex_amd_ddc.so alone,
 * needs no GPU (tests/test_ddc.py runs it in a process of its own). */
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_ddc.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t table[2 * NVX_DDC_GRID];
static int16_t few[64];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, L = -1, M = -1, T = -1, ni = -1, ns = -1, fmt = -1, kk = -7;
    uint64_t n = 7, c = 7, p = 7;
    size_t k = 99;
    double ms = -1.0, hz = -1.0;
    void *in = (void *)(uintptr_t)0x100000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_ddc *d = (nvx_ddc *)(uintptr_t)0x300000, *fake = (nvx_ddc *)not_a_plan;
    nvx_ddc_config cfg;

    nvx_ddc_config_default(NULL);
    nvx_ddc_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.n_inputs == 1 && cfg.n_slices == 1 && cfg.input_rate_hz == 2400000 && cfg.format == NVX_DDC_CU8, 1);
    EXPECT(nvx_ddc_create(NULL, &d), NVX_ERR_ARG);
    EXPECT(nvx_ddc_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_ddc_create(&cfg, &d), NVX_ERR_ARG);
    EXPECT(d == NULL, 1);
    nvx_ddc_config_default(&cfg); cfg.n_inputs = 0;
    EXPECT(nvx_ddc_create(&cfg, &d), NVX_ERR_ARG);
    nvx_ddc_config_default(&cfg); cfg.n_slices = 0;
    EXPECT(nvx_ddc_create(&cfg, &d), NVX_ERR_ARG);
    nvx_ddc_config_default(&cfg); cfg.n_inputs = 256; cfg.n_slices = 256;                /* 65536 rows */
    EXPECT(nvx_ddc_create(&cfg, &d), NVX_ERR_ARG);
    nvx_ddc_config_default(&cfg); cfg.n_inputs = 65536;
    EXPECT(nvx_ddc_create(&cfg, &d), NVX_ERR_ARG);
    nvx_ddc_config_default(&cfg); cfg.n_inputs = 0x10000; cfg.n_slices = 0x10000;        /* the product wraps an int */
    EXPECT(nvx_ddc_create(&cfg, &d), NVX_ERR_ARG);
    nvx_ddc_config_default(&cfg); cfg.format = 4;
    EXPECT(nvx_ddc_create(&cfg, &d), NVX_ERR_ARG);
    nvx_ddc_config_default(&cfg); cfg.format = -1;
    EXPECT(nvx_ddc_create(&cfg, &d), NVX_ERR_ARG);
    nvx_ddc_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_ddc_create(&cfg, &d), NVX_ERR_ARG);
    nvx_ddc_config_default(&cfg); cfg.input_rate_hz = 95999;
    EXPECT(nvx_ddc_create(&cfg, &d), NVX_ERR_ARG);
    nvx_ddc_config_default(&cfg); cfg.input_rate_hz = 3200001;
    EXPECT(nvx_ddc_create(&cfg, &d), NVX_ERR_ARG);
    nvx_ddc_config_default(&cfg); cfg.input_rate_hz = 2048001;                           /* L = 252000 */
    EXPECT(nvx_ddc_create(&cfg, &d), NVX_ERR_ARG);
    EXPECT(nvx_ddc_last_error() != NULL && nvx_ddc_last_error()[0] != 0, 1);
    nvx_ddc_destroy(NULL);
    nvx_ddc_destroy(fake);

    EXPECT(nvx_ddc_grid(0, 1000.0, &kk, &hz), NVX_ERR_ARG);
    EXPECT(nvx_ddc_grid(4000000, 1000.0, &kk, &hz), NVX_ERR_ARG);
    EXPECT(nvx_ddc_grid(2400000, NAN, &kk, &hz), NVX_ERR_ARG);
    EXPECT(nvx_ddc_grid(2400000, INFINITY, &kk, &hz), NVX_ERR_ARG);
    EXPECT(nvx_ddc_grid(2400000, 1e300, &kk, &hz), NVX_ERR_ARG);
    EXPECT(nvx_ddc_grid(2400000, 1175500.0, &kk, &hz), NVX_ERR_ARG);                     /* beyond fi / 2 - 25000 */
    EXPECT(nvx_ddc_grid(96000, 24000.0, &kk, &hz), NVX_ERR_ARG);
    EXPECT(kk == -7 && hz == -1.0, 1);
    EXPECT(nvx_ddc_grid(2400000, 612345.0, NULL, NULL), NVX_OK);
    EXPECT(nvx_ddc_grid(2400000, 612345.0, &kk, &hz), NVX_OK);
    EXPECT(kk == 1045 && hz == 1045 * 2400000.0 / 4096, 1);
    EXPECT(nvx_ddc_grid(2400000, -400000.0, &kk, &hz), NVX_OK);
    EXPECT(kk == -683, 1);
    EXPECT(nvx_ddc_table(NULL, 0), NVX_DDC_GRID);
    table[0] = 5;
    EXPECT(nvx_ddc_table(table, NVX_DDC_GRID - 1), NVX_DDC_GRID);                        /* too small: the need, nothing written */
    EXPECT(table[0], 5);
    EXPECT(nvx_ddc_table(table, NVX_DDC_GRID), NVX_DDC_GRID);
    EXPECT(table[0] == 32767 && table[1] == 0 && table[2 * 1024] == 0 && table[2 * 1024 + 1] == 32767 && table[2 * 2048] == -32767, 1);

    EXPECT(nvx_ddc_set_shift(NULL, 0, 0, 1000.0, &hz), NVX_ERR_ARG);
    EXPECT(nvx_ddc_set_shift(fake, -1, 0, 1000.0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_ddc_get_shift(NULL, 0, 0, &kk, &hz), NVX_ERR_ARG);
    EXPECT(nvx_ddc_get_shift(fake, 0, 0, NULL, NULL), NVX_ERR_ARG);
    EXPECT(kk == -683, 1);
    EXPECT(nvx_ddc_resident(NULL, in, 1024, 1024, out, 1024, 0, &k, NULL), NVX_ERR_ARG);
    EXPECT(nvx_ddc_resident(fake, in, 1024, 1024, out, 1024, 0, &k, NULL), NVX_ERR_ARG);
    EXPECT(nvx_ddc_resident(NULL, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, SIZE_MAX, NULL, NULL), NVX_ERR_ARG);
    EXPECT(nvx_ddc_push(NULL, 0, few, 16, few, 16, &k), NVX_ERR_ARG);
    EXPECT(nvx_ddc_push(fake, 0, few, 16, few, 16, &k), NVX_ERR_ARG);
    EXPECT(nvx_ddc_push(NULL, -1, NULL, SIZE_MAX, NULL, 0, NULL), NVX_ERR_ARG);
    EXPECT(k, 99);
    EXPECT(nvx_ddc_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_ddc_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_ddc_position(NULL, 0, &c, &p), NVX_ERR_ARG);
    EXPECT(nvx_ddc_position(fake, 0, &c, &p), NVX_ERR_ARG);
    EXPECT(c == 7 && p == 7, 1);
    EXPECT(nvx_ddc_plan(NULL, &L, &M, &T, &ni, &ns, &fmt), NVX_ERR_ARG);
    EXPECT(nvx_ddc_plan(fake, &L, &M, &T, &ni, &ns, &fmt), NVX_ERR_ARG);
    EXPECT(L == -1 && M == -1 && T == -1 && ni == -1 && ns == -1 && fmt == -1, 1);
    EXPECT(nvx_ddc_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_ddc_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_ddc_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_ddc_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_ddc_last_error(), "not a down-converter bank") != NULL, 1);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("ddc null-safety ok\n");
    return 0;
}
