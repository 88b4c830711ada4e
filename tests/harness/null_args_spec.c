/* The entry points of include/navtex_amd_spec.h called with NULL and nonsense arguments: error codes, never a crash, and
 * never a launch (every call here is refused before a device is looked for).  Linked against libnavtex_amd_spec.so alone,
 * needs no GPU (tests/test_spec.py runs it in a process of its own). */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_spec.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t few[64];
static uint16_t levels[64];
static double row[256], lag[256];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, ns = -1, fmt = -1, nl = -1, av = -1, i;
    uint64_t n = 7, pos = 7;
    double ms = -1.0;
    void *in = (void *)(uintptr_t)0x100000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_spectrum *c = (nvx_spectrum *)(uintptr_t)0x300000, *fake = (nvx_spectrum *)not_a_plan;
    nvx_spec_config cfg;
    nvx_spec_params par;
    nvx_spec_hit hit[2];

    nvx_spec_config_default(NULL);
    nvx_spec_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.format == NVX_SPEC_CS16 && cfg.n_rows == 1 && cfg.n_log2 == 11 && cfg.avg == 8, 1);
    EXPECT(nvx_spec_create(NULL, &c), NVX_ERR_ARG);
    EXPECT(nvx_spec_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_spec_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(c == NULL, 1);
    nvx_spec_config_default(&cfg); cfg.n_rows = 0;
    EXPECT(nvx_spec_create(&cfg, &c), NVX_ERR_ARG);
    nvx_spec_config_default(&cfg); cfg.n_rows = 65536;
    EXPECT(nvx_spec_create(&cfg, &c), NVX_ERR_ARG);
    nvx_spec_config_default(&cfg); cfg.n_log2 = 7;
    EXPECT(nvx_spec_create(&cfg, &c), NVX_ERR_ARG);
    nvx_spec_config_default(&cfg); cfg.n_log2 = 13;
    EXPECT(nvx_spec_create(&cfg, &c), NVX_ERR_ARG);
    nvx_spec_config_default(&cfg); cfg.avg = 0;
    EXPECT(nvx_spec_create(&cfg, &c), NVX_ERR_ARG);
    nvx_spec_config_default(&cfg); cfg.avg = 65;                  /* 65 * 1024 > 65536 */
    EXPECT(nvx_spec_create(&cfg, &c), NVX_ERR_ARG);
    nvx_spec_config_default(&cfg); cfg.n_log2 = 8; cfg.avg = 513;
    EXPECT(nvx_spec_create(&cfg, &c), NVX_ERR_ARG);
    nvx_spec_config_default(&cfg); cfg.avg = 0x7fffffff;
    EXPECT(nvx_spec_create(&cfg, &c), NVX_ERR_ARG);
    nvx_spec_config_default(&cfg); cfg.format = 4;
    EXPECT(nvx_spec_create(&cfg, &c), NVX_ERR_ARG);
    nvx_spec_config_default(&cfg); cfg.format = -1;
    EXPECT(nvx_spec_create(&cfg, &c), NVX_ERR_ARG);
    nvx_spec_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_spec_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(nvx_spec_last_error() != NULL && nvx_spec_last_error()[0] != 0, 1);
    nvx_spec_destroy(NULL);
    nvx_spec_destroy(fake);

    EXPECT(nvx_spec_lines_for(NULL, 0, 1024), NVX_ERR_ARG);
    EXPECT(nvx_spec_lines_for(fake, 0, 1024), NVX_ERR_ARG);
    EXPECT(nvx_spec_resident(NULL, in, 1024, 1024, out, 4, NULL), NVX_ERR_ARG);
    EXPECT(nvx_spec_resident(fake, in, 1024, 1024, out, 4, NULL), NVX_ERR_ARG);
    EXPECT(nvx_spec_resident(NULL, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_spec_push(NULL, 0, few, 16, levels, 1), NVX_ERR_ARG);
    EXPECT(nvx_spec_push(fake, 0, few, 16, levels, 1), NVX_ERR_ARG);
    EXPECT(nvx_spec_push(NULL, -1, NULL, SIZE_MAX, NULL, SIZE_MAX), NVX_ERR_ARG);
    EXPECT(nvx_spec_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_spec_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_spec_measure(NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_spec_measure(fake, -1), NVX_ERR_ARG);
    row[3] = 5.0;
    EXPECT(nvx_spec_get(NULL, 0, row, lag, lag, &n), NVX_ERR_ARG);
    EXPECT(nvx_spec_get(fake, 0, row, NULL, NULL, NULL), NVX_ERR_ARG);
    EXPECT(row[3] == 5.0 && n == 7, 1);
    EXPECT(nvx_spec_position(NULL, 0, &pos), NVX_ERR_ARG);
    EXPECT(nvx_spec_position(fake, 0, &pos), NVX_ERR_ARG);
    EXPECT(pos == 7, 1);
    EXPECT(nvx_spec_plan(NULL, &fmt, &ns, &nl, &av), NVX_ERR_ARG);
    EXPECT(nvx_spec_plan(fake, &fmt, &ns, &nl, &av), NVX_ERR_ARG);
    EXPECT(ns == -1 && fmt == -1 && nl == -1 && av == -1, 1);
    EXPECT(nvx_spec_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_spec_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_spec_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_spec_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_spec_last_error(), "not a spectrum monitor") != NULL, 1);

    /* the finder needs no plan and no device */
    nvx_spec_params_default(NULL);
    nvx_spec_params_default(&par);
    EXPECT(par.struct_size == sizeof par && par.guard_bins == 3 && par.min_lines == 8 && par.min_coherence == 0.95 && par.min_score_db == 6.0, 1);
    for (i = 0; i < 256; i++) { row[i] = 1.0; lag[i] = 0.0; }
    EXPECT(nvx_spec_find_lines(NULL, lag, lag, 8, 8, 100, NULL, hit, 2), NVX_ERR_ARG);
    EXPECT(nvx_spec_find_lines(row, NULL, lag, 8, 8, 100, NULL, hit, 2), NVX_ERR_ARG);
    EXPECT(nvx_spec_find_lines(row, lag, NULL, 8, 8, 100, NULL, hit, 2), NVX_ERR_ARG);
    EXPECT(nvx_spec_find_lines(row, lag, lag, 7, 8, 100, NULL, hit, 2), NVX_ERR_ARG);
    EXPECT(nvx_spec_find_lines(row, lag, lag, 13, 8, 100, NULL, hit, 2), NVX_ERR_ARG);
    EXPECT(nvx_spec_find_lines(row, lag, lag, 8, 1, 100, NULL, hit, 2), NVX_ERR_ARG);          /* A < 2: no lag products */
    EXPECT(nvx_spec_find_lines(row, lag, lag, 8, 8, 7, NULL, hit, 2), NVX_ERR_ARG);            /* fewer than min_lines */
    EXPECT(nvx_spec_find_lines(row, lag, lag, 8, 8, 100, NULL, NULL, 2), NVX_ERR_ARG);
    EXPECT(nvx_spec_find_lines(row, lag, lag, 8, 8, 100, NULL, hit, -1), NVX_ERR_ARG);
    par.struct_size = 4;
    EXPECT(nvx_spec_find_lines(row, lag, lag, 8, 8, 100, &par, hit, 2), NVX_ERR_ARG);
    EXPECT(nvx_spec_find_lines(row, lag, lag, 8, 8, 100, NULL, hit, 2), 0);                    /* a flat row: nothing */
    EXPECT(nvx_spec_find_lines(row, lag, lag, 8, 8, 100, NULL, NULL, 0), 0);
    /* one steady line a quarter of a bin above bin 10 (index 138): SC = SP (7/8) e^(j pi (10 + 1/4)) */
    row[138] = 1000.0; lag[138] = 875.0 * 0.70710678118654752;
    EXPECT(nvx_spec_find_lines(row, lag, lag, 8, 8, 100, NULL, hit, 2), 1);
    EXPECT(hit[0].bin == 138 && hit[0].cycles_per_sample > 10.2499 / 256 && hit[0].cycles_per_sample < 10.2501 / 256, 1);
    EXPECT(hit[0].step == 171966464u && hit[0].coherence > 0.9999 && hit[0].coherence < 1.0001 && hit[0].score_db > 29.99 && hit[0].score_db < 30.01, 1);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("spec null-safety ok\n");
    return 0;
}
