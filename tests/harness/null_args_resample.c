/* The entry points of include/navtex_amd_resample.h called with NULL and nonsense arguments: error codes, never a crash,
 * and never a launch (every call here is refused before a device is looked for).  Linked against
 * libnavtex_amd_resample.so alone, needs no GPU (tests/test_resample.py runs it in a process of its own). */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_resample.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t taps[NVX_RS_MAX_TAPS];
static int16_t few[64];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, L = -1, M = -1, T = -1, S = -1, ns = -1, fmt = -1;
    uint64_t n = 7, c = 7, p = 7;
    size_t k = 99;
    double ms = -1.0;
    void *in = (void *)(uintptr_t)0x100000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_resampler *r = (nvx_resampler *)(uintptr_t)0x300000, *fake = (nvx_resampler *)not_a_plan;
    nvx_resample_config cfg;

    nvx_resample_config_default(NULL);
    nvx_resample_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.n_streams == 1 && cfg.input_rate_hz == 2048000 && cfg.format == NVX_RS_CS16, 1);
    EXPECT(nvx_resample_create(NULL, &r), NVX_ERR_ARG);
    EXPECT(nvx_resample_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_resample_create(&cfg, &r), NVX_ERR_ARG);
    EXPECT(r == NULL, 1);
    nvx_resample_config_default(&cfg); cfg.n_streams = 0;
    EXPECT(nvx_resample_create(&cfg, &r), NVX_ERR_ARG);
    nvx_resample_config_default(&cfg); cfg.n_streams = 65536;
    EXPECT(nvx_resample_create(&cfg, &r), NVX_ERR_ARG);
    nvx_resample_config_default(&cfg); cfg.format = 4;
    EXPECT(nvx_resample_create(&cfg, &r), NVX_ERR_ARG);
    nvx_resample_config_default(&cfg); cfg.format = -1;
    EXPECT(nvx_resample_create(&cfg, &r), NVX_ERR_ARG);
    nvx_resample_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_resample_create(&cfg, &r), NVX_ERR_ARG);
    nvx_resample_config_default(&cfg); cfg.input_rate_hz = 95999;
    EXPECT(nvx_resample_create(&cfg, &r), NVX_ERR_ARG);
    nvx_resample_config_default(&cfg); cfg.input_rate_hz = 3200001;
    EXPECT(nvx_resample_create(&cfg, &r), NVX_ERR_ARG);
    nvx_resample_config_default(&cfg); cfg.input_rate_hz = 10000000;
    EXPECT(nvx_resample_create(&cfg, &r), NVX_ERR_ARG);
    nvx_resample_config_default(&cfg); cfg.input_rate_hz = 2048001;                      /* L = 252000 */
    EXPECT(nvx_resample_create(&cfg, &r), NVX_ERR_ARG);
    nvx_resample_config_default(&cfg); cfg.input_rate_hz = 1260252;                      /* L = 1000, T = 36 */
    EXPECT(nvx_resample_create(&cfg, &r), NVX_ERR_ARG);
    EXPECT(nvx_resample_last_error() != NULL && nvx_resample_last_error()[0] != 0, 1);
    nvx_resample_destroy(NULL);
    nvx_resample_destroy(fake);

    EXPECT(nvx_resample_design(0, &L, &M, &T, &S, taps, NVX_RS_MAX_TAPS), NVX_ERR_ARG);
    EXPECT(nvx_resample_design(4000000, &L, &M, &T, &S, taps, NVX_RS_MAX_TAPS), NVX_ERR_ARG);
    EXPECT(nvx_resample_design(2048000, &L, &M, &T, &S, taps, -1), NVX_ERR_ARG);
    EXPECT(L == -1 && M == -1 && T == -1 && S == -1, 1);
    EXPECT(nvx_resample_design(2048000, NULL, NULL, NULL, NULL, NULL, 0), 63 * 58);
    taps[0] = 12345;
    EXPECT(nvx_resample_design(2048000, &L, &M, &T, &S, taps, 63 * 58 - 1), 63 * 58);       /* too small: the need, no tap written */
    EXPECT(taps[0] == 12345 && L == 63 && M == 512 && T == 58 && S == 15, 1);
    EXPECT(nvx_resample_design(2048000, NULL, NULL, NULL, NULL, taps, 63 * 58), 63 * 58);
    EXPECT(taps[0] != 12345, 1);
    EXPECT(nvx_resample_out_count(0, 0, 100), -1);
    EXPECT(nvx_resample_out_count(2048000, UINT64_MAX, 2), -1);                          /* the position wraps */
    EXPECT(nvx_resample_out_count(2048000, (uint64_t)1 << 63, 0), -1);
    EXPECT(nvx_resample_out_count(2048000, 0, 655360), 80640);
    EXPECT(nvx_resample_out_count(2048000, ((uint64_t)1 << 62) + 5, 655360), 80640);

    EXPECT(nvx_resample_resident(NULL, in, 1024, 1024, out, 1024, 0, &k, NULL), NVX_ERR_ARG);
    EXPECT(nvx_resample_resident(fake, in, 1024, 1024, out, 1024, 0, &k, NULL), NVX_ERR_ARG);
    EXPECT(nvx_resample_resident(NULL, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, SIZE_MAX, NULL, NULL), NVX_ERR_ARG);
    EXPECT(nvx_resample_push(NULL, 0, few, 16, few, 16, &k), NVX_ERR_ARG);
    EXPECT(nvx_resample_push(fake, 0, few, 16, few, 16, &k), NVX_ERR_ARG);
    EXPECT(nvx_resample_push(NULL, -1, NULL, SIZE_MAX, NULL, 0, NULL), NVX_ERR_ARG);
    EXPECT(k, 99);
    EXPECT(nvx_resample_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_resample_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_resample_position(NULL, 0, &c, &p), NVX_ERR_ARG);
    EXPECT(nvx_resample_position(fake, 0, &c, &p), NVX_ERR_ARG);
    EXPECT(c == 7 && p == 7, 1);
    EXPECT(nvx_resample_plan(NULL, &L, &M, &T, &ns, &fmt), NVX_ERR_ARG);
    EXPECT(nvx_resample_plan(fake, &L, &M, &T, &ns, &fmt), NVX_ERR_ARG);
    EXPECT(ns == -1 && fmt == -1, 1);
    EXPECT(nvx_resample_set_form(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_resample_set_form(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_resample_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_resample_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_resample_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_resample_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_resample_last_error(), "not a resampler") != NULL, 1);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("resample null-safety ok\n");
    return 0;
}
