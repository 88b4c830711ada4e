/* The entry points of include/navtex_amd_align.h called with NULL and nonsense arguments: error codes, never a crash, and
 * never a launch (every call here is refused before a device is looked for).  Linked against libnavtex_amd_align.so alone,
 * needs no GPU (tests/test_align.py runs it in a process of its own). */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_align.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t few[64];
static int64_t table[128][2], power[2];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, ns = -1, fmt = -1, md = -1, mc = -1, dq = 99;
    uint64_t n = 7, pos = 7;
    double ms = -1.0;
    void *in = (void *)(uintptr_t)0x100000, *in2 = (void *)(uintptr_t)0x180000, *out = (void *)(uintptr_t)0x200000, *out2 = (void *)(uintptr_t)0x280000;
    nvx_row_aligner *c = (nvx_row_aligner *)(uintptr_t)0x300000, *fake = (nvx_row_aligner *)not_a_plan;
    nvx_align_config cfg;
    nvx_align_estimate est;
    int16_t taps[NVX_ALIGN_PHASES * NVX_ALIGN_TAPS];

    nvx_align_config_default(NULL);
    nvx_align_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.format == NVX_ALIGN_CS16 && cfg.n_pairs == 1 && cfg.max_delay == 4096 && cfg.min_contrast == 64, 1);
    EXPECT(nvx_align_create(NULL, &c), NVX_ERR_ARG);
    EXPECT(nvx_align_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_align_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(c == NULL, 1);
    nvx_align_config_default(&cfg); cfg.n_pairs = 0;
    EXPECT(nvx_align_create(&cfg, &c), NVX_ERR_ARG);
    nvx_align_config_default(&cfg); cfg.n_pairs = 65536;
    EXPECT(nvx_align_create(&cfg, &c), NVX_ERR_ARG);
    nvx_align_config_default(&cfg); cfg.format = 4;
    EXPECT(nvx_align_create(&cfg, &c), NVX_ERR_ARG);
    nvx_align_config_default(&cfg); cfg.format = -1;
    EXPECT(nvx_align_create(&cfg, &c), NVX_ERR_ARG);
    nvx_align_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_align_create(&cfg, &c), NVX_ERR_ARG);
    nvx_align_config_default(&cfg); cfg.max_delay = 0;
    EXPECT(nvx_align_create(&cfg, &c), NVX_ERR_ARG);
    nvx_align_config_default(&cfg); cfg.max_delay = NVX_ALIGN_MAX_DELAY_LIMIT + 1;
    EXPECT(nvx_align_create(&cfg, &c), NVX_ERR_ARG);
    nvx_align_config_default(&cfg); cfg.min_contrast = 0;
    EXPECT(nvx_align_create(&cfg, &c), NVX_ERR_ARG);
    nvx_align_config_default(&cfg); cfg.min_contrast = (1 << 20) + 1;
    EXPECT(nvx_align_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(nvx_align_last_error() != NULL && nvx_align_last_error()[0] != 0, 1);
    nvx_align_destroy(NULL);
    nvx_align_destroy(fake);

    EXPECT(nvx_align_resident(NULL, in, 1024, in2, 1024, 1024, out, 1024, out2, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_align_resident(fake, in, 1024, in2, 1024, 1024, out, 1024, out2, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_align_resident(NULL, NULL, 0, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, NULL, SIZE_MAX, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_align_push(NULL, 0, few, few, 16, few, few), NVX_ERR_ARG);
    EXPECT(nvx_align_push(fake, 0, few, few, 16, few, few), NVX_ERR_ARG);
    EXPECT(nvx_align_push(NULL, -1, NULL, NULL, SIZE_MAX, NULL, NULL), NVX_ERR_ARG);
    EXPECT(nvx_align_measure_resident(NULL, 0, in, 4096, in2, 4096, 4096, 0, 64, &table[0][0], power, NULL), NVX_ERR_ARG);
    EXPECT(nvx_align_measure_resident(fake, 0, in, 4096, in2, 4096, 4096, 0, 64, &table[0][0], power, NULL), NVX_ERR_ARG);
    EXPECT(nvx_align_measure_resident(NULL, 9, NULL, 0, NULL, 0, SIZE_MAX, -1, -1, NULL, NULL, NULL), NVX_ERR_ARG);
    EXPECT(nvx_align_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_align_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_align_set_delay(NULL, 0, 32), NVX_ERR_ARG);
    EXPECT(nvx_align_set_delay(fake, -1, 32), NVX_ERR_ARG);
    EXPECT(nvx_align_get_delay(NULL, 0, &dq), NVX_ERR_ARG);
    EXPECT(nvx_align_get_delay(fake, 0, &dq), NVX_ERR_ARG);
    EXPECT(dq == 99, 1);
    EXPECT(nvx_align_position(NULL, 0, &pos), NVX_ERR_ARG);
    EXPECT(nvx_align_position(fake, 0, &pos), NVX_ERR_ARG);
    EXPECT(pos == 7, 1);
    EXPECT(nvx_align_plan(NULL, &fmt, &ns, &md, &mc), NVX_ERR_ARG);
    EXPECT(nvx_align_plan(fake, &fmt, &ns, &md, &mc), NVX_ERR_ARG);
    EXPECT(ns == -1 && fmt == -1 && md == -1 && mc == -1, 1);
    EXPECT(nvx_align_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_align_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_align_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_align_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_align_last_error(), "not a row aligner") != NULL, 1);

    /* the parts that need no device */
    EXPECT(nvx_align_delay(), NVX_ALIGN_GROUP_DELAY);
    EXPECT(nvx_align_taps(NULL), NVX_ERR_ARG);
    EXPECT(nvx_align_taps(taps), NVX_OK);
    EXPECT(taps[NVX_ALIGN_GROUP_DELAY] == 16384 && taps[0] == 0, 1);
    EXPECT(nvx_align_window(1023, 0, 64), 0);
    EXPECT(nvx_align_window(1024 + 63, 0, 64), 1024);
    EXPECT(nvx_align_window(SIZE_MAX, 0, 64), 0);
    EXPECT(nvx_align_window(5000, 0, 65), 0);
    memset(&est, 0x55, sizeof est);
    EXPECT(nvx_align_find(NULL, 0, 64, 4096, 1 << 20, 1 << 20, 64, &est), NVX_ERR_ARG);
    EXPECT(nvx_align_find(&table[0][0], 0, 64, 4096, 1 << 20, 1 << 20, 64, NULL), NVX_ERR_ARG);
    EXPECT(nvx_align_find(&table[0][0], 0, 63, 4096, 1 << 20, 1 << 20, 64, &est), NVX_ERR_ARG);
    EXPECT(nvx_align_find(&table[0][0], 0, 16384, 4096, 1 << 20, 1 << 20, 64, &est), NVX_ERR_ARG);
    EXPECT(nvx_align_find(&table[0][0], 0, 64, 0, 1 << 20, 1 << 20, 64, &est), NVX_ERR_ARG);
    EXPECT(nvx_align_find(&table[0][0], 0, 64, 4096, -1, 1 << 20, 64, &est), NVX_ERR_ARG);
    EXPECT(nvx_align_find(&table[0][0], 0, 64, 4096, 1 << 20, 1 << 20, 0, &est), NVX_ERR_ARG);
    EXPECT(nvx_align_find(&table[0][0], 1 << 21, 64, 4096, 1 << 20, 1 << 20, 64, &est), NVX_ERR_ARG);
    EXPECT(est.reason == 0x55555555, 1);
    table[5][1] = INT64_MIN;
    EXPECT(nvx_align_find(&table[0][0], 0, 128, 4096, 1 << 20, 1 << 20, 64, &est), NVX_ERR_ARG);
    table[5][1] = 0;
    EXPECT(nvx_align_find(&table[0][0], 0, 128, 4096, 0, 0, 64, &est), NVX_OK);
    EXPECT(est.reason == 1 && est.delay_q5 == 0, 1);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("align null-safety ok\n");
    return 0;
}
