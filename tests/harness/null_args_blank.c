/* The entry points of include/navtex_amd_blank.h called with NULL and nonsense arguments: error codes, never a crash, and
 * never a launch (every call here is refused before a device is looked for).  Linked against libnavtex_amd_blank.so alone,
 * needs no GPU (tests/test_blank.py runs it in a process of its own). */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_blank.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t few[64];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, ns = -1, fmt = -1;
    uint32_t thr = 7, hold = 7, fl = 7;
    uint64_t n = 7, c = 7, d = 7, g = 7;
    double ms = -1.0;
    void *in = (void *)(uintptr_t)0x100000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_blanker *b = (nvx_blanker *)(uintptr_t)0x300000, *fake = (nvx_blanker *)not_a_plan;
    nvx_blank_config cfg;

    nvx_blank_config_default(NULL);
    nvx_blank_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.format == NVX_BLANK_CS16 && cfg.n_streams == 1, 1);
    EXPECT(cfg.thr_q8 == 1024 && cfg.hold == 32 && cfg.floor == 64, 1);
    EXPECT(nvx_blank_create(NULL, &b), NVX_ERR_ARG);
    EXPECT(nvx_blank_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_blank_create(&cfg, &b), NVX_ERR_ARG);
    EXPECT(b == NULL, 1);
    nvx_blank_config_default(&cfg); cfg.n_streams = 0;
    EXPECT(nvx_blank_create(&cfg, &b), NVX_ERR_ARG);
    nvx_blank_config_default(&cfg); cfg.n_streams = 65536;
    EXPECT(nvx_blank_create(&cfg, &b), NVX_ERR_ARG);
    nvx_blank_config_default(&cfg); cfg.format = 4;
    EXPECT(nvx_blank_create(&cfg, &b), NVX_ERR_ARG);
    nvx_blank_config_default(&cfg); cfg.format = -1;
    EXPECT(nvx_blank_create(&cfg, &b), NVX_ERR_ARG);
    nvx_blank_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_blank_create(&cfg, &b), NVX_ERR_ARG);
    nvx_blank_config_default(&cfg); cfg.thr_q8 = 255;
    EXPECT(nvx_blank_create(&cfg, &b), NVX_ERR_ARG);
    nvx_blank_config_default(&cfg); cfg.thr_q8 = 1;
    EXPECT(nvx_blank_create(&cfg, &b), NVX_ERR_ARG);
    nvx_blank_config_default(&cfg); cfg.thr_q8 = 4097;
    EXPECT(nvx_blank_create(&cfg, &b), NVX_ERR_ARG);
    nvx_blank_config_default(&cfg); cfg.thr_q8 = 0xffffffffu;
    EXPECT(nvx_blank_create(&cfg, &b), NVX_ERR_ARG);
    nvx_blank_config_default(&cfg); cfg.hold = 1025;
    EXPECT(nvx_blank_create(&cfg, &b), NVX_ERR_ARG);
    nvx_blank_config_default(&cfg); cfg.hold = 0x80000000u;
    EXPECT(nvx_blank_create(&cfg, &b), NVX_ERR_ARG);
    nvx_blank_config_default(&cfg); cfg.floor = 65536;
    EXPECT(nvx_blank_create(&cfg, &b), NVX_ERR_ARG);
    EXPECT(nvx_blank_last_error() != NULL && nvx_blank_last_error()[0] != 0, 1);
    nvx_blank_destroy(NULL);
    nvx_blank_destroy(fake);

    EXPECT(nvx_blank_resident(NULL, in, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_blank_resident(fake, in, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_blank_resident(NULL, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_blank_push(NULL, 0, few, 16, few), NVX_ERR_ARG);
    EXPECT(nvx_blank_push(fake, 0, few, 16, few), NVX_ERR_ARG);
    EXPECT(nvx_blank_push(NULL, -1, NULL, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_blank_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_blank_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_blank_position(NULL, 0, &c), NVX_ERR_ARG);
    EXPECT(nvx_blank_position(fake, 0, &c), NVX_ERR_ARG);
    EXPECT(nvx_blank_stats(NULL, 0, &n, &d, &g, 1), NVX_ERR_ARG);
    EXPECT(nvx_blank_stats(fake, 0, &n, &d, &g, 0), NVX_ERR_ARG);
    EXPECT(c == 7 && n == 7 && d == 7 && g == 7, 1);
    EXPECT(nvx_blank_plan(NULL, &fmt, &ns, &thr, &hold, &fl), NVX_ERR_ARG);
    EXPECT(nvx_blank_plan(fake, &fmt, &ns, &thr, &hold, &fl), NVX_ERR_ARG);
    EXPECT(ns == -1 && fmt == -1 && thr == 7 && hold == 7 && fl == 7, 1);
    EXPECT(nvx_blank_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_blank_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_blank_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_blank_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_blank_last_error(), "not a blanker") != NULL, 1);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("blank null-safety ok\n");
    return 0;
}
