/* The entry points of include/navtex_amd_iqc.h called with NULL and nonsense arguments: error codes, never a crash, and
 * never a launch (every call here is refused before a device is looked for).  Linked against libnavtex_amd_iqc.so alone,
 * needs no GPU (tests/test_iqc.py runs it in a process of its own). */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_iqc.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t few[64];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, ns = -1, fmt = -1, wl = -1;
    uint64_t n = 7, pos = 7;
    double ms = -1.0;
    void *in = (void *)(uintptr_t)0x100000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_iq_corrector *c = (nvx_iq_corrector *)(uintptr_t)0x300000, *fake = (nvx_iq_corrector *)not_a_plan;
    nvx_iqc_config cfg;
    nvx_iqc_status st;

    memset(&st, 0x55, sizeof st);
    nvx_iqc_config_default(NULL);
    nvx_iqc_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.format == NVX_IQC_CS16 && cfg.n_streams == 1 && cfg.window_log2 == 4, 1);
    EXPECT(nvx_iqc_create(NULL, &c), NVX_ERR_ARG);
    EXPECT(nvx_iqc_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_iqc_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(c == NULL, 1);
    nvx_iqc_config_default(&cfg); cfg.n_streams = 0;
    EXPECT(nvx_iqc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_iqc_config_default(&cfg); cfg.n_streams = 65536;
    EXPECT(nvx_iqc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_iqc_config_default(&cfg); cfg.format = 4;
    EXPECT(nvx_iqc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_iqc_config_default(&cfg); cfg.format = -1;
    EXPECT(nvx_iqc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_iqc_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_iqc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_iqc_config_default(&cfg); cfg.window_log2 = 0;
    EXPECT(nvx_iqc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_iqc_config_default(&cfg); cfg.window_log2 = 3;
    EXPECT(nvx_iqc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_iqc_config_default(&cfg); cfg.window_log2 = 8;
    EXPECT(nvx_iqc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_iqc_config_default(&cfg); cfg.window_log2 = -2;
    EXPECT(nvx_iqc_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(nvx_iqc_last_error() != NULL && nvx_iqc_last_error()[0] != 0, 1);
    nvx_iqc_destroy(NULL);
    nvx_iqc_destroy(fake);

    EXPECT(nvx_iqc_resident(NULL, in, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_iqc_resident(fake, in, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_iqc_resident(NULL, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_iqc_push(NULL, 0, few, 16, few), NVX_ERR_ARG);
    EXPECT(nvx_iqc_push(fake, 0, few, 16, few), NVX_ERR_ARG);
    EXPECT(nvx_iqc_push(NULL, -1, NULL, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_iqc_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_iqc_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_iqc_set(NULL, 0, 0, 0, 0, 16384), NVX_ERR_ARG);
    EXPECT(nvx_iqc_set(fake, 0, 0, 0, 0, 16384), NVX_ERR_ARG);
    EXPECT(nvx_iqc_set_mode(NULL, 0, NVX_IQC_HOLD), NVX_ERR_ARG);
    EXPECT(nvx_iqc_set_mode(fake, -1, NVX_IQC_TRACK), NVX_ERR_ARG);
    EXPECT(nvx_iqc_get(NULL, 0, &st), NVX_ERR_ARG);
    EXPECT(nvx_iqc_get(fake, 0, &st), NVX_ERR_ARG);
    EXPECT(st.c_q == 0x55555555 && st.samples == 0x5555555555555555ull, 1);
    EXPECT(nvx_iqc_position(NULL, 0, &pos), NVX_ERR_ARG);
    EXPECT(nvx_iqc_position(fake, 0, &pos), NVX_ERR_ARG);
    EXPECT(pos == 7, 1);
    EXPECT(nvx_iqc_plan(NULL, &fmt, &ns, &wl), NVX_ERR_ARG);
    EXPECT(nvx_iqc_plan(fake, &fmt, &ns, &wl), NVX_ERR_ARG);
    EXPECT(ns == -1 && fmt == -1 && wl == -1, 1);
    EXPECT(nvx_iqc_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_iqc_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_iqc_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_iqc_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_iqc_last_error(), "not an IQ corrector") != NULL, 1);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("iqc null-safety ok\n");
    return 0;
}
