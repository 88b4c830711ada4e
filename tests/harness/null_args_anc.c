/* The entry points of include/navtex_amd_anc.h called with NULL and nonsense arguments: error codes, never a crash, and
 * never a launch (every call here is refused before a device is looked for).  Linked against libnavtex_amd_anc.so alone,
 * needs no GPU (tests/test_anc.py runs it in a process of its own). */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_anc.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t few[64];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, ns = -1, fmt = -1, wl = -1;
    uint64_t n = 7, pos = 7;
    double ms = -1.0;
    void *in = (void *)(uintptr_t)0x100000, *in2 = (void *)(uintptr_t)0x180000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_noise_canceller *c = (nvx_noise_canceller *)(uintptr_t)0x300000, *fake = (nvx_noise_canceller *)not_a_plan;
    nvx_anc_config cfg;
    nvx_anc_status st;

    memset(&st, 0x55, sizeof st);
    nvx_anc_config_default(NULL);
    nvx_anc_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.format == NVX_ANC_CS16 && cfg.n_pairs == 1 && cfg.window_log2 == 2, 1);
    EXPECT(nvx_anc_create(NULL, &c), NVX_ERR_ARG);
    EXPECT(nvx_anc_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_anc_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(c == NULL, 1);
    nvx_anc_config_default(&cfg); cfg.n_pairs = 0;
    EXPECT(nvx_anc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_anc_config_default(&cfg); cfg.n_pairs = 65536;
    EXPECT(nvx_anc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_anc_config_default(&cfg); cfg.format = 4;
    EXPECT(nvx_anc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_anc_config_default(&cfg); cfg.format = -1;
    EXPECT(nvx_anc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_anc_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_anc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_anc_config_default(&cfg); cfg.window_log2 = 0;
    EXPECT(nvx_anc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_anc_config_default(&cfg); cfg.window_log2 = 3;
    EXPECT(nvx_anc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_anc_config_default(&cfg); cfg.window_log2 = 8;
    EXPECT(nvx_anc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_anc_config_default(&cfg); cfg.window_log2 = -2;
    EXPECT(nvx_anc_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(nvx_anc_last_error() != NULL && nvx_anc_last_error()[0] != 0, 1);
    nvx_anc_destroy(NULL);
    nvx_anc_destroy(fake);

    EXPECT(nvx_anc_resident(NULL, in, 1024, in2, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_anc_resident(fake, in, 1024, in2, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_anc_resident(NULL, NULL, 0, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_anc_push(NULL, 0, few, few, 16, few), NVX_ERR_ARG);
    EXPECT(nvx_anc_push(fake, 0, few, few, 16, few), NVX_ERR_ARG);
    EXPECT(nvx_anc_push(NULL, -1, NULL, NULL, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_anc_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_anc_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_anc_set(NULL, 0, 8192, 0), NVX_ERR_ARG);
    EXPECT(nvx_anc_set(fake, 0, 8192, 0), NVX_ERR_ARG);
    EXPECT(nvx_anc_set_mode(NULL, 0, NVX_ANC_HOLD), NVX_ERR_ARG);
    EXPECT(nvx_anc_set_mode(fake, -1, NVX_ANC_TRACK), NVX_ERR_ARG);
    EXPECT(nvx_anc_get(NULL, 0, &st), NVX_ERR_ARG);
    EXPECT(nvx_anc_get(fake, 0, &st), NVX_ERR_ARG);
    EXPECT(st.c_im == 0x55555555 && st.samples == 0x5555555555555555ull, 1);
    EXPECT(nvx_anc_position(NULL, 0, &pos), NVX_ERR_ARG);
    EXPECT(nvx_anc_position(fake, 0, &pos), NVX_ERR_ARG);
    EXPECT(pos == 7, 1);
    EXPECT(nvx_anc_plan(NULL, &fmt, &ns, &wl), NVX_ERR_ARG);
    EXPECT(nvx_anc_plan(fake, &fmt, &ns, &wl), NVX_ERR_ARG);
    EXPECT(ns == -1 && fmt == -1 && wl == -1, 1);
    EXPECT(nvx_anc_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_anc_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_anc_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_anc_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_anc_last_error(), "not a noise canceller") != NULL, 1);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("anc null-safety ok\n");
    return 0;
}
