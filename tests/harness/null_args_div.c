/* The entry points of include/navtex_amd_div.h called with NULL and nonsense arguments: error codes, never a crash, and
 * never a launch (every call here is refused before a device is looked for).  Linked against libnavtex_amd_div.so alone,
 * needs no GPU (tests/test_div.py runs it in a process of its own). */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_div.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t few[64];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, ns = -1, nt = -1, fmt = -1, wl = -1;
    uint64_t n = 7, pos = 7;
    double ms = -1.0;
    void *in = (void *)(uintptr_t)0x100000, *in2 = (void *)(uintptr_t)0x180000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_diversity_combiner *c = (nvx_diversity_combiner *)(uintptr_t)0x300000, *fake = (nvx_diversity_combiner *)not_a_plan;
    nvx_div_config cfg;
    nvx_div_status st;

    memset(&st, 0x55, sizeof st);
    nvx_div_config_default(NULL);
    nvx_div_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.format == NVX_DIV_CS16 && cfg.n_pairs == 1 && cfg.n_targets == 1 && cfg.window_log2 == 2, 1);
    EXPECT(nvx_div_create(NULL, &c), NVX_ERR_ARG);
    EXPECT(nvx_div_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_div_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(c == NULL, 1);
    nvx_div_config_default(&cfg); cfg.n_pairs = 0;
    EXPECT(nvx_div_create(&cfg, &c), NVX_ERR_ARG);
    nvx_div_config_default(&cfg); cfg.n_pairs = 65536;
    EXPECT(nvx_div_create(&cfg, &c), NVX_ERR_ARG);
    nvx_div_config_default(&cfg); cfg.n_targets = 0;
    EXPECT(nvx_div_create(&cfg, &c), NVX_ERR_ARG);
    nvx_div_config_default(&cfg); cfg.n_targets = NVX_DIV_MAX_TARGETS + 1;
    EXPECT(nvx_div_create(&cfg, &c), NVX_ERR_ARG);
    nvx_div_config_default(&cfg); cfg.format = 4;
    EXPECT(nvx_div_create(&cfg, &c), NVX_ERR_ARG);
    nvx_div_config_default(&cfg); cfg.format = -1;
    EXPECT(nvx_div_create(&cfg, &c), NVX_ERR_ARG);
    nvx_div_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_div_create(&cfg, &c), NVX_ERR_ARG);
    nvx_div_config_default(&cfg); cfg.window_log2 = 3;
    EXPECT(nvx_div_create(&cfg, &c), NVX_ERR_ARG);
    nvx_div_config_default(&cfg); cfg.window_log2 = 5;
    EXPECT(nvx_div_create(&cfg, &c), NVX_ERR_ARG);
    nvx_div_config_default(&cfg); cfg.window_log2 = 6;
    EXPECT(nvx_div_create(&cfg, &c), NVX_ERR_ARG);
    nvx_div_config_default(&cfg); cfg.window_log2 = -1;
    EXPECT(nvx_div_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(nvx_div_last_error() != NULL && nvx_div_last_error()[0] != 0, 1);
    nvx_div_destroy(NULL);
    nvx_div_destroy(fake);

    EXPECT(nvx_div_resident(NULL, in, 1024, in2, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_div_resident(fake, in, 1024, in2, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_div_resident(NULL, NULL, 0, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_div_push(NULL, 0, few, few, 16, few), NVX_ERR_ARG);
    EXPECT(nvx_div_push(fake, 0, few, few, 16, few), NVX_ERR_ARG);
    EXPECT(nvx_div_push(NULL, -1, NULL, NULL, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_div_set_freq(NULL, 0, 0, 12345u), NVX_ERR_ARG);
    EXPECT(nvx_div_set_freq(fake, -1, 0, 12345u), NVX_ERR_ARG);
    EXPECT(nvx_div_set(NULL, 0, 0, 0, 8192, 0), NVX_ERR_ARG);
    EXPECT(nvx_div_set(fake, 0, 0, 1, 8192, 0), NVX_ERR_ARG);
    EXPECT(nvx_div_set_mode(NULL, 0, 0, NVX_DIV_HOLD), NVX_ERR_ARG);
    EXPECT(nvx_div_set_mode(fake, -1, 0, NVX_DIV_TRACK), NVX_ERR_ARG);
    EXPECT(nvx_div_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_div_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_div_get(NULL, 0, 0, &st), NVX_ERR_ARG);
    EXPECT(nvx_div_get(fake, 0, 0, &st), NVX_ERR_ARG);
    EXPECT(st.w_im == 0x55555555 && st.samples == 0x5555555555555555ull, 1);
    EXPECT(nvx_div_position(NULL, 0, &pos), NVX_ERR_ARG);
    EXPECT(nvx_div_position(fake, 0, &pos), NVX_ERR_ARG);
    EXPECT(pos == 7, 1);
    EXPECT(nvx_div_plan(NULL, &fmt, &ns, &nt, &wl), NVX_ERR_ARG);
    EXPECT(nvx_div_plan(fake, &fmt, &ns, &nt, &wl), NVX_ERR_ARG);
    EXPECT(ns == -1 && nt == -1 && fmt == -1 && wl == -1, 1);
    EXPECT(nvx_div_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_div_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_div_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_div_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_div_last_error(), "not a diversity combiner") != NULL, 1);
    /* the two formulas need no plan: -14 kHz at 252 kS/s is -1/18 of a turn */
    EXPECT(nvx_div_step_from_hz(-14000.0, 252000.0), 4056358002u);
    EXPECT(nvx_div_step_from_hz(0.0, 252000.0) == 0 && nvx_div_step_from_hz(1.0, 0.0) == 0 && nvx_div_step_from_hz(1.0, -5.0) == 0, 1);
    EXPECT(nvx_div_hz_from_step(4056358002u, 252000.0) < -13999.9 && nvx_div_hz_from_step(4056358002u, 252000.0) > -14000.1, 1);
    EXPECT(nvx_div_hz_from_step(0x40000000u, 252000.0) == 63000.0, 1);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("div null-safety ok\n");
    return 0;
}
