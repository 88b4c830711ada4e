/* The entry points of include/navtex_amd_wanc.h called with NULL and nonsense arguments: error codes, never a crash, and
 * never a launch (every call here is refused before a device is looked for).  Linked against libnavtex_amd_wanc.so alone,
 * needs no GPU (tests/test_wanc.py runs it in a process of its own). */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_wanc.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t few[64];
static int32_t weights[NVX_WANC_TAPS_MAX];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, ns = -1, fmt = -1, wl = -1, taps = -1, ll = -1;
    uint64_t n = 7, pos = 7;
    double ms = -1.0;
    void *in = (void *)(uintptr_t)0x100000, *in2 = (void *)(uintptr_t)0x180000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_wide_canceller *c = (nvx_wide_canceller *)(uintptr_t)0x300000, *fake = (nvx_wide_canceller *)not_a_plan;
    nvx_wanc_config cfg;
    nvx_wanc_status st;

    memset(&st, 0x55, sizeof st);
    nvx_wanc_config_default(NULL);
    nvx_wanc_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.format == NVX_WANC_CS16 && cfg.n_pairs == 1 && cfg.window_log2 == 2, 1);
    EXPECT(cfg.n_taps == 8 && cfg.load_log2 == 12, 1);
    EXPECT(nvx_wanc_create(NULL, &c), NVX_ERR_ARG);
    EXPECT(nvx_wanc_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(c == NULL, 1);
    nvx_wanc_config_default(&cfg); cfg.n_pairs = 0;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_wanc_config_default(&cfg); cfg.n_pairs = 65536;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_wanc_config_default(&cfg); cfg.format = 4;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_wanc_config_default(&cfg); cfg.format = -1;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_wanc_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_wanc_config_default(&cfg); cfg.window_log2 = 0;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_wanc_config_default(&cfg); cfg.window_log2 = 3;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_wanc_config_default(&cfg); cfg.window_log2 = 8;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_wanc_config_default(&cfg); cfg.n_taps = 0;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_wanc_config_default(&cfg); cfg.n_taps = 12;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_wanc_config_default(&cfg); cfg.n_taps = 32;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_wanc_config_default(&cfg); cfg.load_log2 = 7;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    nvx_wanc_config_default(&cfg); cfg.load_log2 = 21;
    EXPECT(nvx_wanc_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(nvx_wanc_last_error() != NULL && nvx_wanc_last_error()[0] != 0, 1);
    nvx_wanc_destroy(NULL);
    nvx_wanc_destroy(fake);

    EXPECT(nvx_wanc_resident(NULL, in, 1024, in2, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_wanc_resident(fake, in, 1024, in2, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_wanc_resident(NULL, NULL, 0, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_wanc_push(NULL, 0, few, few, 16, few), NVX_ERR_ARG);
    EXPECT(nvx_wanc_push(fake, 0, few, few, 16, few), NVX_ERR_ARG);
    EXPECT(nvx_wanc_push(NULL, -1, NULL, NULL, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_wanc_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_wanc_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_wanc_set(NULL, 0, weights, weights), NVX_ERR_ARG);
    EXPECT(nvx_wanc_set(fake, 0, weights, weights), NVX_ERR_ARG);
    EXPECT(nvx_wanc_set(NULL, 0, NULL, NULL), NVX_ERR_ARG);
    EXPECT(nvx_wanc_set_mode(NULL, 0, NVX_WANC_HOLD), NVX_ERR_ARG);
    EXPECT(nvx_wanc_set_mode(fake, -1, NVX_WANC_TRACK), NVX_ERR_ARG);
    EXPECT(nvx_wanc_get(NULL, 0, &st), NVX_ERR_ARG);
    EXPECT(nvx_wanc_get(fake, 0, &st), NVX_ERR_ARG);
    EXPECT(st.w_im[3] == 0x55555555 && st.samples == 0x5555555555555555ull, 1);
    EXPECT(nvx_wanc_position(NULL, 0, &pos), NVX_ERR_ARG);
    EXPECT(nvx_wanc_position(fake, 0, &pos), NVX_ERR_ARG);
    EXPECT(pos == 7, 1);
    EXPECT(nvx_wanc_plan(NULL, &fmt, &ns, &wl, &taps, &ll), NVX_ERR_ARG);
    EXPECT(nvx_wanc_plan(fake, &fmt, &ns, &wl, &taps, &ll), NVX_ERR_ARG);
    EXPECT(ns == -1 && fmt == -1 && wl == -1 && taps == -1 && ll == -1, 1);
    EXPECT(nvx_wanc_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_wanc_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_wanc_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_wanc_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_wanc_last_error(), "not a multi-tap canceller") != NULL, 1);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("wanc null-safety ok\n");
    return 0;
}
