/* The entry points of include/navtex_amd_notch.h called with NULL and nonsense arguments: error codes, never a crash, and
 * never a launch (every call here is refused before a device is looked for).  Linked against libnavtex_amd_notch.so alone,
 * needs no GPU (tests/test_notch.py runs it in a process of its own). */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_notch.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t few[64];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, ns = -1, fmt = -1, wl = -1, nn = -1;
    uint64_t n = 7, pos = 7;
    uint32_t step = 7;
    double ms = -1.0;
    void *in = (void *)(uintptr_t)0x100000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_tone_notch *c = (nvx_tone_notch *)(uintptr_t)0x300000, *fake = (nvx_tone_notch *)not_a_plan;
    nvx_notch_config cfg;
    nvx_notch_status st;

    memset(&st, 0x55, sizeof st);
    nvx_notch_config_default(NULL);
    nvx_notch_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.format == NVX_NOTCH_CS16 && cfg.n_rows == 1 && cfg.n_notches == 1 && cfg.width_log2 == 5, 1);
    EXPECT(nvx_notch_create(NULL, &c), NVX_ERR_ARG);
    EXPECT(nvx_notch_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_notch_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(c == NULL, 1);
    nvx_notch_config_default(&cfg); cfg.n_rows = 0;
    EXPECT(nvx_notch_create(&cfg, &c), NVX_ERR_ARG);
    nvx_notch_config_default(&cfg); cfg.n_rows = 65536;
    EXPECT(nvx_notch_create(&cfg, &c), NVX_ERR_ARG);
    nvx_notch_config_default(&cfg); cfg.n_notches = 0;
    EXPECT(nvx_notch_create(&cfg, &c), NVX_ERR_ARG);
    nvx_notch_config_default(&cfg); cfg.n_notches = 5;
    EXPECT(nvx_notch_create(&cfg, &c), NVX_ERR_ARG);
    nvx_notch_config_default(&cfg); cfg.format = 4;
    EXPECT(nvx_notch_create(&cfg, &c), NVX_ERR_ARG);
    nvx_notch_config_default(&cfg); cfg.format = -1;
    EXPECT(nvx_notch_create(&cfg, &c), NVX_ERR_ARG);
    nvx_notch_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_notch_create(&cfg, &c), NVX_ERR_ARG);
    nvx_notch_config_default(&cfg); cfg.width_log2 = 1;
    EXPECT(nvx_notch_create(&cfg, &c), NVX_ERR_ARG);
    nvx_notch_config_default(&cfg); cfg.width_log2 = 7;
    EXPECT(nvx_notch_create(&cfg, &c), NVX_ERR_ARG);
    nvx_notch_config_default(&cfg); cfg.width_log2 = -2;
    EXPECT(nvx_notch_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(nvx_notch_last_error() != NULL && nvx_notch_last_error()[0] != 0, 1);
    nvx_notch_destroy(NULL);
    nvx_notch_destroy(fake);

    EXPECT(nvx_notch_resident(NULL, in, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_notch_resident(fake, in, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_notch_resident(NULL, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_notch_push(NULL, 0, few, 16, few), NVX_ERR_ARG);
    EXPECT(nvx_notch_push(fake, 0, few, 16, few), NVX_ERR_ARG);
    EXPECT(nvx_notch_push(NULL, -1, NULL, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_notch_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_notch_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_notch_set_freq(NULL, 0, 0, 12345u), NVX_ERR_ARG);
    EXPECT(nvx_notch_set_freq(fake, -1, 0, 12345u), NVX_ERR_ARG);
    EXPECT(nvx_notch_enable(NULL, 0, 0, 1), NVX_ERR_ARG);
    EXPECT(nvx_notch_enable(fake, 0, 0, 0), NVX_ERR_ARG);
    EXPECT(nvx_notch_measure(NULL, 0, 0), NVX_ERR_ARG);
    EXPECT(nvx_notch_measure(fake, 0, 0), NVX_ERR_ARG);
    EXPECT(nvx_notch_refine(NULL, 0, 0, &step), NVX_ERR_ARG);
    EXPECT(nvx_notch_refine(fake, 0, 0, NULL), NVX_ERR_ARG);
    EXPECT(step == 7, 1);
    EXPECT(nvx_notch_get(NULL, 0, 0, &st), NVX_ERR_ARG);
    EXPECT(nvx_notch_get(fake, 0, 0, &st), NVX_ERR_ARG);
    EXPECT(st.step == 0x55555555u && st.samples == 0x5555555555555555ull, 1);
    EXPECT(nvx_notch_position(NULL, 0, &pos), NVX_ERR_ARG);
    EXPECT(nvx_notch_position(fake, 0, &pos), NVX_ERR_ARG);
    EXPECT(pos == 7, 1);
    EXPECT(nvx_notch_plan(NULL, &fmt, &ns, &nn, &wl), NVX_ERR_ARG);
    EXPECT(nvx_notch_plan(fake, &fmt, &ns, &nn, &wl), NVX_ERR_ARG);
    EXPECT(ns == -1 && fmt == -1 && wl == -1 && nn == -1, 1);
    EXPECT(nvx_notch_delay(NULL), NVX_ERR_ARG);
    EXPECT(nvx_notch_delay(fake), NVX_ERR_ARG);
    EXPECT(nvx_notch_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_notch_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_notch_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_notch_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_notch_last_error(), "not a tone notch") != NULL, 1);
    /* the two helpers need no plan: 1000 Hz at 252 kS/s and back, a negative frequency, and nonsense */
    EXPECT(nvx_notch_step_from_hz(63000.0, 252000.0), 0x40000000u);
    EXPECT(nvx_notch_step_from_hz(-63000.0, 252000.0), 0xc0000000u);
    EXPECT(nvx_notch_step_from_hz(1000.0, 0.0), 0);
    EXPECT(nvx_notch_hz_from_step(0xc0000000u, 252000.0) == -63000.0, 1);
    EXPECT(nvx_notch_hz_from_step(nvx_notch_step_from_hz(1000.0, 252000.0), 252000.0) > 999.9999 &&
           nvx_notch_hz_from_step(nvx_notch_step_from_hz(1000.0, 252000.0), 252000.0) < 1000.0001, 1);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("notch null-safety ok\n");
    return 0;
}
