/* The entry points of include/navtex_amd_tap.h called with NULL and nonsense arguments: error codes, never a crash, and never a
 * launch (every call here is refused before a device is looked for).  Linked against libnavtex_amd_tap.so alone, needs no GPU
 * (tests/test_tap.py runs it in a process of its own). */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_tap.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t few[64];
static int32_t taps[32768];
static int16_t table[2 * 4096];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, ni = -1, nt = -1, kind = -1, L = -1, M = -1, T = -1, k = -7;
    uint64_t n = 7, pos = 7, made = 7;
    size_t n_out = 7;
    double ms = -1.0, hz = -1.0;
    void *in = (void *)(uintptr_t)0x100000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_tap *c = (nvx_tap *)(uintptr_t)0x300000, *fake = (nvx_tap *)not_a_plan;
    nvx_tap_config cfg;

    nvx_tap_config_default(NULL);
    nvx_tap_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.n_inputs == 1 && cfg.n_taps == 1 && cfg.output_rate_hz == 12000, 1);
    EXPECT(cfg.kind == NVX_TAP_IQ, 1);
    EXPECT(nvx_tap_create(NULL, &c), NVX_ERR_ARG);
    EXPECT(nvx_tap_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(c == NULL, 1);
    nvx_tap_config_default(&cfg); cfg.n_inputs = 0;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    nvx_tap_config_default(&cfg); cfg.n_taps = 0;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    nvx_tap_config_default(&cfg); cfg.n_inputs = 65536;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    nvx_tap_config_default(&cfg); cfg.n_inputs = 32768; cfg.n_taps = 2;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    nvx_tap_config_default(&cfg); cfg.n_inputs = 65535; cfg.n_taps = 65535;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    nvx_tap_config_default(&cfg); cfg.kind = 2;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    nvx_tap_config_default(&cfg); cfg.kind = -1;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    nvx_tap_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    nvx_tap_config_default(&cfg); cfg.output_rate_hz = 1999;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    nvx_tap_config_default(&cfg); cfg.output_rate_hz = 96001;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    nvx_tap_config_default(&cfg); cfg.output_rate_hz = 7999; cfg.kind = NVX_TAP_REAL;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    nvx_tap_config_default(&cfg); cfg.output_rate_hz = 48001; cfg.kind = NVX_TAP_REAL;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    nvx_tap_config_default(&cfg); cfg.output_rate_hz = 2001;
    EXPECT(nvx_tap_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(strstr(nvx_tap_last_error(), "32768 taps") != NULL, 1);
    nvx_tap_destroy(NULL);
    nvx_tap_destroy(fake);

    EXPECT(nvx_tap_resident(NULL, in, 1024, 1024, out, 32768, 0, &n_out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_tap_resident(fake, in, 1024, 1024, out, 32768, 0, &n_out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_tap_resident(NULL, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, SIZE_MAX, NULL, NULL), NVX_ERR_ARG);
    EXPECT(nvx_tap_push(NULL, 0, few, 1, few, 32, &n_out), NVX_ERR_ARG);
    EXPECT(nvx_tap_push(fake, 0, few, 1, few, 32, &n_out), NVX_ERR_ARG);
    EXPECT(nvx_tap_push(NULL, -1, NULL, SIZE_MAX, NULL, 0, NULL), NVX_ERR_ARG);
    EXPECT(n_out == 7, 1);
    EXPECT(nvx_tap_set_shift(NULL, 0, 0, 100.0, &hz), NVX_ERR_ARG);
    EXPECT(nvx_tap_set_shift(fake, -1, 0, 100.0, &hz), NVX_ERR_ARG);
    EXPECT(nvx_tap_get_shift(NULL, 0, 0, &k, &hz), NVX_ERR_ARG);
    EXPECT(nvx_tap_get_shift(fake, 0, 0, &k, &hz), NVX_ERR_ARG);
    EXPECT(nvx_tap_set_pitch(NULL, 0, 0, 1000.0, &hz), NVX_ERR_ARG);
    EXPECT(nvx_tap_set_pitch(fake, -1, 0, 1000.0, &hz), NVX_ERR_ARG);
    EXPECT(nvx_tap_get_pitch(NULL, 0, 0, &k, &hz), NVX_ERR_ARG);
    EXPECT(nvx_tap_get_pitch(fake, 0, 0, &k, &hz), NVX_ERR_ARG);
    EXPECT(k == -7 && hz == -1.0, 1);
    EXPECT(nvx_tap_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_tap_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_tap_position(NULL, 0, &pos, &made), NVX_ERR_ARG);
    EXPECT(nvx_tap_position(fake, 0, &pos, &made), NVX_ERR_ARG);
    EXPECT(pos == 7 && made == 7, 1);
    EXPECT(nvx_tap_plan(NULL, &L, &M, &T, &ni, &nt, &kind), NVX_ERR_ARG);
    EXPECT(nvx_tap_plan(fake, &L, &M, &T, &ni, &nt, &kind), NVX_ERR_ARG);
    EXPECT(L == -1 && M == -1 && T == -1 && ni == -1 && nt == -1 && kind == -1, 1);
    EXPECT(nvx_tap_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_tap_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_tap_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_tap_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_tap_last_error(), "not a channel tap") != NULL, 1);
    /* the design, the grid and the table need no device and no plan */
    EXPECT(nvx_tap_design(1999, NVX_TAP_IQ, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_tap_design(96001, NVX_TAP_IQ, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_tap_design(7999, NVX_TAP_REAL, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_tap_design(48001, NVX_TAP_REAL, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_tap_design(12000, 2, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_tap_design(2001, NVX_TAP_IQ, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_tap_design(0, NVX_TAP_IQ, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_tap_design(12000, NVX_TAP_IQ, &L, &M, &T, NULL, -1), NVX_ERR_ARG);
    EXPECT(L == -1 && M == -1 && T == -1, 1);
    EXPECT(nvx_tap_design(12000, NVX_TAP_IQ, NULL, NULL, NULL, NULL, 0), 602);
    EXPECT(nvx_tap_design(12000, NVX_TAP_IQ, &L, &M, &T, taps, 601), 602);
    EXPECT(L == 1 && M == 21 && T == 602 && taps[0] == 0 && taps[300] == 0, 1);
    EXPECT(nvx_tap_design(11025, NVX_TAP_REAL, &L, &M, &T, taps, 32768), 7 * 3602);
    EXPECT(L == 7 && M == 160 && T == 3602, 1);
    { long long sum = 0; int t; for (t = 0; t < 3602; t++) sum += taps[5 * 3602 + t]; EXPECT(sum, 1 << 21); }
    EXPECT(nvx_tap_grid(12000, NVX_TAP_IQ, 14000.0, &k, &hz), NVX_OK);
    EXPECT(k == 228 && hz == 228 * 252000.0 / 4096, 1);
    EXPECT(nvx_tap_grid(12000, NVX_TAP_IQ, 14000.0, NULL, NULL), NVX_OK);
    EXPECT(nvx_tap_grid(12000, NVX_TAP_IQ, 121300.0, &k, &hz), NVX_ERR_ARG);
    EXPECT(nvx_tap_grid(1999, NVX_TAP_IQ, 0.0, &k, &hz), NVX_ERR_ARG);
    EXPECT(nvx_tap_grid(12000, 7, 0.0, &k, &hz), NVX_ERR_ARG);
    EXPECT(k == 228, 1);
    EXPECT(nvx_tap_table(NULL, 0), 4096);
    EXPECT(nvx_tap_table(table, 4095), 4096);
    EXPECT(table[0] == 0 && table[1] == 0, 1);
    EXPECT(nvx_tap_table(table, 4096), 4096);
    EXPECT(table[0] == 32767 && table[1] == 0 && table[2 * 1024] == 0 && table[2 * 1024 + 1] == 32767, 1);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("tap null-safety ok\n");
    return 0;
}
