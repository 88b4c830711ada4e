/* The entry points of include/navtex_amd_narrow.h called with NULL and nonsense arguments: error codes, never a crash, and
 * never a launch (every call here is refused before a device is looked for).  Linked against libnavtex_amd_narrow.so alone,
 * needs no GPU (tests/test_narrow.py runs it in a process of its own). */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_narrow.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t few[64];
static int16_t taps[32768];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, ns = -1, fmt = -1, kind = -1, L = -1, M = -1, T = -1;
    uint64_t n = 7, pos = 7, made = 7;
    size_t n_out = 7;
    double ms = -1.0;
    void *in = (void *)(uintptr_t)0x100000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_nb_interpolator *c = (nvx_nb_interpolator *)(uintptr_t)0x300000, *fake = (nvx_nb_interpolator *)not_a_plan;
    nvx_nb_config cfg;

    nvx_nb_config_default(NULL);
    nvx_nb_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.n_streams == 1 && cfg.rate_num == 12000 && cfg.rate_den == 1, 1);
    EXPECT(cfg.format == NVX_NB_S16 && cfg.kind == NVX_NB_IQ, 1);
    EXPECT(nvx_nb_create(NULL, &c), NVX_ERR_ARG);
    EXPECT(nvx_nb_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_nb_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(c == NULL, 1);
    nvx_nb_config_default(&cfg); cfg.n_streams = 0;
    EXPECT(nvx_nb_create(&cfg, &c), NVX_ERR_ARG);
    nvx_nb_config_default(&cfg); cfg.n_streams = 65536;
    EXPECT(nvx_nb_create(&cfg, &c), NVX_ERR_ARG);
    nvx_nb_config_default(&cfg); cfg.format = 4;
    EXPECT(nvx_nb_create(&cfg, &c), NVX_ERR_ARG);
    nvx_nb_config_default(&cfg); cfg.format = -1;
    EXPECT(nvx_nb_create(&cfg, &c), NVX_ERR_ARG);
    nvx_nb_config_default(&cfg); cfg.kind = 2;
    EXPECT(nvx_nb_create(&cfg, &c), NVX_ERR_ARG);
    nvx_nb_config_default(&cfg); cfg.kind = -1;
    EXPECT(nvx_nb_create(&cfg, &c), NVX_ERR_ARG);
    nvx_nb_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_nb_create(&cfg, &c), NVX_ERR_ARG);
    nvx_nb_config_default(&cfg); cfg.rate_num = 1999;
    EXPECT(nvx_nb_create(&cfg, &c), NVX_ERR_ARG);
    nvx_nb_config_default(&cfg); cfg.rate_num = 96001;
    EXPECT(nvx_nb_create(&cfg, &c), NVX_ERR_ARG);
    nvx_nb_config_default(&cfg); cfg.rate_den = 0;
    EXPECT(nvx_nb_create(&cfg, &c), NVX_ERR_ARG);
    nvx_nb_config_default(&cfg); cfg.rate_den = 3;
    EXPECT(nvx_nb_create(&cfg, &c), NVX_ERR_ARG);
    nvx_nb_config_default(&cfg); cfg.rate_num = 2001;
    EXPECT(nvx_nb_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(strstr(nvx_nb_last_error(), "1024 phases") != NULL, 1);
    nvx_nb_destroy(NULL);
    nvx_nb_destroy(fake);

    EXPECT(nvx_nb_resident(NULL, in, 1024, 1024, out, 32768, 0, &n_out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_nb_resident(fake, in, 1024, 1024, out, 32768, 0, &n_out, NULL), NVX_ERR_ARG);
    EXPECT(nvx_nb_resident(NULL, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, SIZE_MAX, NULL, NULL), NVX_ERR_ARG);
    EXPECT(nvx_nb_push(NULL, 0, few, 1, few, 32, &n_out), NVX_ERR_ARG);
    EXPECT(nvx_nb_push(fake, 0, few, 1, few, 32, &n_out), NVX_ERR_ARG);
    EXPECT(nvx_nb_push(NULL, -1, NULL, SIZE_MAX, NULL, 0, NULL), NVX_ERR_ARG);
    EXPECT(n_out == 7, 1);
    EXPECT(nvx_nb_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_nb_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_nb_position(NULL, 0, &pos, &made), NVX_ERR_ARG);
    EXPECT(nvx_nb_position(fake, 0, &pos, &made), NVX_ERR_ARG);
    EXPECT(pos == 7 && made == 7, 1);
    EXPECT(nvx_nb_plan(NULL, &L, &M, &T, &ns, &fmt, &kind), NVX_ERR_ARG);
    EXPECT(nvx_nb_plan(fake, &L, &M, &T, &ns, &fmt, &kind), NVX_ERR_ARG);
    EXPECT(L == -1 && M == -1 && T == -1 && ns == -1 && fmt == -1 && kind == -1, 1);
    EXPECT(nvx_nb_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_nb_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_nb_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_nb_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_nb_last_error(), "not a narrowband interpolator") != NULL, 1);
    /* the design needs no device and no plan */
    EXPECT(nvx_nb_design(1999, 1, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_nb_design(96001, 1, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_nb_design(192001, 2, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_nb_design(12000, 0, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_nb_design(12000, 3, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_nb_design(2001, 1, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_nb_design(0, 1, &L, &M, &T, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_nb_design(12000, 1, &L, &M, &T, NULL, -1), NVX_ERR_ARG);
    EXPECT(L == -1 && M == -1 && T == -1, 1);
    EXPECT(nvx_nb_design(12000, 1, NULL, NULL, NULL, NULL, 0), 21 * 30);
    EXPECT(nvx_nb_design(24000, 2, &L, &M, &T, taps, 21 * 30 - 1), 21 * 30);
    EXPECT(L == 21 && M == 1 && T == 30 && taps[0] == 0 && taps[21 * 30 - 2] == 0, 1);
    EXPECT(nvx_nb_design(11025, 2, &L, &M, &T, taps, 32768), 320 * 30);
    EXPECT(L == 320 && M == 7 && T == 30, 1);
    { long sum = 0; int t; for (t = 0; t < 30; t++) sum += taps[5 * 30 + t]; EXPECT(sum, 16384); }
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("narrow null-safety ok\n");
    return 0;
}
