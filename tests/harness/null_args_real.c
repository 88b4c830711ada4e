/* The entry points of include/navtex_amd_real.h called with NULL and nonsense arguments: error codes, never a crash, and
 * never a launch (every call here is refused before a device is looked for).  Linked against libnavtex_amd_real.so alone,
 * needs no GPU (tests/test_real.py runs it in a process of its own). */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "navtex_amd_real.h"
#define EXPECT(expr, want) do { long long r_ = (long long)(expr); printf("%-110s -> %lld\n", #expr, r_); if (r_ != (long long)(want)) bad++; } while (0)
static int16_t few[64];
static uint64_t not_a_plan[64];                /* zeroed memory where a plan is expected */
int main(void)
{
    int bad = 0, ns = -1, fmt = -1, inv = -1, K = -1, S = -1;
    uint64_t n = 7, pos = 7, made = 7;
    size_t n_out = 7;
    double ms = -1.0;
    int16_t taps[14];
    void *in = (void *)(uintptr_t)0x100000, *out = (void *)(uintptr_t)0x200000;      /* never dereferenced: refused first */
    nvx_real_converter *c = (nvx_real_converter *)(uintptr_t)0x300000, *fake = (nvx_real_converter *)not_a_plan;
    nvx_real_config cfg;

    nvx_real_config_default(NULL);
    nvx_real_config_default(&cfg);
    EXPECT(cfg.struct_size == sizeof cfg && cfg.device == 0 && cfg.format == NVX_REAL_S16 && cfg.n_streams == 1 && cfg.invert == 0, 1);
    EXPECT(nvx_real_create(NULL, &c), NVX_ERR_ARG);
    EXPECT(nvx_real_create(&cfg, NULL), NVX_ERR_ARG);
    cfg.struct_size = 8;
    EXPECT(nvx_real_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(c == NULL, 1);
    nvx_real_config_default(&cfg); cfg.n_streams = 0;
    EXPECT(nvx_real_create(&cfg, &c), NVX_ERR_ARG);
    nvx_real_config_default(&cfg); cfg.n_streams = 65536;
    EXPECT(nvx_real_create(&cfg, &c), NVX_ERR_ARG);
    nvx_real_config_default(&cfg); cfg.format = 4;
    EXPECT(nvx_real_create(&cfg, &c), NVX_ERR_ARG);
    nvx_real_config_default(&cfg); cfg.format = -1;
    EXPECT(nvx_real_create(&cfg, &c), NVX_ERR_ARG);
    nvx_real_config_default(&cfg); cfg.device = -1;
    EXPECT(nvx_real_create(&cfg, &c), NVX_ERR_ARG);
    nvx_real_config_default(&cfg); cfg.invert = 2;
    EXPECT(nvx_real_create(&cfg, &c), NVX_ERR_ARG);
    nvx_real_config_default(&cfg); cfg.invert = -1;
    EXPECT(nvx_real_create(&cfg, &c), NVX_ERR_ARG);
    EXPECT(nvx_real_last_error() != NULL && nvx_real_last_error()[0] != 0, 1);
    nvx_real_destroy(NULL);
    nvx_real_destroy(fake);

    EXPECT(nvx_real_resident(NULL, in, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_real_resident(fake, in, 1024, 1024, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_real_resident(fake, in, 1024, 1023, out, 1024, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_real_resident(NULL, NULL, 0, SIZE_MAX, NULL, SIZE_MAX, SIZE_MAX, NULL), NVX_ERR_ARG);
    EXPECT(nvx_real_push(NULL, 0, few, 16, few, 32, &n_out), NVX_ERR_ARG);
    EXPECT(nvx_real_push(fake, 0, few, 16, few, 32, &n_out), NVX_ERR_ARG);
    EXPECT(nvx_real_push(NULL, -1, NULL, SIZE_MAX, NULL, 0, NULL), NVX_ERR_ARG);
    EXPECT(n_out == 7, 1);
    EXPECT(nvx_real_reset(NULL, -1), NVX_ERR_ARG);
    EXPECT(nvx_real_reset(fake, 0), NVX_ERR_ARG);
    EXPECT(nvx_real_position(NULL, 0, &pos, &made), NVX_ERR_ARG);
    EXPECT(nvx_real_position(fake, 0, &pos, &made), NVX_ERR_ARG);
    EXPECT(pos == 7 && made == 7, 1);
    EXPECT(nvx_real_plan(NULL, &fmt, &ns, &inv), NVX_ERR_ARG);
    EXPECT(nvx_real_plan(fake, &fmt, &ns, &inv), NVX_ERR_ARG);
    EXPECT(ns == -1 && fmt == -1 && inv == -1, 1);
    EXPECT(nvx_real_timing(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_real_timing(fake, 1), NVX_ERR_ARG);
    EXPECT(nvx_real_time_stats(NULL, &ms, &n, 1), NVX_ERR_ARG);
    EXPECT(nvx_real_time_stats(fake, NULL, NULL, 0), NVX_ERR_ARG);
    EXPECT(ms == -1.0 && n == 7, 1);
    EXPECT(strstr(nvx_real_last_error(), "not a real-input converter") != NULL, 1);
    /* the taps need no device and no plan */
    EXPECT(nvx_real_taps(taps, 13, &K, &S), NVX_ERR_ARG);
    EXPECT(K == -1 && S == -1, 1);
    EXPECT(nvx_real_taps(NULL, 0, &K, &S), 14);
    EXPECT(K == 13 && S == 14, 1);
    EXPECT(nvx_real_taps(taps, 14, NULL, NULL), 14);
    EXPECT(taps[0] == 10376 && taps[13] == 1, 1);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("real null-safety ok\n");
    return 0;
}
