/* The entry points of include/navtex_amd_afc.h called with NULL objects and pointers: error codes, never a crash; and the
 * layouts of its two structs, for tests/test_afc.py to hold against the Python binding's.
 * Linked against libnavtex_amd.so alone, needs no GPU (tests/test_afc.py runs it in a process of its own). */
#include <stddef.h>
#include <stdio.h>
#include "navtex_amd_afc.h"
#define EXPECT(expr, want) do { int r_ = (expr); printf("%-64s -> %d\n", #expr, r_); if (r_ != (want)) bad++; } while (0)
#define FIELD(t, f) printf("layout %s.%s %zu %zu\n", #t, #f, offsetof(t, f), sizeof(((t *)0)->f))
int main(void)
{
    int bad = 0;
    int32_t k[4];
    nvx_afc_config c;
    nvx_afc_status st;
    nvx_afc_config_default(NULL);
    nvx_afc_config_default(&c);
    if (c.struct_size != sizeof c || c.gain_shift != 1 || c.max_step != 8 || c.range_k != 48 || c.min_samples != 256 || c.contrast_min != 0.7) bad++;
    EXPECT(nvx_afc_enable(NULL, 0, 0, &c), NVX_ERR_ARG);
    EXPECT(nvx_afc_enable(NULL, 0, 1, NULL), NVX_ERR_ARG);
    EXPECT(nvx_afc_disable(NULL, 0, 0, 1), NVX_ERR_ARG);
    EXPECT(nvx_afc_read(NULL, 0, 0, &st), NVX_ERR_ARG);
    EXPECT(nvx_afc_read(NULL, 0, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_afc_trace(NULL, 0, 0, k, 4), NVX_ERR_ARG);
    EXPECT(nvx_afc_trace(NULL, 0, 0, NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_group_afc_enable(NULL, 0, 0, &c), NVX_ERR_ARG);
    EXPECT(nvx_group_afc_enable(NULL, 0, 0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_group_afc_disable(NULL, 0, 0, 0), NVX_ERR_ARG);
    EXPECT(nvx_group_afc_read(NULL, 0, 0, &st), NVX_ERR_ARG);
    EXPECT(nvx_group_afc_read(NULL, 0, 1, NULL), NVX_ERR_ARG);
    EXPECT(nvx_group_afc_trace(NULL, 0, 0, k, 4), NVX_ERR_ARG);
    EXPECT(nvx_group_afc_trace(NULL, 0, 0, NULL, 0), NVX_ERR_ARG);
    printf("layout nvx_afc_config * 0 %zu\n", sizeof(nvx_afc_config));
    FIELD(nvx_afc_config, struct_size); FIELD(nvx_afc_config, gain_shift); FIELD(nvx_afc_config, max_step);
    FIELD(nvx_afc_config, range_k); FIELD(nvx_afc_config, min_samples); FIELD(nvx_afc_config, contrast_min);
    printf("layout nvx_afc_status * 0 %zu\n", sizeof(nvx_afc_status));
    FIELD(nvx_afc_status, enabled); FIELD(nvx_afc_status, centre_k); FIELD(nvx_afc_status, k_last); FIELD(nvx_afc_status, last_step);
    FIELD(nvx_afc_status, offset_hz); FIELD(nvx_afc_status, launches); FIELD(nvx_afc_status, updates); FIELD(nvx_afc_status, held);
    FIELD(nvx_afc_status, clamped);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("afc null-safety ok\n");
    return 0;
}
