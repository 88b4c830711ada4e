/* The entry points of include/navtex_amd_tune.h called with NULL objects and pointers: error codes, never a crash.
 * Linked against libnavtex_amd.so alone, needs no GPU (tests/test_tune.py runs it in a process of its own). */
#include <stdio.h>
#include "navtex_amd_tune.h"
#define EXPECT(expr, want) do { int r_ = (expr); printf("%-56s -> %d\n", #expr, r_); if (r_ != (want)) bad++; } while (0)
int main(void)
{
    int bad = 0, ref = 0;
    double hz = 0.0;
    EXPECT(nvx_set_carrier(NULL, 0, 0, 14000.0, &hz), NVX_ERR_ARG);
    EXPECT(nvx_set_carrier(NULL, 0, 1, -14000.0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_get_carrier(NULL, 0, 0, &hz, &ref), NVX_ERR_ARG);
    EXPECT(nvx_get_carrier(NULL, 0, 0, NULL, NULL), NVX_ERR_ARG);
    EXPECT(nvx_group_set_carrier(NULL, 0, 0, 14000.0, &hz), NVX_ERR_ARG);
    EXPECT(nvx_group_set_carrier(NULL, 0, 0, 14000.0, NULL), NVX_ERR_ARG);
    EXPECT(nvx_group_get_carrier(NULL, 0, 0, &hz, &ref), NVX_ERR_ARG);
    EXPECT(nvx_group_get_carrier(NULL, 0, 1, NULL, NULL), NVX_ERR_ARG);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("tune null-safety ok\n");
    return 0;
}
