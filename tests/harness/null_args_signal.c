/* The entry points of include/navtex_amd_signal.h called with NULL objects and pointers: error codes, never a crash.
 * Linked against libnavtex_amd.so alone, needs no GPU (tests/test_signal_report.py runs it in a process of its own). */
#include <stdio.h>
#include "navtex_amd_signal.h"
#define EXPECT(expr, want) do { int r_ = (expr); printf("%-48s -> %d\n", #expr, r_); if (r_ != (want)) bad++; } while (0)
int main(void)
{
    int bad = 0;
    nvx_signal_report rep;
    EXPECT(nvx_enable_signal_report(NULL, 1), NVX_ERR_ARG);
    EXPECT(nvx_enable_signal_report(NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_signal_report_read(NULL, 0, 0, &rep, 0), NVX_ERR_ARG);
    EXPECT(nvx_signal_report_read(NULL, 0, 0, NULL, 1), NVX_ERR_ARG);
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("signal null-safety ok\n");
    return 0;
}
