/* The entry points of include/navtex_amd_soft.h called with NULL objects and pointers: error codes and no-ops, never a
 * crash.  Linked against libnavtex_amd.so alone, needs no GPU (tests/test_soft.py runs it in a process of its own). */
#include <stdio.h>
#include "navtex_amd_soft.h"
#define EXPECT(expr, want) do { long r_ = (long)(expr); printf("%-56s -> %ld\n", #expr, r_); if (r_ != (long)(want)) bad++; } while (0)
static void sink(void *user, int stream, const char *bbbb, const char *message, int freq)
{
    (void)user; (void)stream; (void)bbbb; (void)message; (void)freq;
}
static int n_msgs;
static void count(void *user, const char *bbbb, const char *message, int freq) { (void)user; (void)bbbb; (void)message; (void)freq; n_msgs++; }
int main(void)
{
    int bad = 0;
    float v[4] = { 1.0f, -1.0f, 0.0f, 2.0f };
    EXPECT(nvx_enable_soft(NULL, 0), NVX_ERR_ARG);
    EXPECT(nvx_enable_soft(NULL, NVX_SOFT_DECODE), NVX_ERR_ARG);
    EXPECT(nvx_enable_soft(NULL, NVX_SOFT_DECODE | NVX_SOFT_KEEP), NVX_ERR_ARG);
    EXPECT(nvx_set_soft_message_fn(NULL, sink, NULL), NVX_ERR_ARG);
    EXPECT(nvx_set_soft_message_fn(NULL, NULL, NULL), NVX_ERR_ARG);
    EXPECT(nvx_set_soft_message_fn(NULL, nvx_store_on_message, NULL), NVX_ERR_ARG);
    EXPECT(nvx_poll_soft(NULL, 0, 0, v, 4), 0);
    EXPECT(nvx_poll_soft(NULL, 0, 0, NULL, 4), 0);
    EXPECT(nvx_soft_count(NULL, 0, 0), 0);
    nvx_sitor_set_soft(NULL, 1);                               /* no-ops */
    nvx_sitor_receive_soft(NULL, v, 4);
    {
        nvx_sitor *s = nvx_sitor_new(518, count, NULL);
        if (!s) { printf("nvx_sitor_new failed\n"); return 1; }
        nvx_sitor_receive_soft(s, NULL, 4);
        nvx_sitor_set_soft(s, 1);
        nvx_sitor_receive_soft(s, NULL, 4);
        nvx_sitor_receive_soft(s, v, 0);
        nvx_sitor_receive_soft(s, v, 4);
        nvx_sitor_set_soft(s, 0);
        nvx_sitor_free(s);
        EXPECT(n_msgs, 0);
    }
    if (bad) { printf("null-safety FAILED: %d\n", bad); return 1; }
    printf("soft null-safety ok\n");
    return 0;
}
