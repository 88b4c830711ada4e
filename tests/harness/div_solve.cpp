// div_solve.cpp -- the diversity combiner's solve (navtex_amd/div/nvx_div_solve.h) on the host, stand-alone: reads rows of
// "TAA TBB TRE TIM" from the file named on the command line and prints "lead w_re w_im coherence reason" for each, which
// tests/test_div.py holds against the restatement's Python integers line for line.  It also checks the square root and the
// two divisions against their definitions on every row.  Built with -fsanitize=address,undefined; no HIP.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "nvx_div_solve.h"

typedef unsigned __int128 u128;

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: div_solve ROWS\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int64_t t[4];
    long rows = 0;
    while (fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64, &t[0], &t[1], &t[2], &t[3]) == 4) {
        int32_t lead, w_re, w_im, coherence;
        const int reason = nvx_div_solve(t[0], t[1], t[2], t[3], &lead, &w_re, &w_im, &coherence);
        printf("%d %d %d %d %d\n", lead, w_re, w_im, coherence, reason);
        // the helpers on this row's numbers: r * r <= q < (r + 1)^2, and n = q d + rem with 0 <= rem < d
        const uint64_t q = (uint64_t)(t[0] < 0 ? -t[0] : t[0]) >> 2, r = nvx_div_isqrt(q);
        if ((u128)r * r > q || (u128)(r + 1) * (r + 1) <= q) { fprintf(stderr, "isqrt(%" PRIu64 ") = %" PRIu64 "\n", q, r); return 1; }
        const int64_t d = (t[1] < 0 ? -t[1] : t[1]) % 1000003 + 1, quot = nvx_div_floor_div(t[2], d);
        if ((__int128)quot * d > t[2] || (__int128)(quot + 1) * d <= t[2]) { fprintf(stderr, "floor_div(%" PRId64 ", %" PRId64 ") = %" PRId64 "\n", t[2], d, quot); return 1; }
        if (nvx_div_bitlength((uint64_t)t[0]) != (t[0] ? 64 - __builtin_clzll((uint64_t)t[0]) : 0)) { fprintf(stderr, "bitlength(%" PRId64 ")\n", t[0]); return 1; }
        rows++;
    }
    fclose(f);
    fprintf(stderr, "div solve ok: %ld rows\n", rows);
    return 0;
}
