// wanc_solve.cpp -- the multi-tap canceller's solve (navtex_amd/wanc/nvx_wanc_solve.h) on the host, without a device.
//   wanc_solve div      nvx_wanc_div against the processor's IEEE division: corner cases, and random operands of every
//                       exponent, subnormal operands and results and overflow among them
//   wanc_solve solve    reads cases from the standard input, "K window_log2 load_log2 TAA" and then 4 K integers (Re R, Im R,
//                       Re Q, Im Q), and prints "reason coherence w_re[0 .. K) w_im[0 .. K)" per case: tests/test_wanc.py holds
//                       the lines against the restatement
// Built with -fsanitize=address,undefined -ffp-contract=off by tests/test_wanc.py; no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nvx_wanc_solve.h"

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint64_t rnd(void) { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

static long g_checks = 0;
static void check_div(double n, double d)
{
    volatile double vn = n, vd = d;
    const double want = vn / vd, got = nvx_wanc_div(n, d);
    g_checks++;
    if (nvx_wanc_bits(want) != nvx_wanc_bits(got) && !(want != want && got != got)) {
        fprintf(stderr, "nvx_wanc_div(%a, %a) = %a, the processor's %a\n", n, d, got, want);
        exit(1);
    }
}

static int run_div(void)
{
    const double specials[] = { 0.0, -0.0, 1.0, -1.0, 3.0, 1.0 / 3.0, 0x1p-1074, 0x1p-1022, 0x1.fffffffffffffp-1023, 0x1.fffffffffffffp1023, 0x1p53, 0x1p52 + 1,
                                0x1.0000000000001p0, 0x1.fffffffffffffp0, 16384.0, 1e300, 1e-300, __builtin_inf(), -__builtin_inf(), __builtin_nan("") };
    for (double n : specials)
        for (double d : specials)
            if (d > 0.0 && d < __builtin_inf()) { check_div(n, d); check_div(-n, d); }
    for (long i = 0; i < 4000000; i++) {
        uint64_t nb = rnd(), db = rnd() & 0x7fffffffffffffffull;
        const int kind = (int)(rnd() % 8);
        if (kind == 0) nb &= 0x800fffffffffffffull;                                     // a subnormal numerator
        if (kind == 1) db &= 0x000fffffffffffffull;                                     // a subnormal divisor
        if (kind == 2) { nb = (nb & 0x800fffffffffffffull) | ((uint64_t)(rnd() % 80 + 1) << 52); db = (db & 0x000fffffffffffffull) | ((uint64_t)(1023 + rnd() % 80) << 52); }
        if (kind == 3) { nb = (nb & 0x800fffffffffffffull) | ((uint64_t)(2046 - rnd() % 40) << 52); db = (db & 0x000fffffffffffffull) | ((uint64_t)(1023 - rnd() % 60) << 52); }
        if (kind == 4) nb = nvx_wanc_bits(1.0);
        if (kind == 5) { nb &= 0x800ffffffff00000ull; nb |= 0x3ff0000000000000ull; db &= 0x000fffff00000000ull; db |= 0x3ff0000000000000ull; }   // near ties
        if ((db >> 52) == 0x7ff || db == 0 || ((nb >> 52) & 0x7ff) == 0x7ff) continue;
        check_div(nvx_wanc_from_bits(nb), nvx_wanc_from_bits(db));
    }
    printf("wanc div ok: %ld checks\n", g_checks);
    return 0;
}

static int run_solve(void)
{
    int K, wl, ll;
    long long taa;
    while (scanf("%d %d %d %lld", &K, &wl, &ll, &taa) == 4) {
        if (K != 4 && K != 8 && K != 16) return 2;
        std::vector<long long> sums(4 * K);
        for (auto &v : sums)
            if (scanf("%lld", &v) != 1) return 2;
        std::vector<double> ws(NVX_WANC_WS_DOUBLES(K), 0.0);
        for (int k = 0; k < 4 * K; k++) ws[k] = (double)sums[k];
        std::vector<int32_t> w(2 * K);
        int32_t coherence = -1;
        const int reason = nvx_wanc_solve(K, wl, ll, sums[0], taa, ws.data(), 1, w.data(), 1, &coherence);
        printf("%d %d", reason, coherence);
        for (int k = 0; k < 2 * K; k++) printf(" %d", w[k]);
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "div")) return run_div();
    if (argc == 2 && !strcmp(argv[1], "solve")) return run_solve();
    fprintf(stderr, "usage: wanc_solve div | solve\n");
    return 2;
}
