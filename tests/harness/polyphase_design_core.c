/* polyphase_design_core.c -- the three designs that stand on navtex_amd/csrc/nvx_polyphase_design.h (the resampler's, the
 * narrowband interpolator's, the channel tap's) without a device: for the rates the tests name and the rates at the edges
 * of each range (the most phases, the most taps, the longest phase), what the public headers promise of the taps -- every
 * phase sums to exactly 2^S, the taps lie in their type's range, a phase's absolute sums stay within their bounds, T is
 * even and L * T within the table -- and the count rule against a restatement in 128-bit integers at positions up to 2^62.
 * The taps live in an allocation of exactly L * T entries, so a write past it is the sanitizer's to report.
 * Built with -fsanitize=address,undefined by tests/test_polyphase_design.py; links the three nvx_*_design.c, no HIP. */
#include <stdio.h>
#include <stdlib.h>

#include "nvx_narrow_plan.h"
#include "nvx_resample_plan.h"
#include "nvx_tap_plan.h"

typedef unsigned __int128 u128;

static long g_checks = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        g_checks++;                                                             \
        if (!(cond)) {                                                          \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);          \
            fprintf(stderr, __VA_ARGS__);                                       \
            fprintf(stderr, "\n");                                              \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

/* ceil(n L / M) by quotient and remainder */
static u128 restated_outputs_after(uint64_t n, int L, int M)
{
    const u128 pos = (u128)n * (u128)(unsigned)L;
    return pos / (unsigned)M + (pos % (unsigned)M ? 1 : 0);
}

enum which { RS, NB, TAP };

static void check_counts(enum which w, const char *name, int L, int M)
{
    const uint64_t one = 1;
    const uint64_t positions[] = { 0, 1, 2, (uint64_t)M - 1, (uint64_t)M, (uint64_t)M + 1, (uint64_t)L * (uint64_t)M, (one << 31) - 1, one << 31, (one << 32) + 1,
                                   (one << 54) - 1, (one << 54) + 1, (one << 62) - (uint64_t)M, (one << 62) - 1, one << 62 };
    for (size_t i = 0; i < sizeof positions / sizeof positions[0]; i++) {
        const uint64_t n = positions[i];
        const u128 want = restated_outputs_after(n, L, M);
        u128 wide = want;
        uint64_t low = 0;
        if (w == RS) low = nvx_rs_outputs_after(n, L, M);
        if (w == NB) { wide = nvx_nb_outputs_after_wide(n, L, M); low = nvx_nb_outputs_after(n, L, M); }
        if (w == TAP) { wide = nvx_tap_outputs_after_wide(n, L, M); low = nvx_tap_outputs_after(n, L, M); }
        CHECK(wide == want && low == (uint64_t)want, "%s: outputs after %llu samples: %llu", name, (unsigned long long)n, (unsigned long long)low);
        CHECK(nvx_pp_outputs_after_wide(n, L, M) == want && nvx_pp_outputs_after(n, L, M) == (uint64_t)want, "%s: the core's count after %llu samples", name,
              (unsigned long long)n);
    }
}

/* every phase of L * T taps: its sum, its absolute sum, the absolute sum of its high halves, its extremes */
static void check_phases(const char *name, const long long *taps, int L, int T, int S, long long lo, long long hi, long long abs_bound, long long high_bound)
{
    for (int r = 0; r < L; r++) {
        long long sum = 0, asum = 0, hsum = 0;
        for (int t = 0; t < T; t++) {
            const long long v = taps[(size_t)r * T + t];
            CHECK(v >= lo && v <= hi, "%s: tap %d of phase %d is %lld", name, t, r, v);
            sum += v; asum += llabs(v); hsum += llabs(v >> 8);
        }
        CHECK(sum == (1LL << S), "%s: phase %d sums to %lld, not 2^%d", name, r, sum, S);
        CHECK(asum <= abs_bound, "%s: phase %d has the absolute sum %lld", name, r, asum);
        if (high_bound) CHECK(hsum <= high_bound, "%s: phase %d has the high-half sum %lld", name, r, hsum);
    }
}

static void check_shape(const char *name, int L, int M, int T, long max_phases, long max_taps)
{
    CHECK(L >= 1 && M >= 1 && T >= 8 && !(T & 1), "%s: L %d M %d T %d", name, L, M, T);
    CHECK(L <= max_phases && (long)L * T <= max_taps, "%s: L %d, L * T %ld", name, L, (long)L * T);
    CHECK(nvx_pp_gcd((uint64_t)L, (uint64_t)M) == 1, "%s: L %d / M %d is not in lowest terms", name, L, M);
}

static long long *widen16(const int16_t *h, size_t n)
{
    long long *w = (long long *)malloc(n * sizeof *w);
    if (!w) { fprintf(stderr, "out of memory\n"); exit(1); }
    for (size_t i = 0; i < n; i++) w[i] = h[i];
    return w;
}

static void check_resampler(uint32_t rate)
{
    char name[64];
    snprintf(name, sizeof name, "resampler %u S/s", rate);
    int L, M, T;
    const char *why = "";
    CHECK(nvx_rs_plan_numbers(rate, &L, &M, &T, &why) == NVX_OK, "%s: %s", name, why);
    check_shape(name, L, M, T, NVX_RS_MAX_PHASES, NVX_RS_MAX_TAPS);
    const size_t n = (size_t)L * T;
    int16_t *h = (int16_t *)malloc(n * sizeof *h);
    CHECK(h && nvx_rs_plan_taps(rate, L, T, h, &why) == NVX_OK, "%s: %s", name, why);
    long long *w = widen16(h, n);
    check_phases(name, w, L, T, NVX_RS_SHIFT, -32768, 32767, 65535, 0);
    check_counts(RS, name, L, M);
    free(w); free(h);
}

static void check_narrow(uint32_t num, uint32_t den)
{
    char name[64];
    snprintf(name, sizeof name, "interpolator %u / %u S/s", num, den);
    int L, M, T;
    const char *why = "";
    CHECK(nvx_nb_plan_numbers(num, den, &L, &M, &T, &why) == NVX_OK, "%s: %s", name, why);
    check_shape(name, L, M, T, NVX_NB_MAX_PHASES, NVX_NB_MAX_TAPS);
    CHECK(T <= NVX_NB_MAX_T && L > M, "%s: T %d, L %d / M %d", name, T, L, M);
    const size_t n = (size_t)L * T;
    int16_t *h = (int16_t *)malloc(n * sizeof *h);
    CHECK(h && nvx_nb_plan_taps(L, T, h, &why) == NVX_OK, "%s: %s", name, why);
    long long *w = widen16(h, n);
    check_phases(name, w, L, T, NVX_NB_SHIFT, -32768, 32767, 65535, 0);
    check_counts(NB, name, L, M);
    free(w); free(h);
}

static void check_tap(uint32_t fo, int kind)
{
    char name[64];
    snprintf(name, sizeof name, "tap %u S/s, kind %d", fo, kind);
    int L, M, T;
    const char *why = "";
    CHECK(nvx_tap_plan_numbers(fo, kind, &L, &M, &T, &why) == NVX_OK, "%s: %s", name, why);
    check_shape(name, L, M, T, NVX_TAP_MAX_TAPS, NVX_TAP_MAX_TAPS);
    CHECK(L < M, "%s: L %d / M %d", name, L, M);
    const size_t n = (size_t)L * T;
    int32_t *h = (int32_t *)malloc(n * sizeof *h);
    CHECK(h && nvx_tap_plan_taps(fo, kind, L, T, h, &why) == NVX_OK, "%s: %s", name, why);
    long long *w = (long long *)malloc(n * sizeof *w);
    CHECK(w != NULL, "%s: out of memory", name);
    for (size_t i = 0; i < n; i++) w[i] = h[i];
    check_phases(name, w, L, T, NVX_TAP_SHIFT, -(1LL << 24) + 1, (1LL << 24) - 1, (1LL << 24) - 1, 65535);
    check_counts(TAP, name, L, M);
    free(w); free(h);
}

int main(void)
{
    /* tests/resample_ref.py's RATES, the two the launch tests add, L = 1 (M = 1 and M = 12), then the edges: L = 1008 (the most
     * phases a rate can have), L * T = 32760, T = 92; the ends of the range are among the first */
    static const uint32_t RS_RATES[] = { 2048000, 2400000, 2000000, 1920000, 3200000, 1024000, 768000, 384000, 256000, 250000, 192000, 96000, 252252, 100100,
                                         252000, 3024000, 97250, 1000250, 1768400, 1771600, 3175200, 3180000 };
    for (size_t i = 0; i < sizeof RS_RATES / sizeof RS_RATES[0]; i++) check_resampler(RS_RATES[i]);

    /* tests/narrow_cases.py's DESIGN_RATES, then L = 1008 with L * T = 30240 (the most of both), a half-integer rate there, and
     * the ends of the range */
    static const uint32_t NB_RATES[][2] = { { 2000, 1 }, { 4000, 1 }, { 11025, 2 }, { 6000, 1 }, { 8000, 1 }, { 11025, 1 }, { 12000, 1 }, { 16000, 1 }, { 22050, 1 },
                                            { 24000, 1 }, { 32000, 1 }, { 44100, 1 }, { 48000, 1 }, { 50000, 1 }, { 64000, 1 }, { 88200, 1 }, { 96000, 1 },
                                            { 12500, 1 }, { 7350, 1 }, { 72000, 1 }, { 67200, 1 }, { 75600, 1 }, { 70000, 1 }, { 73332, 1 }, { 84000, 1 },
                                            { 64800, 1 }, { 2750, 1 }, { 4750, 1 }, { 5500, 2 }, { 4000, 2 }, { 192000, 2 } };
    for (size_t i = 0; i < sizeof NB_RATES / sizeof NB_RATES[0]; i++) check_narrow(NB_RATES[i][0], NB_RATES[i][1]);

    /* tests/tap_cases.py's DESIGNS, then the edges: L * T = 32756 and 32708, L = 998, and the ends of the audio range */
    static const uint32_t TAP_DESIGNS[][2] = { { 2000, NVX_TAP_IQ }, { 6250, NVX_TAP_IQ }, { 8000, NVX_TAP_IQ }, { 11025, NVX_TAP_IQ }, { 12000, NVX_TAP_IQ },
                                               { 24000, NVX_TAP_IQ }, { 48000, NVX_TAP_IQ }, { 96000, NVX_TAP_IQ }, { 8000, NVX_TAP_REAL }, { 11025, NVX_TAP_REAL },
                                               { 12000, NVX_TAP_REAL }, { 44100, NVX_TAP_REAL }, { 48000, NVX_TAP_REAL }, { 68960, NVX_TAP_IQ },
                                               { 78625, NVX_TAP_IQ }, { 95808, NVX_TAP_IQ }, { 16000, NVX_TAP_REAL } };
    for (size_t i = 0; i < sizeof TAP_DESIGNS / sizeof TAP_DESIGNS[0]; i++) check_tap(TAP_DESIGNS[i][0], (int)TAP_DESIGNS[i][1]);

    /* a refusal leaves through its sentence, with nothing written */
    int L = -1, M = -1, T = -1;
    const char *why = NULL;
    CHECK(nvx_rs_plan_numbers(95999, &L, &M, &T, &why) == NVX_ERR_ARG && why && L == -1, "the resampler took 95999 S/s");
    why = NULL;
    CHECK(nvx_nb_plan_numbers(12000, 3, &L, &M, &T, &why) == NVX_ERR_ARG && why && L == -1, "the interpolator took rate_den 3");
    why = NULL;
    CHECK(nvx_tap_plan_numbers(7999, NVX_TAP_REAL, &L, &M, &T, &why) == NVX_ERR_ARG && why && L == -1, "the tap took audio at 7999 S/s");

    printf("polyphase design core ok: %ld checks\n", g_checks);
    return 0;
}
