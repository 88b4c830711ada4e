/* nvx_narrow_design.c -- the narrowband interpolator's plan on the host (include/navtex_amd_narrow.h): L, M, T from the rate,
 * the int16 taps of the Kaiser-windowed sinc.  Plain C, no device.  The Kaiser, sinc and rounding code is
 * csrc/nvx_polyphase_design.h's, which the resampler and the channel tap compile too; here are the range, the band edges
 * and the kernel's limit on T. */
#include "nvx_narrow_plan.h"

#define PASS_HZ 25000.0                      /* nvx_set_carrier's range */
#define PASS_FRACTION 0.4                    /* of fi, where that is less: the band the real-input converter keeps flat */

static double pass_edge(double fi) { return PASS_FRACTION * fi < PASS_HZ ? PASS_FRACTION * fi : PASS_HZ; }

int nvx_nb_plan_numbers(uint32_t num, uint32_t den, int *L, int *M, int *T, const char **why)
{
    if (den != 1 && den != 2) { *why = "rate_den is 1 or 2"; return NVX_ERR_ARG; }
    if (num == 0) { *why = "the input rate is outside 2000 .. 96000 S/s"; return NVX_ERR_ARG; }
    const uint64_t g0 = nvx_pp_gcd(num, den);
    const uint64_t n = num / g0, d = den / g0;
    if (n < (uint64_t)NVX_NB_MIN_RATE * d || n > (uint64_t)NVX_NB_MAX_RATE * d) { *why = "the input rate is outside 2000 .. 96000 S/s"; return NVX_ERR_ARG; }
    const uint64_t out = (uint64_t)NVX_NB_OUTPUT_RATE * d, g = nvx_pp_gcd(out, n);
    const uint64_t l = out / g, m = n / g;
    if (l > NVX_NB_MAX_PHASES) { *why = "the rate needs more than 1024 phases (L / M = 252000 / rate in lowest terms)"; return NVX_ERR_ARG; }
    /* the prototype runs at rate L * fi; the transition is from fp to fi - fp */
    const double fi = (double)n / (double)d, fp = pass_edge(fi);
    const double fs = (double)l * fi;
    const int t = nvx_pp_even_taps(nvx_pp_kaiser_per_phase(fi - 2.0 * fp, fs, (double)l));
    if (t > NVX_NB_MAX_T) { *why = "the rate needs more than 32 taps per phase"; return NVX_ERR_ARG; }
    if ((long)l * t > NVX_NB_MAX_TAPS) { *why = "the rate needs more than 32768 taps (L * T)"; return NVX_ERR_ARG; }
    *L = (int)l; *M = (int)m; *T = t;
    return NVX_OK;
}

int nvx_nb_plan_taps(int L, int T, int16_t *taps, const char **why)
{
    long long *row;
    double *p = nvx_pp_prototype(0.5 / (double)L, L, T, &row);  /* fi / 2 in cycles per sample of the prototype */
    if (!p) { *why = "out of memory"; return NVX_ERR_NOMEM; }
    int rc = NVX_OK;
    for (int r = 0; r < L && rc == NVX_OK; r++) {
        int big;
        const long long isum = nvx_pp_phase(p, L, T, r, NVX_NB_SHIFT, row, &big);
        long long asum = 0;
        for (int t = 0; t < T; t++) taps[r * T + t] = (int16_t)row[t];          /* |v| <= about 2^14: a phase is at most a unit pulse */
        /* the rounding residue onto the largest tap */
        row[big] += (1LL << NVX_NB_SHIFT) - isum;
        if (row[big] > 32767 || row[big] < -32768) { *why = "a tap leaves int16"; rc = NVX_ERR_ARG; break; }
        taps[r * T + big] = (int16_t)row[big];
        for (int t = 0; t < T; t++) asum += llabs(row[t]);
        if (asum > 65535) { *why = "a phase's absolute tap sum exceeds 65535: the accumulator could leave int32"; rc = NVX_ERR_ARG; }
    }
    free(p);
    return rc;
}
