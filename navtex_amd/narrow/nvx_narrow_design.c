/* nvx_narrow_design.c -- the narrowband interpolator's plan on the host (include/navtex_amd_narrow.h): L, M, T from the rate,
 * the int16 taps of the Kaiser-windowed sinc.  Plain C, no device.  The Kaiser, sinc and rounding code is
 * the resampler's (navtex_amd/resample/nvx_resample_design.c), copied: the two libraries share no object. */
#include <math.h>
#include <stdlib.h>

#include "nvx_narrow_plan.h"

#define PASS_HZ 25000.0                      /* nvx_set_carrier's range */
#define PASS_FRACTION 0.4                    /* of fi, where that is less: the band the real-input converter keeps flat */
#define DESIGN_DB 90.0

static uint64_t gcd_u64(uint64_t a, uint64_t b)
{
    while (b) { uint64_t t = a % b; a = b; b = t; }
    return a;
}

/* modified Bessel function I0 by its power series */
static double bessel_i0(double x)
{
    double sum = 1.0, term = 1.0;
    const double h = 0.5 * x;
    for (int k = 1; k < 200; k++) {
        term *= (h / k) * (h / k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

static double pass_edge(double fi) { return PASS_FRACTION * fi < PASS_HZ ? PASS_FRACTION * fi : PASS_HZ; }

int nvx_nb_plan_numbers(uint32_t num, uint32_t den, int *L, int *M, int *T, const char **why)
{
    if (den != 1 && den != 2) { *why = "rate_den is 1 or 2"; return NVX_ERR_ARG; }
    if (num == 0) { *why = "the input rate is outside 2000 .. 96000 S/s"; return NVX_ERR_ARG; }
    const uint64_t g0 = gcd_u64(num, den);
    const uint64_t n = num / g0, d = den / g0;
    if (n < (uint64_t)NVX_NB_MIN_RATE * d || n > (uint64_t)NVX_NB_MAX_RATE * d) { *why = "the input rate is outside 2000 .. 96000 S/s"; return NVX_ERR_ARG; }
    const uint64_t out = (uint64_t)NVX_NB_OUTPUT_RATE * d, g = gcd_u64(out, n);
    const uint64_t l = out / g, m = n / g;
    if (l > NVX_NB_MAX_PHASES) { *why = "the rate needs more than 1024 phases (L / M = 252000 / rate in lowest terms)"; return NVX_ERR_ARG; }
    /* Kaiser's estimate of the prototype's length at rate L * fi for a transition from fp to fi - fp */
    const double fi = (double)n / (double)d, fp = pass_edge(fi);
    const double fs = (double)l * fi;
    const double dw = 2.0 * M_PI * (fi - 2.0 * fp) / fs;
    const double order = (DESIGN_DB - 7.95) / (2.285 * dw);
    int t = (int)ceil((order + 1.0) / (double)l);
    if (t & 1) t++;
    if (t < 8) t = 8;
    if (t > NVX_NB_MAX_T) { *why = "the rate needs more than 32 taps per phase"; return NVX_ERR_ARG; }
    if ((long)l * t > NVX_NB_MAX_TAPS) { *why = "the rate needs more than 32768 taps (L * T)"; return NVX_ERR_ARG; }
    *L = (int)l; *M = (int)m; *T = t;
    return NVX_OK;
}

int nvx_nb_plan_taps(int L, int T, int16_t *taps, const char **why)
{
    const int nt = L * T;
    double *p = (double *)malloc((size_t)nt * sizeof(double));
    if (!p) { *why = "out of memory"; return NVX_ERR_NOMEM; }
    const double fc = 0.5 / (double)L;                          /* fi / 2 in cycles per sample of the prototype */
    const double beta = 0.1102 * (DESIGN_DB - 8.7);
    const double centre = 0.5 * (nt - 1), i0b = bessel_i0(beta);
    for (int k = 0; k < nt; k++) {
        const double d = k - centre, u = d / (centre + 0.5);     /* the window reaches zero half a sample beyond the ends */
        const double a = 2.0 * M_PI * fc * d;
        const double sinc = fabs(a) < 1e-12 ? 1.0 : sin(a) / a;
        p[k] = 2.0 * fc * sinc * bessel_i0(beta * sqrt(1.0 - u * u)) / i0b;
    }
    int rc = NVX_OK;
    for (int r = 0; r < L && rc == NVX_OK; r++) {
        double sum = 0.0;
        for (int t = 0; t < T; t++) sum += p[r + t * L];
        long isum = 0, asum = 0;
        int big = 0;
        for (int t = 0; t < T; t++) {
            long v = lrint(p[r + t * L] / sum * (double)(1 << NVX_NB_SHIFT));
            taps[r * T + t] = (int16_t)v;                        /* |v| <= about 2^14: a phase is at most a unit pulse */
            isum += v;
            if (labs(v) > labs((long)taps[r * T + big])) big = t;
        }
        /* the rounding residue onto the largest tap */
        const long fixed = (long)taps[r * T + big] + ((1L << NVX_NB_SHIFT) - isum);
        if (fixed > 32767 || fixed < -32768) { *why = "a tap leaves int16"; rc = NVX_ERR_ARG; break; }
        taps[r * T + big] = (int16_t)fixed;
        for (int t = 0; t < T; t++) asum += labs((long)taps[r * T + t]);
        if (asum > 65535) { *why = "a phase's absolute tap sum exceeds 65535: the accumulator could leave int32"; rc = NVX_ERR_ARG; }
    }
    free(p);
    return rc;
}
