/* nvx_resample_design.c -- the resampler's plan on the host (include/navtex_amd_resample.h): L, M, T from the rate, the
 * int16 taps of the Kaiser-windowed sinc, and the count rule.  Plain C, no device. */
#include <math.h>
#include <stdlib.h>

#include "nvx_resample_plan.h"

#define PASS_HZ 25000.0                      /* nvx_set_carrier's range */
#define DESIGN_DB 90.0

static uint32_t gcd_u32(uint32_t a, uint32_t b)
{
    while (b) { uint32_t t = a % b; a = b; b = t; }
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

int nvx_rs_plan_numbers(uint32_t fi, int *L, int *M, int *T, const char **why)
{
    if (fi < NVX_RS_MIN_RATE || fi > NVX_RS_MAX_RATE) { *why = "the input rate is outside 96000 .. 3200000 S/s"; return NVX_ERR_ARG; }
    const uint32_t g = gcd_u32(NVX_RS_OUTPUT_RATE, fi);
    const uint32_t l = NVX_RS_OUTPUT_RATE / g, m = fi / g;
    if (l > NVX_RS_MAX_PHASES) { *why = "the rate needs more than 1024 phases (L = 252000 / gcd(252000, rate))"; return NVX_ERR_ARG; }
    /* Kaiser's estimate of the prototype's length at rate L * fi for a transition from 25 kHz to min(fi, 252000) - 25000 */
    const double fs = (double)l * (double)fi;
    const double stop = (fi < NVX_RS_OUTPUT_RATE ? (double)fi : (double)NVX_RS_OUTPUT_RATE) - PASS_HZ;
    const double dw = 2.0 * M_PI * (stop - PASS_HZ) / fs;
    const double n = (DESIGN_DB - 7.95) / (2.285 * dw);
    int t = (int)ceil((n + 1.0) / (double)l);
    if (t & 1) t++;
    if (t < 8) t = 8;
    if ((long)l * t > NVX_RS_MAX_TAPS) { *why = "the rate needs more than 32768 taps (L * T)"; return NVX_ERR_ARG; }
    *L = (int)l; *M = (int)m; *T = t;
    return NVX_OK;
}

int nvx_rs_plan_taps(uint32_t fi, int L, int T, int16_t *taps, const char **why)
{
    const int nt = L * T;
    double *p = (double *)malloc((size_t)nt * sizeof(double));
    if (!p) { *why = "out of memory"; return NVX_ERR_NOMEM; }
    const double fs = (double)L * (double)fi;
    const double stop = (fi < NVX_RS_OUTPUT_RATE ? (double)fi : (double)NVX_RS_OUTPUT_RATE) - PASS_HZ;
    const double fc = 0.5 * (PASS_HZ + stop) / fs;              /* cut-off in cycles per sample of the prototype */
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
        int big = 0, second = -1;
        for (int t = 0; t < T; t++) {
            long v = lrint(p[r + t * L] / sum * (double)(1 << NVX_RS_SHIFT));
            if (v > 32767) v = 32767;                            /* a phase that is nearly a unit pulse (rates close to 252 kS/s) */
            taps[r * T + t] = (int16_t)v;
            isum += v;
            if (labs(v) > labs((long)taps[r * T + big])) big = t;
        }
        for (int t = 0; t < T; t++)
            if (t != big && (second < 0 || labs((long)taps[r * T + t]) > labs((long)taps[r * T + second]))) second = t;
        /* the rounding residue onto the largest tap, or, where that tap stands at the rail, onto the next one */
        long fixed = (long)taps[r * T + big] + ((1L << NVX_RS_SHIFT) - isum);
        if (fixed > 32767) { big = second; fixed = (long)taps[r * T + big] + ((1L << NVX_RS_SHIFT) - isum); }
        if (fixed > 32767 || fixed < -32768) { *why = "a tap leaves int16"; rc = NVX_ERR_ARG; break; }
        taps[r * T + big] = (int16_t)fixed;
        for (int t = 0; t < T; t++) asum += labs((long)taps[r * T + t]);
        if (asum > 65535) { *why = "a phase's absolute tap sum exceeds 65535: the accumulator could leave int32"; rc = NVX_ERR_ARG; }
    }
    free(p);
    return rc;
}

/* ceil(n * L / M) for n < 2^63 */
uint64_t nvx_rs_outputs_after(uint64_t n, int L, int M)
{
    const unsigned __int128 v = (unsigned __int128)n * (unsigned)L + (unsigned)(M - 1);
    return (uint64_t)(v / (unsigned)M);
}
