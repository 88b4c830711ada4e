/* nvx_resample_design.c -- the resampler's plan on the host (include/navtex_amd_resample.h): L, M, T from the rate, the
 * int16 taps of the Kaiser-windowed sinc, and the count rule.  Plain C, no device.  The Kaiser, sinc and rounding code is
 * csrc/nvx_polyphase_design.h's; here are the range, the band edges and the int16 rail. */
#include "nvx_polyphase_design.h"
#include "nvx_resample_plan.h"

#define PASS_HZ 25000.0                      /* nvx_set_carrier's range */

/* the stop edge: the transition runs from 25 kHz to min(fi, 252000) - 25000 */
static double stop_edge(uint32_t fi) { return (fi < NVX_RS_OUTPUT_RATE ? (double)fi : (double)NVX_RS_OUTPUT_RATE) - PASS_HZ; }

int nvx_rs_plan_numbers(uint32_t fi, int *L, int *M, int *T, const char **why)
{
    if (fi < NVX_RS_MIN_RATE || fi > NVX_RS_MAX_RATE) { *why = "the input rate is outside 96000 .. 3200000 S/s"; return NVX_ERR_ARG; }
    const uint32_t g = (uint32_t)nvx_pp_gcd(NVX_RS_OUTPUT_RATE, fi);
    const uint32_t l = NVX_RS_OUTPUT_RATE / g, m = fi / g;
    if (l > NVX_RS_MAX_PHASES) { *why = "the rate needs more than 1024 phases (L = 252000 / gcd(252000, rate))"; return NVX_ERR_ARG; }
    /* the prototype runs at rate L * fi */
    const double fs = (double)l * (double)fi;
    const int t = nvx_pp_even_taps(nvx_pp_kaiser_per_phase(stop_edge(fi) - PASS_HZ, fs, (double)l));
    if ((long)l * t > NVX_RS_MAX_TAPS) { *why = "the rate needs more than 32768 taps (L * T)"; return NVX_ERR_ARG; }
    *L = (int)l; *M = (int)m; *T = t;
    return NVX_OK;
}

int nvx_rs_plan_taps(uint32_t fi, int L, int T, int16_t *taps, const char **why)
{
    const double fs = (double)L * (double)fi;
    const double fc = 0.5 * (PASS_HZ + stop_edge(fi)) / fs;     /* cut-off in cycles per sample of the prototype */
    long long *row;
    double *p = nvx_pp_prototype(fc, L, T, &row);
    if (!p) { *why = "out of memory"; return NVX_ERR_NOMEM; }
    int rc = NVX_OK;
    for (int r = 0; r < L && rc == NVX_OK; r++) {
        int big, second = -1;
        long long isum = nvx_pp_phase(p, L, T, r, NVX_RS_SHIFT, row, &big), asum = 0;
        /* a phase that is nearly a unit pulse (rates close to 252 kS/s) stands at the rail: the sum and the largest entry
         * are those of the row as it is stored */
        big = 0;
        for (int t = 0; t < T; t++) {
            if (row[t] > 32767) { isum -= row[t] - 32767; row[t] = 32767; }
            taps[r * T + t] = (int16_t)row[t];
            if (llabs(row[t]) > llabs(row[big])) big = t;
        }
        for (int t = 0; t < T; t++)
            if (t != big && (second < 0 || llabs(row[t]) > llabs(row[second]))) second = t;
        /* the rounding residue onto the largest tap, or, where that tap stands at the rail, onto the next one */
        long long fixed = row[big] + ((1LL << NVX_RS_SHIFT) - isum);
        if (fixed > 32767) { big = second; fixed = row[big] + ((1LL << NVX_RS_SHIFT) - isum); }
        if (fixed > 32767 || fixed < -32768) { *why = "a tap leaves int16"; rc = NVX_ERR_ARG; break; }
        row[big] = fixed; taps[r * T + big] = (int16_t)fixed;
        for (int t = 0; t < T; t++) asum += llabs(row[t]);
        if (asum > 65535) { *why = "a phase's absolute tap sum exceeds 65535: the accumulator could leave int32"; rc = NVX_ERR_ARG; }
    }
    free(p);
    return rc;
}

uint64_t nvx_rs_outputs_after(uint64_t n, int L, int M) { return nvx_pp_outputs_after(n, L, M); }
