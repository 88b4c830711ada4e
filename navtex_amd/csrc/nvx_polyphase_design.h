/* nvx_polyphase_design.h -- the polyphase design the rate changers (the resampler and with it the down-converter bank, the
 * narrowband interpolator, the channel tap) share: L / M in lowest terms, Kaiser's tap count, the Kaiser-windowed sinc
 * prototype, a phase normalised and rounded at a shift, and the count rule ceil(n L / M).  Pure C, no HIP: each library's
 * nvx_*_design.c calls these with its own band edges, ranges, rails and sentences, and tests/harness/polyphase_design_core.c
 * walks the three designs without a device.  Internal, and all of it static: every library compiles its own copy. */
#ifndef NVX_POLYPHASE_DESIGN_H
#define NVX_POLYPHASE_DESIGN_H

#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define NVX_PP_DESIGN_DB 90.0               /* the stop band every design asks of its Kaiser window */
#define NVX_PP_PI 3.14159265358979323846

static inline uint64_t nvx_pp_gcd(uint64_t a, uint64_t b)
{
    while (b) { uint64_t t = a % b; a = b; b = t; }
    return a;
}

/* modified Bessel function I0 by its power series */
static inline double nvx_pp_bessel_i0(double x)
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

/* Kaiser's estimate of the prototype's length at `rate` for a transition `width_hz` wide, as taps per phase of l phases:
 * a whole number, still a double (the channel tap bounds it before it becomes an int) */
static inline double nvx_pp_kaiser_per_phase(double width_hz, double rate, double l)
{
    const double dw = 2.0 * NVX_PP_PI * width_hz / rate;
    const double order = (NVX_PP_DESIGN_DB - 7.95) / (2.285 * dw);
    return ceil((order + 1.0) / l);
}

/* ... made even and at least 8 */
static inline int nvx_pp_even_taps(double per_phase)
{
    int t = (int)per_phase;
    if (t & 1) t++;
    if (t < 8) t = 8;
    return t;
}

/* The prototype of L * T taps with its cut-off at fc cycles per sample, centred on index `centre`, and behind it the T-entry
 * row nvx_pp_phase fills: one allocation, the caller's to free; NULL where there is no memory.  The window is L * T wide
 * around the centre whatever the centre is: centred on the whole index L * T / 2 (the row aligner's) the prototype is that of
 * L * T + 1 taps whose last is zero, and phase 0 of a Nyquist cut-off is a unit tap. */
static inline double *nvx_pp_prototype_at(double fc, int L, int T, double centre, long long **row)
{
    const int nt = L * T;
    double *p = (double *)malloc((size_t)nt * sizeof(double) + (size_t)T * sizeof(long long));
    if (!p) return NULL;
    const double beta = 0.1102 * (NVX_PP_DESIGN_DB - 8.7);
    const double half = 0.5 * nt, i0b = nvx_pp_bessel_i0(beta);
    for (int k = 0; k < nt; k++) {
        const double d = k - centre, u = d / half;               /* the window reaches zero half the length from the centre */
        const double a = 2.0 * NVX_PP_PI * fc * d;
        const double sinc = fabs(a) < 1e-12 ? 1.0 : sin(a) / a;
        p[k] = 2.0 * fc * sinc * nvx_pp_bessel_i0(beta * sqrt(1.0 - u * u)) / i0b;
    }
    *row = (long long *)(p + nt);
    return p;
}

/* ... centred between its two middle taps: the rate changers' */
static inline double *nvx_pp_prototype(double fc, int L, int T, long long **row)
{
    return nvx_pp_prototype_at(fc, L, T, 0.5 * (L * T - 1), row);
}

/* Phase r of the prototype, normalised to sum 1 and rounded at `shift`, into row[0 .. T); returns the row's sum and leaves
 * in *big the index of its largest entry (the first of equals).  The rounding residue 2^shift - sum is the caller's to place. */
static inline long long nvx_pp_phase(const double *p, int L, int T, int r, int shift, long long *row, int *big)
{
    double sum = 0.0;
    long long isum = 0;
    int b = 0;
    for (int t = 0; t < T; t++) sum += p[r + t * L];
    for (int t = 0; t < T; t++) {
        const long long v = llrint(p[r + t * L] / sum * (double)(1 << shift));
        row[t] = v;
        isum += v;
        if (llabs(v) > llabs(row[b])) b = t;
    }
    *big = b;
    return isum;
}

/* ceil(n * L / M) for n < 2^63, in full and as its low 64 bits */
static inline unsigned __int128 nvx_pp_outputs_after_wide(uint64_t n, int L, int M)
{
    return ((unsigned __int128)n * (unsigned)L + (unsigned)(M - 1)) / (unsigned)M;
}
static inline uint64_t nvx_pp_outputs_after(uint64_t n, int L, int M) { return (uint64_t)nvx_pp_outputs_after_wide(n, L, M); }

#endif
