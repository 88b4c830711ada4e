/* nvx_scan_find.c -- the band scan's detector (include/navtex_amd_scan.h, rules 1 to 9): a power row -> FSK carriers.
 * Host C, no device.  Every sum runs in the order the header states, so a restatement reproduces it. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "navtex_amd_scan.h"

#define N NVX_SCAN_FFT

NVX_API void nvx_scan_params_default(nvx_scan_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = (uint32_t)sizeof *p;
    p->band_half = 5; p->floor_half = 32; p->guard_bins = 13; p->shadow_bins = 33;
    p->refine_half = 6; p->refine_iters = 4;
    p->min_score_db = 6.0; p->shadow_db = 25.0; p->max_offset_hz = 25000.0;
    p->dc_guard_hz = 60.0; p->dc_max_shift_hz = 120.0;
}

static inline int wrap(int i) { i %= N; return i < 0 ? i + N : i; }
static inline int circ_dist(int a, int b) { const int d = abs(a - b); return d < N - d ? d : N - d; }

static int cmp_double(const void *a, const void *b)
{
    const double x = *(const double *)a, y = *(const double *)b;
    return (x > y) - (x < y);
}

typedef struct { double score; int bin; } cand;
static int cmp_cand(const void *a, const void *b)
{
    const cand *x = (const cand *)a, *y = (const cand *)b;
    if (x->score != y->score) return x->score > y->score ? -1 : 1;
    return (x->bin > y->bin) - (x->bin < y->bin);
}

/* the vertex of the parabola through ln P at m - 1, m, m + 1, as a shift from m */
static double log_parabola(const double *P, int m)
{
    const double pa = P[wrap(m - 1)], pb = P[wrap(m)], pc = P[wrap(m + 1)];
    if (!(pa > 0.0) || !(pb > 0.0) || !(pc > 0.0)) return 0.0;
    const double a = log(pa), b = log(pb), c = log(pc);
    const double den = (a - 2.0 * b) + c;
    if (!(den < 0.0)) return 0.0;
    double d = (0.5 * (a - c)) / den;
    if (d > 1.0) d = 1.0;
    if (d < -1.0) d = -1.0;
    return d;
}

static int arg_max(const double *P, int lo, int hi)
{
    int m = lo;
    for (int i = lo + 1; i <= hi; i++)
        if (P[wrap(i)] > P[wrap(m)]) m = i;
    return m;
}

NVX_API int nvx_scan_find(const double *P, const nvx_scan_params *up, nvx_scan_hit *hits, int cap)
{
    nvx_scan_params p;
    nvx_scan_params_default(&p);
    if (up) {
        if (up->struct_size != sizeof p) return NVX_ERR_ARG;
        p = *up;
    }
    if (!P || cap < 0 || (cap > 0 && !hits)) return NVX_ERR_ARG;
    if (p.band_half < 0 || p.band_half > 64 || p.floor_half < 1 || p.floor_half > 512 || p.guard_bins < 0 || p.shadow_bins < 0 ||
        p.refine_half < 1 || p.refine_half > 64 || p.refine_iters < 0 || p.refine_iters > 64 ||
        !(p.min_score_db == p.min_score_db) || !(p.shadow_db == p.shadow_db) || !(p.max_offset_hz >= 0.0) ||
        !(p.dc_guard_hz == p.dc_guard_hz) || !(p.dc_max_shift_hz == p.dc_max_shift_hz))
        return NVX_ERR_ARG;
    for (int i = 0; i < N; i++)
        if (!(P[i] >= 0.0) || isinf(P[i])) return NVX_ERR_ARG;      /* a power row is finite and not negative */

    const int nf = 2 * p.floor_half + 1;
    double *B = (double *)malloc(sizeof(double) * N), *win = (double *)malloc(sizeof(double) * (size_t)nf);
    cand *cands = (cand *)malloc(sizeof(cand) * N);
    int *kept = (int *)malloc(sizeof(int) * N);
    int found = NVX_ERR_NOMEM;
    if (!B || !win || !cands || !kept) goto out;

    int n_cand = 0;
    for (int i = 0; i < N; i++) {
        double b = 0.0;
        for (int d = -p.band_half; d <= p.band_half; d++) b = b + P[wrap(i + d)];
        B[i] = b;
        for (int d = -p.floor_half; d <= p.floor_half; d++) win[d + p.floor_half] = P[wrap(i + d)];
        qsort(win, (size_t)nf, sizeof(double), cmp_double);
        const double F = (double)(2 * p.band_half + 1) * win[p.floor_half];
        if (!(F > 0.0) || !(b > 0.0)) continue;
        const double score = 10.0 * log10(b / F);
        if (score >= p.min_score_db) { cands[n_cand].score = score; cands[n_cand].bin = i; n_cand++; }
    }
    qsort(cands, (size_t)n_cand, sizeof(cand), cmp_cand);

    int n_kept = 0;
    found = 0;
    for (int c = 0; c < n_cand; c++) {
        const int bin = cands[c].bin;
        int skip = 0;
        for (int k = 0; k < n_kept && !skip; k++) skip = circ_dist(bin, kept[k]) <= p.guard_bins;
        if (skip) continue;
        int shadowed = 0;
        for (int k = 0; k < n_kept && !shadowed; k++)
            shadowed = circ_dist(bin, kept[k]) <= p.shadow_bins && 10.0 * log10(B[kept[k]] / B[bin]) > p.shadow_db;
        if (shadowed) continue;
        kept[n_kept++] = bin;

        int ctr = bin;
        for (int it = 0; it < p.refine_iters; it++) {
            double num = 0.0, den = 0.0;
            for (int d = -p.refine_half; d <= p.refine_half; d++) {
                const double v = P[wrap(ctr + d)];
                num = num + (double)d * v;
                den = den + v;
            }
            if (!(den > 0.0)) break;
            ctr = (int)floor(((double)ctr + num / den) + 0.5);
        }
        const int m_lo = arg_max(P, ctr - p.refine_half, ctr - 1), m_hi = arg_max(P, ctr + 1, ctr + p.refine_half);
        const double lo = (double)m_lo + log_parabola(P, m_lo), hi = (double)m_hi + log_parabola(P, m_hi);
        const double offset = (0.5 * (lo + hi) - (double)(N / 2)) * NVX_SCAN_BIN_HZ;
        const double shift = (hi - lo) * NVX_SCAN_BIN_HZ;
        if (fabs(offset) > p.max_offset_hz) continue;
        if (fabs(offset) <= p.dc_guard_hz && shift < p.dc_max_shift_hz) continue;       /* the input's DC offset */
        if (found < cap) {
            nvx_scan_hit *h = &hits[found];
            h->offset_hz = offset;
            h->score_db = cands[c].score;
            h->shift_hz = shift;
            h->band_power_db = 10.0 * log10(B[bin]);
            h->bin = bin;
        }
        found++;
    }
out:
    free(B); free(win); free(cands); free(kept);
    return found;
}
