/* nvx_spec_find.c -- the spectrum monitor's finder (include/navtex_amd_spec.h, rules 1 to 7): a survey -> steady lines.
 * Host C, no device. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "navtex_amd_spec.h"

#define PI 3.14159265358979323846

NVX_API void nvx_spec_params_default(nvx_spec_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = (uint32_t)sizeof *p;
    p->guard_bins = 3; p->min_lines = 8;
    p->min_coherence = 0.95; p->min_score_db = 6.0;
}

static int cmp_double(const void *a, const void *b)
{
    const double x = *(const double *)a, y = *(const double *)b;
    return (x > y) - (x < y);
}

typedef struct { double power, coherence; int bin; } cand;
static int cmp_cand(const void *a, const void *b)
{
    const cand *x = (const cand *)a, *y = (const cand *)b;
    if (x->power != y->power) return x->power > y->power ? -1 : 1;
    return (x->bin > y->bin) - (x->bin < y->bin);
}

NVX_API int nvx_spec_find_lines(const double *power, const double *lag_re, const double *lag_im, int n_log2, int avg, uint64_t lines,
                                const nvx_spec_params *p, nvx_spec_hit *hits, int cap)
{
    nvx_spec_params d;
    int found = 0, kept = 0, n_cand = 0;
    if (!power || !lag_re || !lag_im || n_log2 < NVX_SPEC_LOG2_MIN || n_log2 > NVX_SPEC_LOG2_MAX || cap < 0 || (cap > 0 && !hits)) return NVX_ERR_ARG;
    if (!p) { nvx_spec_params_default(&d); p = &d; }
    if (p->struct_size != sizeof *p || p->guard_bins < 0 || p->min_lines < 0) return NVX_ERR_ARG;
    if (avg < 2 || lines < (uint64_t)p->min_lines) return NVX_ERR_ARG;                  /* rule 7 */
    const int n = 1 << n_log2;
    double *sorted = (double *)malloc((size_t)n * sizeof(double));
    cand *c = (cand *)malloc((size_t)n * sizeof(cand));
    int *keep = (int *)malloc((size_t)n * sizeof(int));
    if (!sorted || !c || !keep) { free(sorted); free(c); free(keep); return NVX_ERR_NOMEM; }
    memcpy(sorted, power, (size_t)n * sizeof(double));
    qsort(sorted, (size_t)n, sizeof(double), cmp_double);
    const double floor_p = sorted[n / 2];                                               /* rule 1 */
    const double least = floor_p * pow(10.0, p->min_score_db / 10.0);
    for (int i = 0; i < n; i++) {
        if (!(power[i] > 0.0) || !(power[i] >= least)) continue;
        const double g = sqrt(lag_re[i] * lag_re[i] + lag_im[i] * lag_im[i]) * (double)avg / ((double)(avg - 1) * power[i]);      /* rule 2 */
        if (!(g >= p->min_coherence)) continue;                                         /* rule 3 */
        c[n_cand].power = power[i]; c[n_cand].coherence = g; c[n_cand].bin = i;
        n_cand++;
    }
    qsort(c, (size_t)n_cand, sizeof(cand), cmp_cand);
    for (int j = 0; j < n_cand; j++) {
        const int i = c[j].bin;
        int near = 0;
        for (int q = 0; q < kept && !near; q++) {                                       /* rule 4 */
            const int dist = abs(i - keep[q]);
            near = (dist < n - dist ? dist : n - dist) <= p->guard_bins;
        }
        if (near) continue;
        keep[kept++] = i;
        if (found < cap) {
            const int k = i - n / 2;
            const double sign = (k & 1) ? -1.0 : 1.0;
            const double delta = atan2(lag_im[i] * sign, lag_re[i] * sign) / PI;        /* rule 5 */
            const double cycles = ((double)k + delta) / (double)n;
            nvx_spec_hit *h = &hits[found];
            h->cycles_per_sample = cycles;
            h->step = (uint32_t)(int64_t)llrint((cycles - floor(cycles)) * 4294967296.0);
            h->coherence = c[j].coherence;
            h->score_db = floor_p > 0.0 ? 10.0 * log10(c[j].power / floor_p) : HUGE_VAL;
            h->bin = i;
        }
        found++;
    }
    free(sorted); free(c); free(keep);
    return found;
}
