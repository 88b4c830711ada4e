// nvx_afc_law.h -- the AFC law of include/navtex_amd_afc.h, once: the update kernel (navtex_amd/afc/nvx_afc.hip), its
// host twin nvx_afc_step_host (nvx_afc.cpp) and a plain C++ build (tests/harness/afc_law_corners.cpp) all compile this.
// Every fp64 operation below is a statement's only one or is rounded on its own (-ffp-contract=off; g++ on x86-64
// contracts nothing by itself); rint rounds ties to even in the default rounding mode, on the device as on the host.
#ifndef NVX_AFC_LAW_H
#define NVX_AFC_LAW_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NVX_AFC_HD __host__ __device__
#else
#define NVX_AFC_HD
#endif

#define NVX_AFC_LAW_C 0x1.6eb167b830193p+4     /* = NVX_AFC_C of navtex_amd_afc.h */
#define NVX_AFC_K_MAX 8000                     /* NVX_TUNE_MAX_HZ / NVX_TUNE_STEP_HZ */

/* what a launch's note says about a slot (flag bits) */
#define NVX_AFC_F_TRACK   1u                   /* the slot tracks */
#define NVX_AFC_F_PART    2u                   /* its stream took part in the launch */
#define NVX_AFC_F_UPDATE  4u                   /* the gate passed and d was finite: K[L+2] = K[L+1] + d, clamped */
#define NVX_AFC_F_CLAMP   8u                   /* max_step or a range limit cut the step */

/* a slot's parameters on the device: 32 bytes */
typedef struct nvx_afc_par {
    int track;                 /* the slot tracks */
    int kc;                    /* centre */
    int gain_shift, max_step, range_k, min_samples;
    double contrast_min;
} nvx_afc_par;

/* a launch's note for a slot: 8 bytes */
typedef struct nvx_afc_note {
    int k;                     /* K[L]: the k the launch ran with */
    short step;                /* K[L+2] - K[L+1] */
    unsigned short flags;
} nvx_afc_note;

/* K[L+2] of a slot that tracks and took part in launch L, from its record of that launch, k0 = K[L] and k1 = K[L+1];
 * *flags receives NVX_AFC_F_UPDATE / NVX_AFC_F_CLAMP */
static inline NVX_AFC_HD int nvx_afc_step(const nvx_afc_par *p, int k0, int k1, unsigned samples, unsigned b_samples,
                                          double sum_dphi_b, double sum_dphi_y, double sum_mf_hi, double sum_mf_lo, unsigned *flags)
{
    *flags = 0;
    const unsigned nb = b_samples, ny = samples - b_samples;
    if ((long long)samples < (long long)p->min_samples) return k1;
    if (8ull * nb < samples || 8ull * ny < samples) return k1;
    const double mf_diff = sum_mf_hi - sum_mf_lo;
    const double mf_sum = sum_mf_hi + sum_mf_lo;
    const double mf_need = p->contrast_min * mf_sum;
    if (!(mf_diff >= mf_need)) return k1;
    const double mb = sum_dphi_b / (double)nb;
    const double my = sum_dphi_y / (double)ny;
    const double m2 = mb + my;
    const double e = m2 * NVX_AFC_LAW_C;
    const double r = e - (double)(k1 - k0);
    double d = rint(ldexp(r, -p->gain_shift));
    if (!(fabs(d) <= 1.7976931348623157e308)) return k1;       /* NaN or inf: hold */
    unsigned f = NVX_AFC_F_UPDATE;
    const double lim = (double)p->max_step;
    if (d > lim) { d = lim; f |= NVX_AFC_F_CLAMP; }
    if (d < -lim) { d = -lim; f |= NVX_AFC_F_CLAMP; }
    int k2 = k1 + (int)d;
    int lo = p->kc - p->range_k, hi = p->kc + p->range_k;
    if (lo < -NVX_AFC_K_MAX) lo = -NVX_AFC_K_MAX;
    if (hi > NVX_AFC_K_MAX) hi = NVX_AFC_K_MAX;
    if (k2 > hi) { k2 = hi; f |= NVX_AFC_F_CLAMP; }
    if (k2 < lo) { k2 = lo; f |= NVX_AFC_F_CLAMP; }
    *flags = f;
    return k2;
}

#endif
