/* nvx_align_find.c -- the row aligner's host-only parts (include/navtex_amd_align.h): the taps from the shared polyphase
 * design (csrc/nvx_polyphase_design.h) and the estimate of part 2, in integers throughout.  Pure C, no HIP. */
#include <stdlib.h>
#include <string.h>

#include "nvx_align_plan.h"
#include "nvx_polyphase_design.h"

typedef unsigned __int128 u128;

int nvx_align_design_taps(int16_t *taps)
{
    const int L = NVX_ALIGN_PHASES, T = NVX_ALIGN_TAPS;
    long long *row;
    /* cut-off at Nyquist of the rows' rate; the centre on a whole sample: index L * (T - 1 - G) */
    double *p = nvx_pp_prototype_at(0.5 / L, L, T, (double)(L * (T - 1 - NVX_ALIGN_GROUP_DELAY)), &row);
    if (!p) return NVX_ERR_NOMEM;
    for (int f = 0; f < L; f++) {
        int big;
        const long long sum = nvx_pp_phase(p, L, T, f, 14, row, &big);
        row[big] += (1 << 14) - sum;
        for (int k = 0; k < T; k++) taps[f * T + k] = (int16_t)row[T - 1 - k];
    }
    free(p);
    return NVX_OK;
}

NVX_API int nvx_align_taps(int16_t *taps)
{
    return taps ? nvx_align_design_taps(taps) : NVX_ERR_ARG;
}

NVX_API int nvx_align_delay(void) { return NVX_ALIGN_GROUP_DELAY; }

NVX_API uint64_t nvx_align_window(size_t n_in, int lag_first, int n_lags)
{
    if (n_lags < 64 || n_lags > NVX_ALIGN_MAX_LAGS || (n_lags & 63) || n_in > NVX_ALIGN_MAX_IN) return 0;
    const int64_t lag_last = (int64_t)lag_first + n_lags - 1;
    const int64_t span = (lag_last > 0 ? lag_last : 0) - (lag_first < 0 ? (int64_t)lag_first : 0);
    if ((int64_t)n_in - span < NVX_ALIGN_MIN_WINDOW) return 0;
    return (uint64_t)((int64_t)n_in - span) & ~(uint64_t)255;
}

static int cmp_u64(const void *a, const void *b)
{
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : x > y;
}

static int bitlength(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

NVX_API int nvx_align_find(const int64_t *r, int lag_first, int n_lags, uint64_t n_window, int64_t saa, int64_t sbb, int min_contrast,
                           nvx_align_estimate *out)
{
    const int T = NVX_ALIGN_TAPS, G = NVX_ALIGN_GROUP_DELAY, MARGIN = NVX_ALIGN_TAPS / 2 + 2;
    if (!r || !out || n_lags < 64 || n_lags > NVX_ALIGN_MAX_LAGS || (n_lags & 63) || min_contrast < 1 || min_contrast > (1 << 20) || saa < 0 || sbb < 0 ||
        n_window < NVX_ALIGN_MIN_WINDOW || n_window > NVX_ALIGN_MAX_IN || lag_first < -NVX_ALIGN_MAX_DELAY_LIMIT ||
        lag_first > NVX_ALIGN_MAX_DELAY_LIMIT)
        return NVX_ERR_ARG;
    uint64_t largest = 0;
    for (int i = 0; i < 2 * n_lags; i++) {
        if (r[i] == INT64_MIN) return NVX_ERR_ARG;
        const uint64_t m = (uint64_t)(r[i] < 0 ? -r[i] : r[i]);
        if (m > largest) largest = m;
    }
    memset(out, 0, sizeof *out);
    /* 1 */
    if ((uint64_t)saa < n_window || (uint64_t)sbb < n_window) { out->reason = 1; return NVX_OK; }
    /* 2 */
    const int bits = bitlength(largest), s = bits > 30 ? bits - 30 : 0;
    uint64_t *P = (uint64_t *)malloc((size_t)n_lags * sizeof *P);
    if (!P) return NVX_ERR_NOMEM;
    int c = 0;
    for (int i = 0; i < n_lags; i++) {
        const int64_t re = r[2 * i] >> s, im = r[2 * i + 1] >> s;
        P[i] = (uint64_t)(re * re) + (uint64_t)(im * im);
        if (P[i] > P[c]) c = i;
    }
    out->peak_lag = lag_first + c; out->peak_power = P[c];
    /* 3 */
    if (c < MARGIN || n_lags - 1 - c < MARGIN) { free(P); out->reason = 2; return NVX_OK; }
    /* 4 */
    const uint64_t peak = P[c];
    qsort(P, (size_t)n_lags, sizeof *P, cmp_u64);
    const uint64_t median = P[n_lags / 2];
    free(P);
    out->median_power = median;
    if ((u128)peak < (u128)median * (unsigned)min_contrast) { out->reason = 3; return NVX_OK; }
    /* 5 */
    int16_t taps[NVX_ALIGN_PHASES * NVX_ALIGN_TAPS];
    const int rc = nvx_align_design_taps(taps);
    if (rc != NVX_OK) return rc;
    u128 best = 0;
    int best_q5 = 0, have = 0;
    for (int L = c - 1; L <= c + 1; L++)
        for (int f = NVX_ALIGN_PHASES - 1; f >= 0; f--) {
            int64_t v_re = 0, v_im = 0;
            for (int k = 0; k < T; k++) {
                const int i = L + G - k;
                v_re += (int64_t)taps[f * T + k] * (r[2 * i] >> s);
                v_im += (int64_t)taps[f * T + k] * (r[2 * i + 1] >> s);
            }
            const u128 w = (u128)((__int128)v_re * v_re) + (u128)((__int128)v_im * v_im);
            if (!have || w > best) { best = w; best_q5 = 32 * (lag_first + L) - f; have = 1; }
        }
    out->delay_q5 = best_q5;
    /* 6 */
    const u128 den = ((u128)(uint64_t)saa * (uint64_t)sbb) >> (2 * s);
    if (den > 0 && den < ((u128)1 << 112)) {
        const u128 q = best / (den << 14);
        out->coherence_q14 = q > NVX_ALIGN_COHERENCE_ONE ? NVX_ALIGN_COHERENCE_ONE : (int32_t)q;
    }
    return NVX_OK;
}
