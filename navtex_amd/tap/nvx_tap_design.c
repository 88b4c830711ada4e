/* nvx_tap_design.c -- the channel tap's plan on the host (include/navtex_amd_tap.h): L, M, T from the rate and kind, the
 * int32 taps of the Kaiser-windowed sinc at S = 21, and the grid rules of shift and pitch.  Plain C, no device.  The Kaiser,
 * sinc and rounding code is csrc/nvx_polyphase_design.h's, which the resampler and the narrowband interpolator compile too;
 * here are the ranges, the band edges, the bounds on a phase's sums and the two grids. */
#include "nvx_tap_plan.h"

#define PASS_HZ 25000.0                      /* nvx_set_carrier's range */
#define PASS_FRACTION 0.4                    /* of fo, where that is less: the interpolator's band */

static int rate_ok(uint32_t fo, int kind, const char **why)
{
    if (kind == NVX_TAP_IQ) {
        if (fo < NVX_TAP_MIN_RATE || fo > NVX_TAP_MAX_RATE) { *why = "the IQ output rate is outside 2000 .. 96000 S/s"; return 0; }
    } else if (kind == NVX_TAP_REAL) {
        if (fo < NVX_TAP_MIN_AUDIO_RATE || fo > NVX_TAP_MAX_AUDIO_RATE) { *why = "the audio output rate is outside 8000 .. 48000 S/s"; return 0; }
    } else { *why = "the kind is NVX_TAP_IQ or NVX_TAP_REAL"; return 0; }
    return 1;
}

/* pass and stop edge in Hz */
static void edges(uint32_t fo, int kind, double *fp, double *fs)
{
    if (kind == NVX_TAP_REAL) { *fp = NVX_TAP_AUDIO_PASS_HZ; *fs = NVX_TAP_AUDIO_STOP_HZ; return; }
    *fp = PASS_FRACTION * fo < PASS_HZ ? PASS_FRACTION * fo : PASS_HZ;
    *fs = (double)fo - *fp;
}

int nvx_tap_plan_numbers(uint32_t fo, int kind, int *L, int *M, int *T, const char **why)
{
    if (!rate_ok(fo, kind, why)) return NVX_ERR_ARG;
    const uint64_t g = nvx_pp_gcd(NVX_TAP_INPUT_RATE, fo);
    const uint64_t l = fo / g, m = NVX_TAP_INPUT_RATE / g;
    /* the prototype runs at rate L * 252000; the transition is from fp to fs */
    double fp, fs;
    edges(fo, kind, &fp, &fs);
    const double rate = (double)l * NVX_TAP_INPUT_RATE;
    const double per_phase = nvx_pp_kaiser_per_phase(fs - fp, rate, (double)l);
    if (per_phase * (double)l > 2.0 * NVX_TAP_MAX_TAPS) { *why = "the rate needs more than 32768 taps (L * T, L / M = rate / 252000 in lowest terms)"; return NVX_ERR_ARG; }
    const int t = nvx_pp_even_taps(per_phase);
    if ((long)l * t > NVX_TAP_MAX_TAPS) { *why = "the rate needs more than 32768 taps (L * T, L / M = rate / 252000 in lowest terms)"; return NVX_ERR_ARG; }
    *L = (int)l; *M = (int)m; *T = t;
    return NVX_OK;
}

int nvx_tap_plan_taps(uint32_t fo, int kind, int L, int T, int32_t *taps, const char **why)
{
    double fp, fs;
    edges(fo, kind, &fp, &fs);
    const double fc = 0.5 * (fp + fs) / ((double)L * NVX_TAP_INPUT_RATE);      /* the middle of the transition, in cycles per sample of the prototype */
    long long *row;
    double *p = nvx_pp_prototype(fc, L, T, &row);
    if (!p) { *why = "out of memory"; return NVX_ERR_NOMEM; }
    int rc = NVX_OK;
    for (int r = 0; r < L && rc == NVX_OK; r++) {
        int big;
        const long long isum = nvx_pp_phase(p, L, T, r, NVX_TAP_SHIFT, row, &big);
        long long asum = 0, hsum = 0;
        /* the rounding residue onto the largest tap */
        row[big] += (1LL << NVX_TAP_SHIFT) - isum;
        for (int t = 0; t < T; t++) {
            const long long v = taps[r * T + t] = (int32_t)row[t], hh = v >> 8;     /* |v| <= about 2^21; arithmetic: v = 256 hh + hl, hl in [0, 255] */
            asum += llabs(v); hsum += llabs(hh);
        }
        if (hsum > 65535) { *why = "a phase's Sum |h >> 8| exceeds 65535: the high half's sum could leave int32"; rc = NVX_ERR_ARG; }
        else if (asum >= (1LL << 24)) { *why = "a phase's absolute tap sum reaches 2^24"; rc = NVX_ERR_ARG; }
    }
    free(p);
    return rc;
}

/* rint(x n / d) with ties to even for a finite x with |x n / d| below 2^31 (n a power of two: x n is exact) */
static long rint_ratio(double x, double n, double d)
{
    const double num = x * n, half = d / 2.0;
    long k = lrint(num / d);
    const double rem = fma(-(double)k, d, num);                  /* exact: num and k d lie within a factor of two, or k = 0 */
    if (rem > half || (rem == half && (k & 1))) k++;
    else if (rem < -half || (rem == -half && (k & 1))) k--;
    return k;
}

int nvx_tap_shift_k(uint32_t fo, int kind, double hz, int *k_out, const char **why)
{
    if (!rate_ok(fo, kind, why)) return NVX_ERR_ARG;
    if (!isfinite(hz) || fabs(hz) > NVX_TAP_INPUT_RATE) { *why = "the shift is not a frequency inside the input's band"; return NVX_ERR_ARG; }
    const long k = rint_ratio(hz, NVX_TAP_GRID, NVX_TAP_INPUT_RATE);
    /* |k fi / N| <= 126000 - fp, in integers and in fifths of a hertz: 5 fp = min(125000, 2 fo), or 2000 for audio */
    const int64_t fp5 = kind == NVX_TAP_REAL ? 5 * NVX_TAP_AUDIO_PASS_HZ : (2 * (int64_t)fo < 125000 ? 2 * (int64_t)fo : 125000);
    const int64_t lim = (int64_t)NVX_TAP_GRID * (5 * (int64_t)(NVX_TAP_INPUT_RATE / 2) - fp5), mag = 5 * (int64_t)(k < 0 ? -k : k) * NVX_TAP_INPUT_RATE;
    if (mag > lim) { *why = "the tap's pass band must lie inside the input's band: |shift| <= 126000 Hz - pass edge"; return NVX_ERR_ARG; }
    *k_out = (int)k;
    return NVX_OK;
}

int nvx_tap_pitch_k(uint32_t fo, double pitch_hz, int *kp_out, const char **why)
{
    if (!rate_ok(fo, NVX_TAP_REAL, why)) return NVX_ERR_ARG;
    if (!isfinite(pitch_hz) || fabs(pitch_hz) > fo) { *why = "the pitch is not a frequency inside the audio band"; return NVX_ERR_ARG; }
    const long kp = rint_ratio(pitch_hz, NVX_TAP_GRID, (double)fo);
    /* 800 <= kp fo / N <= fo / 2 - 800 */
    const int64_t v = (int64_t)kp * fo;
    if (v < (int64_t)NVX_TAP_AUDIO_STOP_HZ * NVX_TAP_GRID || 2 * v > (int64_t)NVX_TAP_GRID * ((int64_t)fo - 2 * NVX_TAP_AUDIO_STOP_HZ)) {
        *why = "the pitch lies outside 800 Hz .. rate / 2 - 800 Hz: the audio would fold at 0 or at rate / 2";
        return NVX_ERR_ARG;
    }
    *kp_out = (int)kp;
    return NVX_OK;
}
