/* navtex_amd_align.h -- row aligner: two coherent rows of IQ (a main antenna and a sense antenna) that start an unknown number
 * of samples apart, at any rate and in any of the resampler's sample formats -> the same two rows as packed int16 IQ at the
 * same rate, a whole and a fractional number of samples moved so that they are sample-aligned.  The interface of the
 * companion library libnavtex_amd_align.so (none of the other libraries is needed to use it).
 *
 * Two dongles on one clock are coherent in frequency, but their streams start an arbitrary number of samples apart, often
 * thousands; USB buffering, decimator phases and cable lengths add a fraction.  The noise canceller (navtex_amd_anc.h) has
 * one complex weight per pair: half a sample of residue at 252 kS/s caps its null at -15 dB at +-14 kHz, and a hundred
 * samples decorrelate broadband noise altogether.  The aligner measures that delay and removes it.  It sits between the IQ
 * corrector and the canceller:
 *     IQ-correct (each row) -> align -> cancel -> blank -> notch -> DDC / resample -> scan -> tune -> decode
 * It has no notion of rate: everything below is in samples.  It has three parts: a measurement on the GPU
 * (nvx_align_measure_resident), an estimate on the host (nvx_align_find), and the streaming filter (nvx_align_set_delay,
 * nvx_align_resident, nvx_align_push).
 *
 * THE ARITHMETIC, operation by operation.  Integer arithmetic except the one float32 conversion of CF32 input and the design
 * of the taps (double, once, on the host); every shift and every division below is a floor shift or floor division of
 * signed integers.  The GPU results equal a restatement of this text word for word (==, no tolerance), whatever way the
 * input is cut into calls.
 *
 * Conversion.  Exactly as in navtex_amd_iqc.h, per component, to an integer in the int16 range:
 *   NVX_ALIGN_CS16   int16:    the value itself
 *   NVX_ALIGN_CU8    uint8 u:  (2 u - 255) * 128
 *   NVX_ALIGN_CS8    int8 s:   s * 256
 *   NVX_ALIGN_CF32   float f:  y = f * 32768 in float32, rounded to the nearest integer with ties to even, clamped to
 *                              [-32768, 32767]; NaN -> 0
 *   a[n] = (I1, Q1) is the main row, b[n] = (I2, Q2) the sense row.  Samples are interleaved I, Q in every format.
 *
 * 1. MEASURE (nvx_align_measure_resident; stateless, a calibration call like the scan's).
 *   Every converted component x is reduced to m = x >> 4, in -2048 .. 2047.  For lags l = lag_first .. lag_last =
 *   lag_first + n_lags - 1 (n_lags a multiple of 64, at most NVX_ALIGN_MAX_LAGS; |lag_first|, |lag_last| <= max_delay):
 *     n0 = max(0, -lag_first),  N = n_in - (max(0, lag_last) - min(0, lag_first)) rounded down to a multiple of 256
 *     (N >= 1024, NVX_ERR_ARG otherwise; N < 2^30)
 *     R_re[l] = sum (mI1[n] mI2[n + l] + mQ1[n] mQ2[n + l])      R_im[l] = sum (mQ1[n] mI2[n + l] - mI1[n] mQ2[n + l])
 *     SAA = sum (mI1[n]^2 + mQ1[n]^2)                            SBB = sum (mI2[n + lag_first]^2 + mQ2[n + lag_first]^2)
 *   each over n = n0 .. n0 + N - 1, exact in int64 (a term is at most 2^23, a sum at most 2^53).  R[l] is sum a conj(b
 *   shifted by l): a sense row that lags the main row by d samples peaks at l = d.
 *
 * 2. FIND (nvx_align_find; host only, no device, integers throughout, __int128 where needed).  T = NVX_ALIGN_TAPS = 16,
 *   G = NVX_ALIGN_GROUP_DELAY = 7, h_f[k] the taps of part 3.
 *    1. if SAA < N or SBB < N: reason 1, a row is silent; everything else 0
 *    2. s = max(0, bitlength(largest |R_re[l]|, |R_im[l]|) - 30);  r = R >> s per component (|r| < 2^30);
 *       P[l] = r_re^2 + r_im^2;  the coarse peak c is the first l with the largest P.  peak_lag = c, peak_power = P[c].
 *    3. if c - lag_first < T/2 + 2 or lag_last - c < T/2 + 2: reason 2, the peak lies at an end of the table; the caller
 *       moves the window
 *    4. median_power = the entry n_lags / 2 of P sorted upwards.  If P[c] < min_contrast * median_power: reason 3, the rows
 *       share no broadband component.  (A carrier or a station the two rows share gives a flat |R| and ends here: a
 *       narrowband signal cannot define a delay.)
 *    5. for L = c - 1, c, c + 1 and f = 0 .. 31:  V = sum over k = 0 .. T - 1 of h_f[k] r[L + G - k] per component
 *       (|V| < 2^45), W = V_re^2 + V_im^2.  It is the correlation at lag L + G of the main row with the sense row as the
 *       filter of phase f would deliver it, so it peaks where the sense row's delay is L - f/32.  Of the 96 candidates the
 *       one with the largest W is taken, the first of equals in order of increasing delay (L upwards, f downwards).
 *       delay_q5 = 32 L - f.
 *    6. den = (SAA * SBB) >> 2 s;  coherence_q14 = den > 0 ? min(16384, floor(W / (den << 14))) : 0.  Reason 0.
 *   Accuracy (measured with the restatement on the CPU): common noise confined to 0.8 of the band, N = 65536,
 *   twelve true delays anywhere between -90 and 90 samples, on and off the grid: the estimate was at most 0.0174 sample off,
 *   and 1/32 sample (one grid step) is what tests/test_align.py holds it to.  Noise that fills the whole band is outside
 *   this statement: no interpolator is valid there, and errors up to 0.057 sample were seen in the same trials.
 *
 * 3. APPLY (nvx_align_resident, nvx_align_push).  Per pair, d = delay_q5 (|d| <= 32 max_delay; 0 after create):
 *     d >= 0 (the sense row lags):  Dm = ceil(d / 32), Ds = 0, f = 32 Dm - d     the main row waits for the sense row
 *     d <  0 (the main row lags):   Dm = 0, Ds = |d| >> 5, f = |d| & 31
 *     out_main[n]  = a[n - G - Dm]                                               (the conversion word for word, moved)
 *     out_sense[n] = clamp16((sum over k = 0 .. T - 1 of h_f[k] b[n - Ds - k] + 8192) >> 14) per component
 *   so the main row is delayed by G + Dm and the sense row by G + Ds + f/32.  Samples in front of the pair's reset count as
 *   zero.  Phase 0 is the unit tap 2^14 at k = G, so a sense row whose delay is a whole number is the conversion word for
 *   word, moved, as well.  nvx_align_delay() returns G.  Words are (I & 0xffff) | (Q << 16).
 *   Taps.  32 phases of T = 16 taps from the rate changers' Kaiser prototype (90 dB window), cut-off at Nyquist, centred on
 *   a whole sample: h_f[k] = p[(T - 1 - k) * 32 + f] with the prototype's centre at index 32 * 8, each phase normalised to
 *   sum 1, rounded to int16 at 2^14, the rounding residue added to the phase's largest tap: every phase sums to exactly
 *   2^14 and delays by G + f/32 at DC to within 0.001 sample.  sum |h_f| <= 31 308 < 2 * 2^14, so the sum above stays inside int32.
 *   Computed from the shipped taps over |f| <= 0.3 of the rate: gain within +-0.0024 dB, delay within 0.0010 sample of
 *   G + f/32 (tests/test_align.py asserts +-0.01 dB and 1/64 sample).  nvx_align_taps() delivers them.
 *   A pair's output does not depend on how its input was cut into calls, calls of 0 and 1 samples included.
 * Carried state.  Per pair, in device memory, in two rows used alternately (a launch reads one and writes the other): the
 *   last max_delay + T converted samples of each row.  The 64-bit position and the delays live on the host: a delay set
 *   applies from the next call's first sample on, to the carried samples as well, and setting it does not wait for the GPU.
 *   Calls on one plan are ordered by the caller: successive calls go on the same hip_stream, or are synchronised by the caller.
 * Known limits.
 *   (a) A delay is one number per pair.  Delay spread (a path that differs with frequency) is not equalised.
 *   (b) The delay between free-running, non-coherent radios drifts, and nothing here tracks it: measure again.
 *   (c) A narrowband signal that the rows share cannot define a delay (reason 3).
 *   (d) Every call writes the carried samples anew: 8 bytes per pair and sample of max_delay.  Keep max_delay near the need.
 *
 * Errors.  Without a HIP device nvx_align_create returns NVX_ERR_NODEV; NULL or nonsense arguments, spans that leave their
 * allocation and an output that overlaps an input or the other output return NVX_ERR_ARG (checked before anything is
 * launched); nvx_align_last_error() has the sentence.
 */
#ifndef NAVTEX_AMD_ALIGN_H
#define NAVTEX_AMD_ALIGN_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_ALIGN_PHASES 32                  /* the grid of the fractional delay: 1/32 sample */
#define NVX_ALIGN_TAPS 16                    /* T */
#define NVX_ALIGN_GROUP_DELAY 7              /* G */
#define NVX_ALIGN_MAX_DELAY_DEFAULT 4096     /* samples */
#define NVX_ALIGN_MAX_DELAY_LIMIT 1048576    /* 2^20 */
#define NVX_ALIGN_MIN_CONTRAST_DEFAULT 64    /* the peak's power against the median's */
#define NVX_ALIGN_MAX_LAGS 8192
#define NVX_ALIGN_MIN_WINDOW 1024            /* the least N */
#define NVX_ALIGN_COHERENCE_ONE 16384        /* 1.0 in Q14 */

#define NVX_ALIGN_CS16 0                     /* int16 I, Q      (4 bytes per sample) */
#define NVX_ALIGN_CU8  1                     /* uint8 I, Q      (2 bytes per sample) */
#define NVX_ALIGN_CS8  2                     /* int8 I, Q       (2 bytes per sample) */
#define NVX_ALIGN_CF32 3                     /* float32 I, Q    (8 bytes per sample) */

typedef struct nvx_row_aligner nvx_row_aligner;

typedef struct nvx_align_config {
    uint32_t struct_size;       /* sizeof(nvx_align_config) of the caller's header: set by nvx_align_config_default */
    int device;                 /* 0 */
    int format;                 /* NVX_ALIGN_CS16, of both rows of nvx_align_resident and nvx_align_push */
    int n_pairs;                /* 1 */
    int max_delay;              /* 4096: the largest |delay| in samples, 1 .. 2^20 */
    int min_contrast;           /* 64: nvx_align_plan hands it back for nvx_align_find; 1 .. 2^20 */
} nvx_align_config;

/* What nvx_align_find returns. */
typedef struct nvx_align_estimate {
    int32_t delay_q5;           /* 1/32 sample; positive: the sense row lags the main row */
    int32_t reason;             /* 0: found; 1: a row is silent; 2: the peak lies at an end; 3: no contrast */
    int32_t coherence_q14;      /* step 6 */
    int32_t peak_lag;           /* the coarse peak c */
    uint64_t peak_power;        /* P[c] */
    uint64_t median_power;
} nvx_align_estimate;

NVX_API void nvx_align_config_default(nvx_align_config *cfg);
NVX_API int  nvx_align_create(const nvx_align_config *cfg, nvx_row_aligner **out);
NVX_API void nvx_align_destroy(nvx_row_aligner *al);

/* Part 1, over every pair of the plan: n_in samples (at most 2^30) of each row in `format` (one of NVX_ALIGN_*, the call's
 * own: the aligner's CS16 outputs can be measured to verify or refine a setting), in device memory as for nvx_align_resident.
 * r_out: host memory, [n_pairs][n_lags][2] int64 (R_re, R_im); power_out: host memory, [n_pairs][2] int64 (SAA, SBB).
 * The work is ordered on hip_stream and waited for.  It neither reads nor changes a pair's carried state. */
NVX_API int nvx_align_measure_resident(nvx_row_aligner *al, int format, const void *d_main, size_t pitch_main_samples, const void *d_sense,
                                       size_t pitch_sense_samples, size_t n_in, int lag_first, int n_lags, int64_t *r_out, int64_t *power_out,
                                       void *hip_stream);
/* The window's length N of such a call, or 0 where it is refused. */
NVX_API uint64_t nvx_align_window(size_t n_in, int lag_first, int n_lags);
/* Part 2, on one pair's table r[n_lags][2] with its SAA and SBB and the window's length N.  Needs no device and no plan. */
NVX_API int nvx_align_find(const int64_t *r, int lag_first, int n_lags, uint64_t n_window, int64_t saa, int64_t sbb, int min_contrast,
                           nvx_align_estimate *out);
/* The delay of `pair` (-1: every pair) from the next call's first sample on: |delay_q5| <= 32 max_delay. */
NVX_API int nvx_align_set_delay(nvx_row_aligner *al, int pair, int delay_q5);
NVX_API int nvx_align_get_delay(nvx_row_aligner *al, int pair, int *delay_q5);

/* Part 3, every pair of the plan, n_in samples each (at most 2^30).  d_main: [n_pairs][pitch_main_samples] samples in the
 * plan's format in device memory, 16-byte aligned, every row 16-byte aligned (pitch_main_samples times the sample size a
 * multiple of 16 where n_pairs > 1); d_sense with pitch_sense_samples likewise.  The n_in words of every pair's main row are
 * written to d_out_main[pair * pitch_out_main_samples + out_first ...] and those of its sense row to d_out_sense likewise,
 * 4-byte aligned.  Where every row's first word of an output is 16-byte aligned its words are written with aligned 16-byte
 * non-temporal stores; otherwise the same words go out one by one, slower.  All pairs must stand at the same position
 * (NVX_ERR_STATE otherwise).  All four spans are computed without wrapping and held against the allocations they lie in, and
 * neither output span may overlap an input span or the other output's (NVX_ERR_ARG, no launch).  The work is ordered on
 * hip_stream (a hipStream_t; NULL = the null stream) and NOT waited for.  n_in = 0 is valid and launches nothing. */
NVX_API int nvx_align_resident(nvx_row_aligner *al, const void *d_main, size_t pitch_main_samples, const void *d_sense, size_t pitch_sense_samples,
                               size_t n_in, void *d_out_main, size_t pitch_out_main_samples, void *d_out_sense, size_t pitch_out_sense_samples,
                               size_t out_first, void *hip_stream);
/* One pair from host memory to host memory: n_in samples in the plan's format at `main_in` and at `sense_in`, n_in samples of
 * interleaved int16 (I, Q) to out_main and to out_sense.  Returns when done. */
NVX_API int nvx_align_push(nvx_row_aligner *al, int pair, const void *main_in, const void *sense_in, size_t n_in, int16_t *out_main,
                           int16_t *out_sense);

/* A pair (-1: every pair) starts anew: position 0, nothing in front of it.  Its delay stays.  Waits for the launches in flight. */
NVX_API int nvx_align_reset(nvx_row_aligner *al, int pair);
/* Samples consumed by `pair` since its reset. */
NVX_API int nvx_align_position(nvx_row_aligner *al, int pair, uint64_t *consumed);
/* The plan's own numbers (each pointer may be NULL). */
NVX_API int nvx_align_plan(nvx_row_aligner *al, int *format, int *n_pairs, int *max_delay, int *min_contrast);
/* G: by how many samples both rows leave later than they came, beyond the delay set. */
NVX_API int nvx_align_delay(void);
/* The shipped taps, h_f[k] at taps[f * NVX_ALIGN_TAPS + k]: 32 * 16 int16.  Needs no device. */
NVX_API int nvx_align_taps(int16_t *taps);

/* HIP-event time of the aligner's kernels, per call of nvx_align_resident, nvx_align_push or nvx_align_measure_resident,
 * while enabled (nvx_align_time_stats waits for the launches still in flight). */
NVX_API int nvx_align_timing(nvx_row_aligner *al, int enable);
NVX_API int nvx_align_time_stats(nvx_row_aligner *al, double *sum_ms, uint64_t *calls, int reset);
NVX_API const char *nvx_align_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
