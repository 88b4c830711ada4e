/* navtex_amd_notch.h -- tone notch: rows of IQ at any rate and in any of the resampler's sample formats -> rows of packed
 * int16 IQ at the same rate, delayed by a fixed number of samples, with up to four steady carriers per row subtracted.  The
 * interface of the companion library libnavtex_amd_notch.so (none of the other libraries is needed to use it).
 *
 * A steady carrier inside a chain's passband -- a non-directional beacon between 490 and 526.5 kHz, a clock harmonic of the
 * receiver, a switching supply's line -- 20 dB above a weak station and a few hundred hertz from its tones captures the
 * discriminator.  The notch estimates each carrier's complex amplitude in a narrow band around a frequency the caller sets
 * and subtracts the carrier it rebuilds from that.  It is a fixed linear filter, not an adaptive one: no loop, no solved
 * weights.  Its place:
 *     IQ-correct -> cancel -> blank -> notch -> DDC / resample -> scan -> tune -> decode
 * and it is equally valid directly in front of a raw_rate = 0 handle.  It has no notion of rate: everything below is in
 * samples, and a frequency is the 32-bit phase step per sample, step * fs / 2^32.
 *
 * THE ARITHMETIC, operation by operation.  Integer arithmetic except the one float32 conversion of CF32 input; every shift
 * below is a floor shift of signed 64-bit integers.  The GPU result equals a restatement of this text word for word (==, no
 * tolerance), whatever way the input is cut into calls.
 *
 * Conversion.  Exactly as in navtex_amd_anc.h, per component, to an integer in the int16 range:
 *   NVX_NOTCH_CS16   int16:    the value itself
 *   NVX_NOTCH_CU8    uint8 u:  (2 u - 255) * 128
 *   NVX_NOTCH_CS8    int8 s:   s * 256
 *   NVX_NOTCH_CF32   float f:  y = f * 32768 in float32, rounded to the nearest integer with ties to even, clamped to
 *                              [-32768, 32767]; NaN -> 0
 *   x[n] = (I, Q) is sample n of a row; n is the row's absolute 64-bit index since its reset.  Interleaved I, Q.
 * Plan.        n_rows rows; K = n_notches = 1 .. 4 notches per row; width_log2 = r = 2 .. 6, R = 2^r blocks of
 *   G = NVX_NOTCH_BLOCK = 256 samples; one format.  Each (row, notch) has a 32-bit step and an enabled flag; after create
 *   the step is 0 and the notch is disabled.  Every notch of the plan is summed whether it is enabled or not; the flag
 *   decides only whether its carrier is subtracted, so a notch that is enabled later works at once.
 * NCO.         ph = (step * n) mod 2^32,  j = ph >> 20,  (c, s) = W[j]: the down-converter bank's table
 *   (navtex_amd_ddc.h: W[j] = (rint(32767 cos(2 pi j / 4096)), rint(32767 sin(2 pi j / 4096)))).
 * Mix down.    u[n] = (I c + Q s, Q c - I s), each component below 2^31 in magnitude.
 * Block sums.  B[b] is the exact int64 sum of u over block b = n div 256, by absolute index (at most 2^39 per component).
 *   Blocks in front of the row's reset, and in front of the notch's last set_freq, are zero; a block that a reset (where the
 *   tests put it: at any position) or a set_freq cuts into sums only the samples received behind the cut.
 * Smoothing.   M[b] = sum over k = -(R-1) .. R-1 of (R - |k|) B[b + k]   (components at most 2^(39 + 2r)).
 * Interpolation to the sample.  With q = n mod 256:  q < 128: lo = b - 1, f = q + 128;  else: lo = b, f = q - 128
 *   (that is lo = (n - 128) div 256, f = (n - 128) mod 256).   m = M[lo] (256 - f) + M[lo + 1] f   (at most 2^(47 + 2r)).
 * Amplitude in Q4.  sh = 27 + 2r:  a = (m + 2^(sh - 1)) >> sh per component (at most 2^20).
 * Mix up.      e = (a_re c - a_im s, a_re s + a_im c) in int64 (at most 2^36);
 *   E = sum over the row's enabled notches of (e + 2^18) >> 19 per component;
 *   y[n] = clamp16(x[n] - E) per component;  y[n] = (0, 0) for n in front of the row's reset position.
 * Delay.       Sample n needs block b(n) + R complete, so the library has the fixed delay D = (R + 1) * 256 samples: a call of
 *   n_in samples writes n_in words, word n of the row is y[n - D] (I in the low half), and it is (0, 0) while n < D.  With no
 *   notch enabled the output is the conversion delayed by D, word for word.  nvx_notch_delay() returns D.
 * Cutting.     A row's output does not depend on how its input is cut into calls.
 * Setting a frequency.  set_freq, enable and disable apply from the next call's first sample: the words that call writes,
 *   the D pending ones included, are computed with the new step and flags.  set_freq zeroes that notch's block sums (ring
 *   and open block), as if the earlier blocks had been silent: the notch ramps in over 2R blocks.
 * Offset readout.  M'[b] = M[b] >> (2r + 15) per component (at most 2^24).  When block b + R - 1 is complete the notch adds
 *   X += M'[b] conj(M'[b - 1]) in int64, provided all 2R blocks b - R .. b + R - 1 lie wholly behind the last restart (their
 *   first sample at or behind it) and fewer than NVX_NOTCH_MAX_PAIRS = 4096 pairs were added since; then X stands.
 *   Restarts: reset, set_freq, nvx_notch_measure; each applies from the next call's first sample.
 *   offset_hz = arg(X) * fs / (2 pi 256): what the carrier lies above the notch, unambiguous to +-fs / 512.
 *   nvx_notch_refine applies set_freq(step + round(arg(X) * 2^32 / (2 pi 256))) in host double arithmetic.
 *   X is computed on the GPU; nothing but nvx_notch_get and nvx_notch_refine waits for the device.
 * Carried state.  Per row, in device memory, in two rows used alternately (a launch reads one and writes the other): the last
 *   D converted words (the delay line), the reset position, and per notch the last 2R + 2 block sums, the open block's
 *   partial sums, X, its pair count and the first block behind the last restart.  The 64-bit position, the steps and the
 *   flags live on the host and reach the device in front of the next call, on its stream.  Calls on one plan are ordered by
 *   the caller: successive calls go on the same hip_stream, or are synchronised by the caller.
 * Known limits.
 *   (a) It removes a carrier, not its modulation: a beacon's keyed ident sidebands at +-400 / +-1020 Hz stay.
 *   (b) The frequency must be right to about 1 Hz at R = 32 and 252 kS/s (DESIGN 3.15 has the table); the scan gives 5 Hz.
 *       Hence nvx_notch_refine.
 *   (c) Two notches closer than about fs / (256 R) each take the same carrier and over-subtract.  Set one.
 *   (d) A notch on one of the station's own tones removes the station.
 *   (e) The 12-bit table leaves a floor near -67 dB.
 * Cost.  The input is read twice and 4 bytes written per sample, like the IQ corrector, plus 2K table reads per sample.
 *
 * Errors.  Without a HIP device nvx_notch_create returns NVX_ERR_NODEV; NULL or nonsense arguments, spans that leave their
 * allocation and an output that overlaps the input return NVX_ERR_ARG (checked before anything is launched);
 * nvx_notch_last_error() has the sentence.
 */
#ifndef NAVTEX_AMD_NOTCH_H
#define NAVTEX_AMD_NOTCH_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_NOTCH_BLOCK 256                  /* samples per block */
#define NVX_NOTCH_MAX_NOTCHES 4              /* per row */
#define NVX_NOTCH_WIDTH_LOG2_MIN 2
#define NVX_NOTCH_WIDTH_LOG2_MAX 6
#define NVX_NOTCH_WIDTH_LOG2_DEFAULT 5       /* R = 32 blocks */
#define NVX_NOTCH_MAX_PAIRS 4096             /* of the offset readout */

#define NVX_NOTCH_CS16 0                     /* int16 I, Q      (4 bytes per sample) */
#define NVX_NOTCH_CU8  1                     /* uint8 I, Q      (2 bytes per sample) */
#define NVX_NOTCH_CS8  2                     /* int8 I, Q       (2 bytes per sample) */
#define NVX_NOTCH_CF32 3                     /* float32 I, Q    (8 bytes per sample) */

typedef struct nvx_tone_notch nvx_tone_notch;

typedef struct nvx_notch_config {
    uint32_t struct_size;       /* sizeof(nvx_notch_config) of the caller's header: set by nvx_notch_config_default */
    int device;                 /* 0 */
    int format;                 /* NVX_NOTCH_CS16 */
    int n_rows;                 /* 1 */
    int n_notches;              /* 1 */
    int width_log2;             /* 5 */
} nvx_notch_config;

/* What nvx_notch_get returns about one notch of one row. */
typedef struct nvx_notch_status {
    int64_t x_re, x_im;         /* X of the offset readout */
    uint64_t pairs;             /* added to X since the last restart: 0 .. NVX_NOTCH_MAX_PAIRS */
    uint64_t samples;           /* consumed by the row since creation */
    uint32_t step;
    int32_t enabled;
} nvx_notch_status;

NVX_API void nvx_notch_config_default(nvx_notch_config *cfg);
NVX_API int  nvx_notch_create(const nvx_notch_config *cfg, nvx_tone_notch **out);
NVX_API void nvx_notch_destroy(nvx_tone_notch *n);

/* Every row of the plan, n_in samples each (at most 2^30).  d_in: [n_rows][pitch_in_samples] samples in the plan's format in
 * device memory, 16-byte aligned, every row 16-byte aligned (pitch_in_samples times the sample size a multiple of 16 where
 * n_rows > 1).  The n_in words of every row are written (I in the low half) to d_out[row * pitch_out_samples + out_first ...],
 * 4-byte aligned.  Where every row's first word is 16-byte aligned (the address of d_out[out_first], and with more than one
 * row pitch_out_samples a multiple of 4) they are written with aligned 16-byte non-temporal stores; otherwise the same words
 * go out unaligned, slower.  All rows must stand at the same position (NVX_ERR_STATE otherwise).  Both spans are computed
 * without wrapping and held against the allocations they lie in before anything is launched, and the output span (from the
 * first word written to the last, the gaps between its rows included) must not overlap the input span (NVX_ERR_ARG, no
 * launch).  The work is ordered on hip_stream (a hipStream_t; NULL = the null stream) and NOT waited for.  n_in = 0 is valid
 * and launches nothing. */
NVX_API int nvx_notch_resident(nvx_tone_notch *n, const void *d_in, size_t pitch_in_samples, size_t n_in, void *d_out,
                               size_t pitch_out_samples, size_t out_first, void *hip_stream);
/* One row from host memory to host memory: n_in samples in the plan's format at `in`, n_in samples of interleaved int16
 * (I, Q) to out_iq.  Returns when done. */
NVX_API int nvx_notch_push(nvx_tone_notch *n, int row, const void *in, size_t n_in, int16_t *out_iq);

/* A row (-1: every row) starts anew from the next call on: position 0, every block sum zero, X and its count zero.  The
 * steps, the flags and the sample counters stay. */
NVX_API int nvx_notch_reset(nvx_tone_notch *n, int row);
/* The step of `notch` of `row` (-1: every row) from the next call's first sample on; its sums and its readout start anew. */
NVX_API int nvx_notch_set_freq(nvx_tone_notch *n, int row, int notch, uint32_t step);
/* enable != 0: the notch's carrier is subtracted from the next call's first sample on; 0: it is not.  The sums go on. */
NVX_API int nvx_notch_enable(nvx_tone_notch *n, int row, int notch, int enable);
/* The offset readout of the notch starts anew with the next call's first sample. */
NVX_API int nvx_notch_measure(nvx_tone_notch *n, int row, int notch);
/* set_freq to the step the readout points at; *new_step (may be NULL) is that step.  With X = 0 the step stays.  Waits for
 * the launches still in flight, as nvx_notch_get does. */
NVX_API int nvx_notch_refine(nvx_tone_notch *n, int row, int notch, uint32_t *new_step);
NVX_API int nvx_notch_get(nvx_tone_notch *n, int row, int notch, nvx_notch_status *out);
/* Samples consumed by `row` since its reset. */
NVX_API int nvx_notch_position(nvx_tone_notch *n, int row, uint64_t *consumed);
/* The plan's own numbers (each pointer may be NULL). */
NVX_API int nvx_notch_plan(nvx_tone_notch *n, int *format, int *n_rows, int *n_notches, int *width_log2);
/* D = (R + 1) * 256, in samples; negative: an error code. */
NVX_API int64_t nvx_notch_delay(nvx_tone_notch *n);

/* rint(hz / rate * 2^32) mod 2^32 (a negative frequency wraps), and back: the step as a signed number times rate / 2^32. */
NVX_API uint32_t nvx_notch_step_from_hz(double hz, double rate);
NVX_API double nvx_notch_hz_from_step(uint32_t step, double rate);

/* HIP-event time of the notch's kernels, per call, while enabled (nvx_notch_time_stats waits for the launches still in
 * flight). */
NVX_API int nvx_notch_timing(nvx_tone_notch *n, int enable);
NVX_API int nvx_notch_time_stats(nvx_tone_notch *n, double *sum_ms, uint64_t *calls, int reset);
NVX_API const char *nvx_notch_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
