/* navtex_amd_spec.h -- spectrum monitor: rows of IQ at any rate and in any of the resampler's sample formats -> waterfall
 * lines of level words per row, and a survey per row from which a host function names the steady carriers in it.  The
 * interface of the companion library libnavtex_amd_spec.so (none of the other libraries is needed to use it).
 *
 * The tone notch (navtex_amd_notch.h) needs a frequency right to about 1 Hz; the band scan sees only FIR1's passband of a
 * 252 kS/s stream, in fixed bins, and takes an unmodulated carrier for a non-station.  This library is the observer in
 * between: an averaged, half-overlapped, Hann-windowed spectrum of the row as it is, at N = 256 .. 4096 bins, written out
 * line by line for a waterfall, and beside the powers the lag products of successive segments, whose phase gives a steady
 * line's frequency to a small fraction of a bin and whose size tells a steady carrier from noise and from a keyed tone.
 * Its place:
 *     IQ-correct -> cancel -> blank -> [spectrum -> find_lines ->] notch -> DDC / resample -> scan -> tune -> decode
 * It changes nothing in the row: it only looks.  Like the notch it has no notion of rate: everything below is in samples
 * and bins, and a frequency is in cycles per sample, or the 32-bit phase step per sample that nvx_notch_set_freq takes.
 *
 * THE ARITHMETIC, operation by operation.  All floating point is IEEE fp64, every product and every sum rounded on its own:
 * no fused multiply-add anywhere.  The GPU result equals a restatement of this text bit for bit (==, no tolerance), whatever
 * way the input is cut into calls.
 *
 * Conversion.  Exactly as in navtex_amd_anc.h, per component, to an integer in the int16 range:
 *   NVX_SPEC_CS16   int16:    the value itself
 *   NVX_SPEC_CU8    uint8 u:  (2 u - 255) * 128
 *   NVX_SPEC_CS8    int8 s:   s * 256
 *   NVX_SPEC_CF32   float f:  y = f * 32768 in float32, rounded to the nearest integer with ties to even, clamped to
 *                             [-32768, 32767]; NaN -> 0
 *   x[n] = (I, Q) is sample n of a row; n is the row's absolute 64-bit index since its reset.  Interleaved I, Q.
 * Plan.        n_rows rows; n_log2 = 8 .. 12, N = 2^n_log2 = 256 .. 4096 bins (default 11); H = N / 2; avg = A >= 1 segments
 *   per line with A * H <= NVX_SPEC_MAX_HOP = 65536 (default 8); one format.
 * Segment.     Segment s is samples s H .. s H + N - 1 of the row: successive segments overlap by half.
 * Window.      Hann from the twiddle table: w[n] = 0.5 - 0.5 * C_N[n] (the product is exact: one rounding);
 *   v[n] = (w[n] * I[n], w[n] * Q[n]).  C_N[j] = cos(2 pi j / N) and S_N[j] = sin(2 pi j / N) are the table of
 *   navtex_amd/spec/nvx_spec_table.h (4096 entries: first octant correctly rounded, the rest of the turn by exact swaps and
 *   sign flips) at stride 4096 / N; its even entries are the band scan's table (navtex_amd/scan/nvx_scan_table.h) bit for bit,
 *   so for N <= 2048 these are the scan's numbers at stride 2048 / N.
 * Transform.   N-point radix-2 decimation in time, the band scan's text with N in place of 2048: x = v in bit-reversed
 *   order, then stages len = 2, 4, .., N; for a = x[i], b = x[i + len/2], position j of i in its block of len,
 *   (wr, wi) = (C_N[j * N / len], -S_N[j * N / len]):
 *       t.re = b.re * wr - b.im * wi;   t.im = b.re * wi + b.im * wr;   x[i] = a + t;   x[i + len/2] = a - t.
 *   Z_s[k] = x[k] is bin k of segment s.
 * Per segment and bin.  Power p = re * re + im * im (two products, one sum).  Lag product, for every segment of a line but its
 *   first, with the segment before it in the same line, c = Z_s * conj(Z_(s-1)): with a = Z_s, b = Z_(s-1),
 *       c.re = a.re * b.re + a.im * b.im;   c.im = a.im * b.re - a.re * b.im   (two products and one sum or difference each).
 * Line.        Line l is segments l A .. l A + A - 1: it spans (A + 1) H samples from sample l A H on, and lines hop by A H.
 *   P_line[k] is the sum of its A values of p in ascending segment order, from 0.0; C_line[k] the sum of its A - 1 lag
 *   products likewise (0.0 where A = 1).  Lines are independent of each other given the samples, so one workgroup per
 *   (row, line) and an ordered fold give the bits a sequential walk gives (the band scan's two-level argument).
 * Level word.  What a waterfall shows: an exact integer function of the double.  With u the 64 bits of P_line[k]:
 *       L = clamp((u >> 44) - (991 << 8), 0, 65535)   as uint16,
 *   a piecewise-linear log2 in Q8 with its zero at 2^-32: the exponent and the top eight mantissa bits, monotone, never above
 *   the true logarithm and at most 0.26 dB below it (the chord's sag) plus 0.01 dB (the truncation).  P = 0 gives 0.  The
 *   largest P_line a plan can meet, A <= 2^9 segments of at most 2 (2^12 2^15)^2, is below 2^64: L <= (64 + 32) * 256 = 24576,
 *   so the upper clamp never acts.  Index i of an output line holds bin (i + N/2) mod N, i.e. the frequency (i - N/2) / N
 *   cycles per sample: the scan's order and sign convention.
 *   NVX_SPEC_LEVEL_DB(L) is the level in dB (10 log10 of P_line).
 * Survey.      What the finder reads.  Per row, in device memory: SP[k] and SC[k], the sums of P_line[k] and C_line[k] over
 *   the lines completed since the last restart, in ascending line order, from 0.0, and the number of those lines beside them.
 *   Restarts: create, nvx_spec_reset, nvx_spec_measure; each applies from the next call: a line counts if its first sample lies
 *   at or behind the restart's position (the next call's first sample).  nvx_spec_get returns the survey in the order of an
 *   output line: index i holds bin (i + N/2) mod N.
 * Cutting.     A row's lines, level words and survey do not depend on how its input is cut into calls.  The library carries
 *   the converted samples not yet consumed by a complete line -- fewer than (A + 1) H per row, in device memory, in a ring
 *   where sample n lies at word n mod (A + 1) H -- and a call completes the lines whose last sample it brings:
 *   lines(p) = 0 for p < (A + 1) H, else (p - (A + 1) H) div (A H) + 1, is how many are complete at position p.  Every row of
 *   a plan stands at the same position in nvx_spec_resident (NVX_ERR_STATE otherwise), so a call completes the same number
 *   of lines in every row.  Calls on one plan are ordered by the caller: successive calls go on the same hip_stream, or are
 *   synchronised by the caller.
 * Kernels.     nvx_spec_line<format, n_log2> (one workgroup of N / 4 threads per row and line: staging, conversion, window,
 *   transform, both sums in registers, level words, P_line and C_line to a scratch row), nvx_spec_fold (the scratch rows
 *   into the survey, ascending) and nvx_spec_carry<format> (the unconsumed tail into the ring).
 *
 * THE FINDER (host only): a survey -> steady lines.  With N bins, indices i as nvx_spec_get gives them, k = i - N/2 the signed
 * bin, A = avg:
 *  1. floor       F = the median of the N values SP[i]: the value at index N/2 of them sorted ascending;
 *  2. coherence   g[i] = sqrt(SC[i].re^2 + SC[i].im^2) * A / ((A - 1) * SP[i]); noise gives about 1/6 (Hann at half overlap), a
 *                 steady carrier about 1, a keyed tone less than 1; a bin whose SP is not positive is no candidate;
 *  3. candidates  SP[i] >= F * 10^(min_score_db / 10) and g[i] >= min_coherence, walked by descending SP, lower index first
 *                 on ties;
 *  4. a candidate within guard_bins (circular distance <=) of one kept before it is skipped;
 *  5. frequency of a kept bin: d = atan2(im', re') / pi with (re', im') = SC[i] * (-1)^k, in bins above the bin's centre and
 *                 unambiguous within +-1 bin (successive segments lie N/2 samples apart, so a line at k + d bins turns the
 *                 lag product by pi (k + d)); the line stands at (k + d) / N cycles per sample;
 *  6. hits are reported in the order kept, each with cycles_per_sample, step = rint(cycles * 2^32) mod 2^32 (what
 *                 nvx_notch_set_freq takes), coherence, score_db = 10 log10(SP[i] / F) and bin = i;
 *  7. A < 2, or fewer than min_lines lines, is NVX_ERR_ARG.
 * atan2, sqrt, log10 and pow are libm's: the finder is held to tolerances, not to bits.
 *
 * Known limits.
 *   (a) A carrier weaker than what else falls into its bin, such as a station's own spectrum, is not found.
 *   (b) A strong station's tones look steady when a segment is much shorter than a bit period.  Below about 20 ms per
 *       segment, decimate first with the zoom bank or the channel tap, then look.
 *   (c) The finder names steady lines, not what they are.  A notch on a station's tone still removes the station.
 *   (d) The level word is for display, not for arithmetic.
 *
 * Errors.  Without a HIP device nvx_spec_create returns NVX_ERR_NODEV; NULL or nonsense arguments, spans that leave their
 * allocation, an output that overlaps the input and a call that would complete more lines than line_cap return NVX_ERR_ARG
 * (checked before anything is launched); nvx_spec_last_error() has the sentence.  nvx_spec_find_lines needs no device.
 */
#ifndef NAVTEX_AMD_SPEC_H
#define NAVTEX_AMD_SPEC_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_SPEC_LOG2_MIN 8
#define NVX_SPEC_LOG2_MAX 12
#define NVX_SPEC_LOG2_DEFAULT 11             /* N = 2048 */
#define NVX_SPEC_AVG_DEFAULT 8
#define NVX_SPEC_MAX_HOP 65536               /* A * H at most */
#define NVX_SPEC_LEVEL_ZERO (991 << 8)       /* the level word's zero: 2^-32 */
/* the level word in dB: 10 log10(2) * (L / 256 - 32) */
#define NVX_SPEC_LEVEL_DB(L) (3.010299956639812 * ((double)(L) / 256.0 - 32.0))

#define NVX_SPEC_CS16 0                      /* int16 I, Q      (4 bytes per sample) */
#define NVX_SPEC_CU8  1                      /* uint8 I, Q      (2 bytes per sample) */
#define NVX_SPEC_CS8  2                      /* int8 I, Q       (2 bytes per sample) */
#define NVX_SPEC_CF32 3                      /* float32 I, Q    (8 bytes per sample) */

typedef struct nvx_spectrum nvx_spectrum;

typedef struct nvx_spec_config {
    uint32_t struct_size;       /* sizeof(nvx_spec_config) of the caller's header: set by nvx_spec_config_default */
    int device;                 /* 0 */
    int format;                 /* NVX_SPEC_CS16 */
    int n_rows;                 /* 1 */
    int n_log2;                 /* 11 */
    int avg;                    /* 8 */
} nvx_spec_config;

typedef struct nvx_spec_params {
    uint32_t struct_size;       /* sizeof(nvx_spec_params) of the caller's header: set by nvx_spec_params_default */
    int guard_bins;             /* 3 */
    int min_lines;              /* 8 */
    int reserved;               /* 0 */
    double min_coherence;       /* 0.95 */
    double min_score_db;        /* 6.0 */
} nvx_spec_params;

typedef struct nvx_spec_hit {
    double cycles_per_sample;   /* where the line stands: (k + d) / N, in [-1/2, 1/2] */
    double coherence;           /* g of its bin */
    double score_db;            /* 10 log10(SP / F) of its bin */
    uint32_t step;              /* rint(cycles_per_sample * 2^32) mod 2^32: what nvx_notch_set_freq takes */
    int bin;                    /* the bin's index i in the survey */
} nvx_spec_hit;

NVX_API void nvx_spec_config_default(nvx_spec_config *cfg);
NVX_API int  nvx_spec_create(const nvx_spec_config *cfg, nvx_spectrum **out);
NVX_API void nvx_spec_destroy(nvx_spectrum *s);

/* How many lines the next call of n_in samples completes in `row`; negative: an error code. */
NVX_API int64_t nvx_spec_lines_for(nvx_spectrum *s, int row, size_t n_in);

/* Every row of the plan, n_in samples each (at most 2^30).  d_in: [n_rows][pitch_in_samples] samples in the plan's format in
 * device memory, 16-byte aligned, every row 16-byte aligned (pitch_in_samples times the sample size a multiple of 16 where
 * n_rows > 1).  d_levels: [n_rows][line_cap][N] uint16 in device memory, 16-byte aligned: line j the call completes in a row
 * goes to that row's line j; NULL: survey only (line_cap is ignored).  Returns the number of lines written per row (with
 * d_levels = NULL: completed), or a negative error code.  A call that would complete more than line_cap lines is
 * NVX_ERR_ARG and launches nothing.  All rows must stand at the same position (NVX_ERR_STATE otherwise).  Both spans are
 * computed without wrapping and held against the allocations they lie in before anything is launched, and the whole of
 * d_levels must not overlap the input span (NVX_ERR_ARG, no launch).  The work is ordered on hip_stream (a hipStream_t;
 * NULL = the null stream) and NOT waited for.  n_in = 0 is valid and launches nothing. */
NVX_API int nvx_spec_resident(nvx_spectrum *s, const void *d_in, size_t pitch_in_samples, size_t n_in, void *d_levels,
                              size_t line_cap, void *hip_stream);
/* One row from host memory to host memory: n_in samples in the plan's format at `in`; the lines completed go to
 * levels[line_cap][N] (may be NULL: survey only).  Returns the number of lines when done. */
NVX_API int nvx_spec_push(nvx_spectrum *s, int row, const void *in, size_t n_in, uint16_t *levels, size_t line_cap);

/* A row (-1: every row) starts anew from the next call on: position 0, nothing carried, the survey empty. */
NVX_API int nvx_spec_reset(nvx_spectrum *s, int row);
/* The survey of a row (-1: every row) starts anew with the next call's first sample; the lines go on as they were. */
NVX_API int nvx_spec_measure(nvx_spectrum *s, int row);
/* The survey of `row`: power[N], lag_re[N], lag_im[N] (each may be NULL), index i holding bin (i + N/2) mod N, and the number
 * of lines in it.  The only call that waits for the device. */
NVX_API int nvx_spec_get(nvx_spectrum *s, int row, double *power, double *lag_re, double *lag_im, uint64_t *lines);
/* Samples consumed by `row` since its reset. */
NVX_API int nvx_spec_position(nvx_spectrum *s, int row, uint64_t *consumed);
/* The plan's own numbers (each pointer may be NULL). */
NVX_API int nvx_spec_plan(nvx_spectrum *s, int *format, int *n_rows, int *n_log2, int *avg);

NVX_API void nvx_spec_params_default(nvx_spec_params *p);
/* power, lag_re, lag_im: [2^n_log2] as nvx_spec_get gives them, `lines` its count, avg the plan's A; p may be NULL (the
 * defaults); at most cap hits are written.  Returns the number of hits found (which may exceed cap), or NVX_ERR_ARG. */
NVX_API int nvx_spec_find_lines(const double *power, const double *lag_re, const double *lag_im, int n_log2, int avg,
                                uint64_t lines, const nvx_spec_params *p, nvx_spec_hit *hits, int cap);

/* HIP-event time of the monitor's kernels, per call, while enabled (nvx_spec_time_stats waits for the launches still in
 * flight). */
NVX_API int nvx_spec_timing(nvx_spectrum *s, int enable);
NVX_API int nvx_spec_time_stats(nvx_spectrum *s, double *sum_ms, uint64_t *calls, int reset);
NVX_API const char *nvx_spec_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
