/* navtex_amd_div.h -- diversity combiner: two coherent rows of IQ (two antennas whose fades fall at different times) at any
 * rate and in any of the resampler's sample formats -> per station (target) one row of packed int16 IQ at the same rate, the
 * weaker row turned onto the stronger one's phase, scaled and added to it.  The interface of the companion library
 * libnavtex_amd_div.so (none of the other libraries is needed to use it).
 *
 * On MF at night the sky wave and the ground wave of a station beat, and the station fades through nulls that last longer
 * than the 280 ms between the two transmissions of a SITOR-B character, which the soft DX/RX combining
 * (navtex_amd_soft.h) therefore cannot bridge.  A second antenna whose nulls fall elsewhere can.  Where the noise canceller
 * (navtex_amd_anc.h) subtracts what two rows share, the combiner adds it: it is the other mode of a two-tuner radio.  Per
 * target it measures, in a band fs/256 wide around the target's frequency, the 2 x 2 covariance of the two rows and applies
 * the principal eigenvector: the stronger row with the weight 1, the weaker one with a complex weight of magnitude <= 1.
 * The rows must be sample-aligned and coherent; the combiner sits behind everything that treats the two rows alike:
 *     IQ-correct (each row) -> align -> (blank / notch / DDC / resample, each row alike) -> combine -> scan -> tune -> decode
 * It has no notion of rate: everything below is in samples, and a frequency is a 32-bit phase step per sample.
 *
 * THE ARITHMETIC, operation by operation.  Integer arithmetic except the one float32 conversion of CF32 input; every shift
 * and every division below is a floor shift or floor division of signed 64-bit integers.  The GPU result equals a
 * restatement of this text word for word (==, no tolerance), whatever way the input is cut into calls.
 *
 * 1. Conversion.  Exactly as in navtex_amd_anc.h, per component, to an integer in the int16 range:
 *   NVX_DIV_CS16   int16:    the value itself
 *   NVX_DIV_CU8    uint8 u:  (2 u - 255) * 128
 *   NVX_DIV_CS8    int8 s:   s * 256
 *   NVX_DIV_CF32   float f:  y = f * 32768 in float32, rounded to the nearest integer with ties to even, clamped to
 *                            [-32768, 32767]; NaN -> 0
 *   One plan has one format for both rows.  a[n] is the main row, b[n] the second row; n is the absolute 64-bit index of a
 *   pair's sample since its reset.  Samples are interleaved I, Q in every format.
 * 2. NCO and mix-down.  Per target, as in navtex_amd_notch.h: ph = (step * n) mod 2^32, j = ph >> 20, (c, s) = W[j] of the
 *   down-converter bank's table of 4096 steps (W[j] = (rint(32767 cos(2 pi j / 4096)), rint(32767 sin(2 pi j / 4096)))).
 *   For each row, with (I, Q) the converted sample: u = (I c + Q s, Q c - I s); each component within 2^31.
 * 3. Block sums.  NVX_DIV_BLOCK = 256 samples by absolute index.  A[m] and B[m] are the exact int64 sums of u_a and u_b over
 *   block m (each component at most 2^39).  Reduced: A' = A >> 16, B' = B >> 16 per component (each at most 2^23).
 * 4. Cells.  NVX_DIV_CELL = 65536 samples by absolute index: 256 blocks.  A cell has four exact sums over its blocks,
 *   each at most 2^55:
 *     SAA = sum (A're^2 + A'im^2)                    SBB = sum (B're^2 + B'im^2)
 *     SRE = sum (A're B're + A'im B'im)              SIM = sum (A'im B're - A're B'im)
 *   SRE + j SIM = sum A' conj(B').
 * 5. Window.  W = 2^window_log2 cells (window_log2 = 0, 1, 2 or 4; default 2).  TAA, TBB, TRE, TIM are the sums over the last
 *   W complete cells, each at most 2^59.
 * 6. Solve.  In NVX_DIV_TRACK mode, at the first sample of every cell in front of which W cells are complete since the
 *   target's last restart (cell k with k >= F + W, F the target's first counted cell: see 8):
 *    1. if TAA + TBB < 1024: weight (0, 0), lead 0, coherence 0, reason 1: both rows are silent in the band
 *    2. sh = max(0, bitlength(max(TAA, TBB)) - 29);  taa, tbb, tre, tim = TAA >> sh, TBB >> sh, TRE >> sh, TIM >> sh
 *       (taa, tbb < 2^29; |tre|, |tim| <= 2^29)
 *    3. d = taa - tbb;  q = d^2 + 4 (tre^2 + tim^2), below 2^62
 *    4. r = floor(sqrt(q)) exactly: the largest integer whose square is at most q, found in integers
 *    5. lead = 0 if d >= 0, else 1;  den = r + |d|.  If den = 0: weight (0, 0), lead 0, coherence 0, reason 0
 *    6. w_re = floor((tre * 32768 + den) / (2 den));  w_im = floor((x * 32768 + den) / (2 den)) with x = tim for lead 0 and
 *       x = -tim for lead 1; each clamped to [-8192, 8192].  That is 2 sum A' conj(B') / den, or its conjugate, in Q13, rounded:
 *       the weaker branch's component of the principal eigenvector of the 2 x 2 in-band covariance where the stronger
 *       branch's is exactly 1 -- maximal-ratio combining for rows of equal noise.
 *    7. m = (taa * tbb) >> 14;  coherence = m > 0 ? min(16384, floor((tre^2 + tim^2) / m)) : 0  (Q14).  Reported only.
 *   A cell start with reason 0 counts as solved, any other as rejected.
 * 7. Apply.  The weak row is the second row for lead 0 and the main row for lead 1; (Iw, Qw) is the weak row's converted
 *   sample and (Is, Qs) the strong row's:
 *     p = w_re Iw - w_im Qw + 4096,   r' = w_re Qw + w_im Iw + 4096        (|p|, |r'| < 2^31 for |w_re|, |w_im| <= 32767)
 *     out[n] = (clamp16(Is + (p >> 13)) & 0xffff) | (clamp16(Qs + (r' >> 13)) << 16)
 *   The weight (0, 0) with lead 0 gives the main row's conversion word for word: the state after create, after a reset and
 *   until W cells are complete.
 * 8. Restarts.
 *   nvx_div_reset: the pair stands at position 0; for every target every sum is zero, the weight (0, 0) with lead 0, the
 *     coherence and the reason 0, F = 0.  The steps, the modes and the counters stay.
 *   nvx_div_set_freq at position p: the target's weight becomes (0, 0) with lead 0, its sums zero, its coherence and reason 0.
 *     Its first counted cell F is the first cell whose first sample is at or behind p: F = ceil(p / 65536).  Samples in front
 *     of that cell are not summed.  A weight set before it and not yet applied is dropped.
 *   NVX_DIV_HOLD keeps the weight while the sums go on.  nvx_div_set replaces lead and weight from the next call's first
 *     sample; in NVX_DIV_TRACK mode the next solve replaces them.
 * 9. Cutting.  A pair's output and status do not depend on how its input is cut into calls.  (A cell start is solved by the
 *   call that holds the cell's first sample, with the mode that call finds.)
 * 10. Carried state.  Per pair and target, in device memory, in two rows used alternately (a launch reads one and writes the
 *   other): the open block's partial A and B, the open cell's partial sums, the ring of the last W cell sums, the first
 *   counted cell, the cells complete saturated at W, lead, weight, coherence, mode and reason.  The 64-bit position, the
 *   steps, the modes and the pending sets and restarts live on the host and reach the device on the call's stream.  Calls on
 *   one plan are ordered by the caller: successive calls go on the same hip_stream, or are synchronised by the caller.
 *
 * Known limits.
 *   (a) It assumes equal noise on the two rows in the band.  A row with more noise is given too much weight.
 *   (b) Local noise that both rows share, and that is stronger than the station in the band, steers the weight onto the
 *       noise.  Cancel first (navtex_amd_anc.h, navtex_amd_wanc.h), or combine only where the noise is atmospheric.
 *   (c) The band is fs/256 wide (+-984 Hz to the first null at 252 kS/s): run it at the narrowest rate available.
 *   (d) The weight lags by about W/2 cells.  Fades faster than about 4 s per period (at 252 kS/s) want W <= 2: at 3 s per
 *       period W = 4 delivers nothing.
 *   (e) When the stronger branch changes, the output's phase steps once by the two paths' phase difference.
 *   (f) A sum of two full-scale rows clamps.
 * Cost.  Both rows are read twice and 4 bytes written per sample and target.
 *
 * Errors.  Without a HIP device nvx_div_create returns NVX_ERR_NODEV; NULL or nonsense arguments, spans that leave their
 * allocation and an output that overlaps an input return NVX_ERR_ARG (checked before anything is launched); pairs at unequal
 * positions return NVX_ERR_STATE; nvx_div_last_error() has the sentence.
 */
#ifndef NAVTEX_AMD_DIV_H
#define NAVTEX_AMD_DIV_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_DIV_BLOCK 256                    /* samples per block */
#define NVX_DIV_CELL 65536                   /* samples per cell */
#define NVX_DIV_MAX_TARGETS 4
#define NVX_DIV_WINDOW_LOG2_DEFAULT 2        /* W = 4 cells; 0, 1 and 4 are the other values */
#define NVX_DIV_W_ONE 8192                   /* 1.0 in Q13: the largest component a solve gives */
#define NVX_DIV_W_MAX 32767                  /* |w_re|, |w_im| of a set weight */
#define NVX_DIV_COHERENCE_ONE 16384          /* 1.0 in Q14 */

#define NVX_DIV_TRACK 0                      /* solve at every cell start once the window is full */
#define NVX_DIV_HOLD 1                       /* keep the weight; the sums go on */

#define NVX_DIV_CS16 0                       /* int16 I, Q      (4 bytes per sample) */
#define NVX_DIV_CU8  1                       /* uint8 I, Q      (2 bytes per sample) */
#define NVX_DIV_CS8  2                       /* int8 I, Q       (2 bytes per sample) */
#define NVX_DIV_CF32 3                       /* float32 I, Q    (8 bytes per sample) */

typedef struct nvx_diversity_combiner nvx_diversity_combiner;

typedef struct nvx_div_config {
    uint32_t struct_size;       /* sizeof(nvx_div_config) of the caller's header: set by nvx_div_config_default */
    int device;                 /* 0 */
    int format;                 /* NVX_DIV_CS16, of both rows */
    int n_pairs;                /* 1 */
    int n_targets;              /* 1 (1 .. NVX_DIV_MAX_TARGETS): output rows per pair; every target starts with step 0 */
    int window_log2;            /* 2 */
} nvx_div_config;

/* What nvx_div_get returns about one target of one pair. */
typedef struct nvx_div_status {
    int32_t lead;               /* 0: the main row is the strong one, 1: the second row */
    int32_t w_re, w_im;         /* the weak row's weight (Q13): that of the pair's last sample, or set or restarted since */
    int32_t mode;               /* NVX_DIV_TRACK or NVX_DIV_HOLD */
    int32_t last_reason;        /* of the last cell start solved or rejected since the restart: 0 or 1 */
    int32_t coherence_q14;      /* of that cell start: step 6.7 */
    int64_t sums[4];            /* TAA, TBB, TRE, TIM over the complete cells of the window */
    uint32_t step;              /* the target's phase step */
    uint32_t reserved;          /* 0 */
    uint64_t samples;           /* consumed by the pair since creation */
    uint64_t cells_solved;      /* cell starts with reason 0 since creation */
    uint64_t cells_rejected;    /* ... with another reason */
} nvx_div_status;

NVX_API void nvx_div_config_default(nvx_div_config *cfg);
NVX_API int  nvx_div_create(const nvx_div_config *cfg, nvx_diversity_combiner **out);
NVX_API void nvx_div_destroy(nvx_diversity_combiner *c);

/* Every pair of the plan, n_in samples each (at most 2^30).  d_main: [n_pairs][pitch_main_samples] samples in the plan's
 * format in device memory, 16-byte aligned, every row 16-byte aligned (pitch_main_samples times the sample size a multiple of
 * 16 where n_pairs > 1); d_second with pitch_second_samples likewise.  n_pairs * n_targets rows of n_in words are written (I
 * in the low half): row = pair * n_targets + target goes to d_out[row * pitch_out_samples + out_first ...], 4-byte aligned.
 * Where every row's first word is 16-byte aligned (the address of d_out[out_first], and with more than one row
 * pitch_out_samples a multiple of 4) they are written with aligned 16-byte non-temporal stores; otherwise the same words go
 * out unaligned, slower.  All pairs must stand at the same position (NVX_ERR_STATE otherwise).  All three spans are computed
 * without wrapping and held against the allocations they lie in before anything is launched, and the output span (from the
 * first word written to the last, the gaps between its rows included) must overlap neither input span (NVX_ERR_ARG, no
 * launch).  The work is ordered on hip_stream (a hipStream_t; NULL = the null stream) and NOT waited for.  n_in = 0 is valid
 * and launches nothing. */
NVX_API int nvx_div_resident(nvx_diversity_combiner *c, const void *d_main, size_t pitch_main_samples, const void *d_second,
                             size_t pitch_second_samples, size_t n_in, void *d_out, size_t pitch_out_samples, size_t out_first,
                             void *hip_stream);
/* One pair from host memory to host memory: n_in samples in the plan's format at `main_in` and at `second_in`; out_iq holds
 * n_targets rows of n_in interleaved int16 (I, Q), one row after another.  Returns when done. */
NVX_API int nvx_div_push(nvx_diversity_combiner *c, int pair, const void *main_in, const void *second_in, size_t n_in, int16_t *out_iq);

/* The phase step of `target` of `pair` (-1: every pair) from the next call's first sample on; the target starts anew there (8).
 * Waits for nothing, as the four calls below. */
NVX_API int nvx_div_set_freq(nvx_diversity_combiner *c, int pair, int target, uint32_t step);
/* Lead (0 or 1) and weight of `target` of `pair` (-1: every pair) from the next call's first sample on: w_re and w_im within
 * +-NVX_DIV_W_MAX.  In NVX_DIV_TRACK mode the next solve replaces them. */
NVX_API int nvx_div_set(nvx_diversity_combiner *c, int pair, int target, int lead, int w_re, int w_im);
/* NVX_DIV_TRACK or NVX_DIV_HOLD for `target` of `pair` (-1: every pair) from the next call's first sample on. */
NVX_API int nvx_div_set_mode(nvx_diversity_combiner *c, int pair, int target, int mode);
/* A pair (-1: every pair) starts anew (8). */
NVX_API int nvx_div_reset(nvx_diversity_combiner *c, int pair);
/* Waits for the launches still in flight. */
NVX_API int nvx_div_get(nvx_diversity_combiner *c, int pair, int target, nvx_div_status *out);
/* Samples consumed by `pair` since its reset. */
NVX_API int nvx_div_position(nvx_diversity_combiner *c, int pair, uint64_t *consumed);
/* The plan's own numbers (each pointer may be NULL). */
NVX_API int nvx_div_plan(nvx_diversity_combiner *c, int *format, int *n_pairs, int *n_targets, int *window_log2);

/* The notch's two formulas: the step nearest to hz at `rate` samples per second (negative frequencies wrap; 0 for a rate
 * that is not positive), and the frequency of a step read as a signed number. */
NVX_API uint32_t nvx_div_step_from_hz(double hz, double rate);
NVX_API double nvx_div_hz_from_step(uint32_t step, double rate);

/* HIP-event time of the combiner's three kernels, per call, while enabled (nvx_div_time_stats waits for the launches still
 * in flight). */
NVX_API int nvx_div_timing(nvx_diversity_combiner *c, int enable);
NVX_API int nvx_div_time_stats(nvx_diversity_combiner *c, double *sum_ms, uint64_t *calls, int reset);
NVX_API const char *nvx_div_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
