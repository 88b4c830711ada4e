/* navtex_amd_narrow.h -- narrowband interpolator: audio or low-rate IQ at 2 .. 96 kS/s in any of four formats -> packed int16
 * IQ at 252 kS/s.  The interface of the companion library libnavtex_amd_narrow.so (none of the other libraries is needed to
 * use it).
 *
 * The resampler (navtex_amd_resample.h) starts at 96 kS/s and the real-input converter (navtex_amd_real.h) halves a rate.
 * What most NAVTEX receivers deliver is narrower: the audio of an SSB receiver (one real channel at 8 .. 48 kS/s with the
 * tone pair around 1000 .. 1700 Hz), 12 kS/s IQ from network receivers, 48 kS/s sound-card IQ.  This library is the link in
 * front for those:
 *     audio / low-rate IQ -> (real ->) narrow -> scan -> tune -> decode
 *
 * THE ARITHMETIC, operation by operation.  Everything is integer arithmetic except the one float32 conversion of F32 / CF32
 * input.  The GPU result equals a restatement of this text word for word (==, no tolerance).
 *
 * Rate.   fi = rate_num / rate_den S/s with rate_den 1 or 2 (2: the output of the real-input converter fed an odd rate:
 *   11025 S/s real gives 5512.5 S/s IQ).  The fraction is reduced first; 2000 <= fi <= 96000.
 *   L / M = 252000 * rate_den / rate_num in lowest terms.
 * Kinds and conversion, per component, to an integer in the int16 range:
 *   NVX_NB_IQ     x[n] = (I, Q), interleaved, in the resampler's four formats (format = NVX_NB_S16 .. NVX_NB_F32 reads
 *                 CS16, CU8, CS8, CF32);
 *   NVX_NB_REAL   x[n] = (I, 0), one component per sample, in the real-input converter's four formats.  The Q half of every
 *                 output word is then exactly 0.
 *   int16:    the value itself
 *   uint8 u:  (2 u - 255) * 128
 *   int8 s:   s * 256
 *   float f:  y = f * 32768 in float32, rounded to the nearest integer with ties to even, clamped to [-32768, 32767];
 *             NaN -> 0
 * Filter.  A plan owns T taps per phase, int16 taps h[r][t], r = 0 .. L-1, t = 0 .. T-1, and S = 14.  With x[k] = 0 for
 *   k < 0 (k counts a stream's input samples since its reset), output n of the stream since its reset is
 *       pos = n * M;   q = pos div L;   r = pos mod L;
 *       acc = sum over t = 0 .. T-1 of h[r][t] * x[q - t]              (an exact 32-bit integer sum, per component)
 *       out = clamp16((acc + 2^13) >> 14)                              (arithmetic shift)
 *       word[n] = (out_I & 0xffff) | (out_Q << 16)
 *   The clamp is real: with Sum |h| about 37 900 a full-scale input matched in sign to the taps reaches about +-75 800.
 * Counts.  After a stream has consumed N input samples in total it has produced exactly ceil(N * L / M) outputs: every n
 *   with n * M < N * L.  A stream's output does not depend on how its input was cut into calls; calls of zero samples and
 *   of one sample count.
 * Taps.  Computed once per plan on the host (nvx_nb_design hands out the same numbers without a device), by the
 *   resampler's recipe.  Pass edge fp = min(25000, 0.4 fi), stop edge fi - fp, so the cut-off is fi / 2 at the prototype's
 *   rate L * fi.  Kaiser's estimate N of the order for 90 dB and that transition; T = ceil((N + 1) / L) rounded up to
 *   even, at least 8; beta = 0.1102 (90 - 8.7); the window reaches zero half a sample beyond the ends; prototype
 *   p[k] = h[k mod L][k div L]; each phase scaled to sum 2^S, rounded, the rounding residue put on the phase's largest tap.
 *   S = 14, not the resampler's 15: at S = 15 this design has Sum |h| about 75 800 per phase for every fi <= 62500 and the
 *   accumulator could leave int32; at S = 14 it is about 37 900.  The design refuses a phase with Sum |h| > 65535.  What
 *   holds for every supported rate, and is what callers and tests may rely on:
 *     every phase sums to exactly 2^14 (a constant input c comes out as c);
 *     sum over t of |h[r][t]| <= 65535 for every phase, so |acc| + 2^13 <= 65535 * 32768 + 2^13 < 2^31;   T is even;
 *     response of the prototype relative to DC: within +-0.1 dB for |f| <= fp and <= -76 dB for every |f| from fi - fp up
 *     to L * fi / 2.
 *   0.4 fi is also exactly the band the real-input converter keeps flat.
 * Supported.  2000 <= fi <= 96000, L <= 1024, L * T <= 32768; anything else is NVX_ERR_ARG at plan creation and from
 *   nvx_nb_design, with a sentence in nvx_nb_last_error().
 * Carried state.  Per stream the last T - 1 converted samples live in device memory, in two rows used alternately (a launch
 *   reads one and writes the other); the 64-bit positions live on the host.  Calls on one plan are ordered by the caller:
 *   successive calls go on the same hip_stream, or are synchronised by the caller.
 *
 * Errors.  Without a HIP device nvx_nb_create returns NVX_ERR_NODEV; NULL or nonsense arguments and spans that leave their
 * allocation return NVX_ERR_ARG (checked before anything is launched); nvx_nb_last_error() has the sentence.  nvx_nb_design
 * needs no device.
 */
#ifndef NAVTEX_AMD_NARROW_H
#define NAVTEX_AMD_NARROW_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_NB_OUTPUT_RATE 252000
#define NVX_NB_SHIFT 14                      /* S */
#define NVX_NB_MIN_RATE 2000
#define NVX_NB_MAX_RATE 96000
#define NVX_NB_MAX_PHASES 1024               /* L */
#define NVX_NB_MAX_TAPS 32768                /* L * T */

#define NVX_NB_S16 0                         /* int16      (IQ: 4 bytes per sample, REAL: 2) */
#define NVX_NB_U8  1                         /* uint8      (IQ: 2, REAL: 1) */
#define NVX_NB_S8  2                         /* int8       (IQ: 2, REAL: 1) */
#define NVX_NB_F32 3                         /* float32    (IQ: 8, REAL: 4) */

#define NVX_NB_IQ   0                        /* x[n] = (I, Q) */
#define NVX_NB_REAL 1                        /* x[n] = (I, 0) */

typedef struct nvx_nb_interpolator nvx_nb_interpolator;

typedef struct nvx_nb_config {
    uint32_t struct_size;       /* sizeof(nvx_nb_config) of the caller's header: set by nvx_nb_config_default */
    int device;                 /* 0 */
    int n_streams;              /* 1 (1 .. 65535) */
    uint32_t rate_num;          /* 12000 */
    uint32_t rate_den;          /* 1 (1 or 2) */
    int format;                 /* NVX_NB_S16 */
    int kind;                   /* NVX_NB_IQ */
} nvx_nb_config;

NVX_API void nvx_nb_config_default(nvx_nb_config *cfg);
NVX_API int  nvx_nb_create(const nvx_nb_config *cfg, nvx_nb_interpolator **out);
NVX_API void nvx_nb_destroy(nvx_nb_interpolator *c);

/* The plan's numbers and taps for rate_num / rate_den, without a device: *L, *M, *T (each may be NULL) and, where taps is not
 * NULL and cap is large enough, the L * T taps in phase-major order taps[r * T + t].  Returns L * T (the capacity needed;
 * with taps == NULL or cap < L * T no tap is written), or NVX_ERR_ARG for a rate outside the supported range. */
NVX_API int nvx_nb_design(uint32_t rate_num, uint32_t rate_den, int *L, int *M, int *T, int16_t *taps, int cap);

/* Every stream of the plan, n_in input samples each (at most 2^30).  d_in: [n_streams][pitch_in_samples] samples in the
 * plan's format and kind in device memory, 16-byte aligned, every row 16-byte aligned (pitch_in_samples times the sample
 * size a multiple of 16 where n_streams > 1).  The ceil((N + n_in) L / M) - ceil(N L / M) outputs of every stream (N: what
 * it had consumed) are written as packed words (I in the low half) to d_out[stream * pitch_out_samples + out_first ...],
 * 4-byte aligned; *n_out (may be NULL) receives their number.  A call whose outputs would reach 2^31 is NVX_ERR_ARG.  A row
 * whose first output word is 16-byte aligned takes aligned 16-byte stores; otherwise the same words go out unaligned.  All
 * streams must stand at the same position (NVX_ERR_STATE otherwise).  Both spans are computed without wrapping and held
 * against the allocations they lie in before anything is launched (NVX_ERR_ARG, no launch).  The work is ordered on
 * hip_stream (a hipStream_t; NULL = the null stream) and NOT waited for.  n_in = 0 is valid and launches nothing. */
NVX_API int nvx_nb_resident(nvx_nb_interpolator *c, const void *d_in, size_t pitch_in_samples, size_t n_in, void *d_out,
                            size_t pitch_out_samples, size_t out_first, size_t *n_out, void *hip_stream);
/* One stream from host memory to host memory: n_in samples in the plan's format and kind at `in`; the outputs as interleaved
 * int16 (I, Q) at out_iq, ready for nvx_push_iq; *n_out (may be NULL) their number.  cap_samples smaller than the number of
 * outputs: NVX_ERR_ARG, nothing consumed.  Returns when done. */
NVX_API int nvx_nb_push(nvx_nb_interpolator *c, int stream, const void *in, size_t n_in, int16_t *out_iq, size_t cap_samples,
                        size_t *n_out);

/* A stream (-1: every stream) starts anew: position 0, silence in front.  Waits for the launches still in flight. */
NVX_API int nvx_nb_reset(nvx_nb_interpolator *c, int stream);
/* Input samples consumed and outputs produced by `stream` since its reset (either pointer may be NULL).  *produced is
 * ceil(consumed L / M), exact while the stream has consumed fewer than 2^54 samples and its low 64 bits beyond. */
NVX_API int nvx_nb_position(nvx_nb_interpolator *c, int stream, uint64_t *consumed, uint64_t *produced);
/* The plan's own numbers (each pointer may be NULL). */
NVX_API int nvx_nb_plan(nvx_nb_interpolator *c, int *L, int *M, int *T, int *n_streams, int *format, int *kind);

/* HIP-event time of the interpolator's kernel, per call, while enabled (nvx_nb_time_stats waits for the launches still in
 * flight). */
NVX_API int nvx_nb_timing(nvx_nb_interpolator *c, int enable);
NVX_API int nvx_nb_time_stats(nvx_nb_interpolator *c, double *sum_ms, uint64_t *calls, int reset);
NVX_API const char *nvx_nb_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
