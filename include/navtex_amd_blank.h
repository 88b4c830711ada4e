/* navtex_amd_blank.h -- impulse noise blanker: IQ at any rate and in any of the resampler's sample formats -> packed int16
 * IQ at the same rate, with impulsive samples replaced by zero.
 * The interface of the companion library libnavtex_amd_blank.so (none of the other libraries is needed to use it).
 *
 * MF reception is dominated by impulsive interference: static crashes, switching supplies, electric fences -- bursts a
 * fraction of a millisecond long and tens of dB above everything else.  Every other stage here is linear and assumes
 * stationary noise; behind the narrow filters a 1 ms burst is a 10 ms pulse and can no longer be told from signal.  The
 * blanker sits at the wide rate, in front of the selectivity:
 *     blank -> a CS16 plan of nvx_resample_* or nvx_ddc_*, a raw_rate = 1 or raw_rate = 0 handle, or nvx_scan_*.
 * It has no notion of rate: everything below is in samples.
 *
 * THE ARITHMETIC, operation by operation.  Integer arithmetic except the one float32 conversion of CF32 input.  The GPU
 * result equals a restatement of this text word for word (==, no tolerance).
 *
 * Conversion.  Per component, to an integer in the int16 range, as the resampler converts (navtex_amd_resample.h):
 *   NVX_BLANK_CS16   int16:    the value itself
 *   NVX_BLANK_CU8    uint8 u:  (2 u - 255) * 128
 *   NVX_BLANK_CS8    int8 s:   s * 256
 *   NVX_BLANK_CF32   float f:  y = f * 32768 in float32, rounded to the nearest integer with ties to even, clamped to
 *                              [-32768, 32767]; NaN -> 0
 *   x[n] = (I, Q); n counts a stream's samples since its reset.  Samples are interleaved I, Q in every format.
 * Magnitude.   m[n] = |I| + |Q|, in 0 .. 65536.
 * Block sums.  Blocks of NVX_BLANK_BLOCK = 1024 samples by absolute index, b = n div 1024;  S[b] = sum of m over the block,
 *   at most 2^26.
 * Level.       For b >= 4:  ref = min(S[b-1], S[b-2], S[b-3], S[b-4]);
 *                           level(b) = max((thr_q8 * (ref >> 10)) >> 8, floor)       (the product is at most 2^28)
 *   For b < 4 nothing is detected.  The minimum of four block means keeps a burst from raising the level it is judged by;
 *   four loud blocks in a row do raise it, so a sustained strong signal is blanked for 4 blocks and then passed.
 * Detection.   d[n] = m[n] > level(n div 1024).
 * Hold.        Sample n is blanked if some j in [max(0, n - hold), n] has d[j].  There is no look-ahead: a guard in front of
 *   the detection would delay the output by the guard.  Out of scope.
 * Output.      out[n] = blanked ? 0 : (I & 0xffff) | (Q << 16).
 * Counters.    Per stream: samples, detections (sum of d) and blanked samples, exact integers (nvx_blank_stats).
 * Parameters.  They belong to the plan:
 *   thr_q8   256 .. 4096 (1.0 .. 16.0), default 1024 (4.0).  On the restatement with Gaussian noise 4.0 detects 2e-5 of the
 *            samples, 5.0 detects none in 4 M, and 3.0 detects 0.2 %.
 *            thr_q8 = 0 is the bypass: out is the conversion, nothing is detected or counted as blanked.
 *   hold     0 .. 1024, default 32
 *   floor    0 .. 65535, default 64
 * A stream's output does not depend on how its input was cut into calls.
 * Carried state.  Per stream, in device memory, in two rows used alternately (a launch reads one and writes the other): the
 *   last four complete block sums, the open block's partial sum, the distance to the last detection saturated at hold + 1.
 *   The 64-bit position lives on the host.  A reset zeroes all of it: nothing is detected until four blocks are complete
 *   again.  Calls on one plan are ordered by the caller: successive calls go on the same hip_stream, or are synchronised
 *   by the caller.
 * Cost.  A full extra pass over the input: per sample the format's bytes are read once and 4 bytes written (CS16: 8 bytes,
 *   CU8: 6).  It is an option for receivers that need it.
 *
 * Errors.  Without a HIP device nvx_blank_create returns NVX_ERR_NODEV; NULL or nonsense arguments and spans that leave
 * their allocation return NVX_ERR_ARG (checked before anything is launched); nvx_blank_last_error() has the sentence.
 */
#ifndef NAVTEX_AMD_BLANK_H
#define NAVTEX_AMD_BLANK_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_BLANK_BLOCK 1024                 /* NB: samples per block */
#define NVX_BLANK_THR_MIN 256                /* 1.0 */
#define NVX_BLANK_THR_MAX 4096               /* 16.0 */
#define NVX_BLANK_THR_DEFAULT 1024           /* 4.0 */
#define NVX_BLANK_HOLD_MAX 1024
#define NVX_BLANK_HOLD_DEFAULT 32
#define NVX_BLANK_FLOOR_MAX 65535
#define NVX_BLANK_FLOOR_DEFAULT 64

#define NVX_BLANK_CS16 0                     /* int16 I, Q      (4 bytes per sample) */
#define NVX_BLANK_CU8  1                     /* uint8 I, Q      (2 bytes per sample) */
#define NVX_BLANK_CS8  2                     /* int8 I, Q       (2 bytes per sample) */
#define NVX_BLANK_CF32 3                     /* float32 I, Q    (8 bytes per sample) */

typedef struct nvx_blanker nvx_blanker;

typedef struct nvx_blank_config {
    uint32_t struct_size;       /* sizeof(nvx_blank_config) of the caller's header: set by nvx_blank_config_default */
    int device;                 /* 0 */
    int format;                 /* NVX_BLANK_CS16 */
    int n_streams;              /* 1 */
    uint32_t thr_q8;            /* 1024 */
    uint32_t hold;              /* 32 */
    uint32_t floor;             /* 64 */
} nvx_blank_config;

NVX_API void nvx_blank_config_default(nvx_blank_config *cfg);
NVX_API int  nvx_blank_create(const nvx_blank_config *cfg, nvx_blanker **out);
NVX_API void nvx_blank_destroy(nvx_blanker *b);

/* Every stream of the plan, n_in samples each (at most 2^30).  d_in: [n_streams][pitch_in_samples] samples in the plan's
 * format in device memory, 16-byte aligned, every row 16-byte aligned (pitch_in_samples times the sample size a multiple of
 * 16 where n_streams > 1).  The n_in words of every stream are written (I in the low half) to
 * d_out[stream * pitch_out_samples + out_first ...], 4-byte aligned.  Where every row's first word is 16-byte aligned (the
 * address of d_out[out_first], and with more than one stream pitch_out_samples a multiple of 4) they are written with
 * aligned 16-byte stores; otherwise the same words go out unaligned, slower.  All streams must stand at the same position
 * (NVX_ERR_STATE otherwise).  Both spans are computed without wrapping and held against the allocations they lie in before
 * anything is launched (NVX_ERR_ARG, no launch).  The work is ordered on hip_stream (a hipStream_t; NULL = the null stream)
 * and NOT waited for.  n_in = 0 is valid and launches nothing. */
NVX_API int nvx_blank_resident(nvx_blanker *b, const void *d_in, size_t pitch_in_samples, size_t n_in, void *d_out,
                               size_t pitch_out_samples, size_t out_first, void *hip_stream);
/* One stream from host memory to host memory: n_in samples in the plan's format at `in`, n_in samples of interleaved int16
 * (I, Q) to out_iq.  Returns when done. */
NVX_API int nvx_blank_push(nvx_blanker *b, int stream, const void *in, size_t n_in, int16_t *out_iq);

/* A stream (-1: every stream) starts anew: position 0, nothing detected until four blocks are complete.  Its counters stay. */
NVX_API int nvx_blank_reset(nvx_blanker *b, int stream);
/* Samples consumed by `stream` since its reset. */
NVX_API int nvx_blank_position(nvx_blanker *b, int stream, uint64_t *consumed);
/* The counters of `stream` since creation or the last call with reset != 0 (any pointer may be NULL); waits for the
 * launches still in flight. */
NVX_API int nvx_blank_stats(nvx_blanker *b, int stream, uint64_t *samples, uint64_t *detections, uint64_t *blanked, int reset);
/* The plan's own numbers (each pointer may be NULL). */
NVX_API int nvx_blank_plan(nvx_blanker *b, int *format, int *n_streams, uint32_t *thr_q8, uint32_t *hold, uint32_t *floor);

/* HIP-event time of the blanker's kernel, per launch, while enabled (nvx_blank_time_stats waits for the launches still in
 * flight). */
NVX_API int nvx_blank_timing(nvx_blanker *b, int enable);
NVX_API int nvx_blank_time_stats(nvx_blanker *b, double *sum_ms, uint64_t *launches, int reset);
NVX_API const char *nvx_blank_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
