/* navtex_amd_resample.h -- resampler: IQ at another rate and in another sample format -> packed int16 IQ at 252 kS/s.
 * The interface of the companion library libnavtex_amd_resample.so (libnavtex_amd.so itself is not needed to use it).
 *
 * The library proper takes int16 IQ at exactly 2.016 MS/s or 252 kS/s.  Other radios and recordings deliver 2.048 / 2.4 /
 * 1.024 MS/s as unsigned bytes, 768 / 384 / 192 kS/s as int16, 250 / 256 kS/s, float32 files, 96 kS/s sound-card IQ.  The
 * resampler is the link in front:   resample -> nvx_push_iq / nvx_process_resident / nvx_scan_* of a raw_rate = 0 handle.
 *
 * THE ARITHMETIC, operation by operation.  Everything is integer arithmetic except the one float32 conversion of CF32
 * input.  The GPU result equals a restatement of this text word for word (==, no tolerance).
 *
 * Rates.  fi = input_rate_hz, g = gcd(252000, fi), L = 252000 / g, M = fi / g.
 * Input conversion, per component, to an integer x in the int16 range:
 *   NVX_RS_CS16   int16:    the value itself
 *   NVX_RS_CU8    uint8 u:  (2 u - 255) * 128          (the 127.5 offset of 8-bit dongles, exact)
 *   NVX_RS_CS8    int8 s:   s * 256
 *   NVX_RS_CF32   float f:  y = f * 32768 in float32 (exact, or +-inf), rounded to the nearest integer with ties to even,
 *                           clamped to [-32768, 32767]; NaN -> 0
 *   Samples are interleaved I, Q in every format (CS16: one packed 32-bit word as nvx_process_resident takes it).
 * Filter.  A plan owns T taps per phase, int16 taps h[r][t], r = 0 .. L-1, t = 0 .. T-1, and S = 15.  With x[k] = 0 for
 *   k < 0 (k counts a stream's input samples since its reset), output n of the stream since its reset is
 *       pos = n * M;   q = pos div L;   r = pos mod L;
 *       acc = sum over t = 0 .. T-1 of h[r][t] * x[q - t]              (an exact 32-bit integer sum)
 *       out[n] = clamp16((acc + 2^(S-1)) >> S)                         (arithmetic shift; I and Q alike)
 * Counts.  After a stream has consumed N input samples in total it has produced exactly ceil(N * L / M) outputs: every n
 *   with n * M < N * L.  A stream's output does not depend on how its input was cut into calls.  For fi a multiple of 25,
 *   fi * 8 / 25 input samples from a frame boundary give exactly one frame of 80640 outputs.
 * Taps.  Computed once per plan on the host (nvx_resample_design hands out the same numbers without a device): a
 *   Kaiser-windowed sinc designed for 90 dB, cut-off midway between 25 kHz and min(fi, 252000) - 25000 Hz, prototype
 *   p[k] = h[k mod L][k div L] at rate L * fi, each phase scaled to sum 2^S, rounded, and the rounding residue put on the
 *   phase's largest tap.  What holds for every supported rate, and is what callers and tests may rely on:
 *     every phase sums to exactly 2^S (a constant input c comes out as c; no spur at multiples of fi);
 *     sum over t of |h[r][t]| <= 65535 for every phase (acc cannot leave int32);   T is even;
 *     response of the prototype relative to DC: within +-0.1 dB for |f| <= 25 kHz (nvx_set_carrier's range), and
 *     <= -76 dB for every |f| from min(fi, 252000) - 25000 up to L * fi / 2.
 * Supported.  96000 <= fi <= 3200000, L <= 1024, L * T <= 32768; anything else is NVX_ERR_ARG at plan creation (and from
 *   nvx_resample_design), with a sentence in nvx_resample_last_error().  Above 3.2 MS/s int16 taps at S = 15 no longer
 *   reach 76 dB (10 MS/s: about -68 dB): out of scope -- decimate in the radio.
 * Carried state.  Per stream the last T-1 converted samples live in device memory, in two rows used alternately (a
 *   launch reads one and writes the other); the 64-bit counters live on the host.  Calls on one plan are ordered by
 *   the caller: successive calls go on the same hip_stream, or are synchronised by the caller.
 *
 * Errors.  Without a HIP device nvx_resample_create returns NVX_ERR_NODEV; NULL or nonsense arguments and spans that
 * leave their allocation return NVX_ERR_ARG (checked before anything is launched); nvx_resample_last_error() has the
 * sentence.  nvx_resample_design and nvx_resample_out_count need no device.
 */
#ifndef NAVTEX_AMD_RESAMPLE_H
#define NAVTEX_AMD_RESAMPLE_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_RS_OUTPUT_RATE 252000
#define NVX_RS_SHIFT 15                      /* S */
#define NVX_RS_MIN_RATE 96000
#define NVX_RS_MAX_RATE 3200000
#define NVX_RS_MAX_PHASES 1024               /* L */
#define NVX_RS_MAX_TAPS 32768                /* L * T */

#define NVX_RS_CS16 0                        /* int16 I, Q      (4 bytes per sample) */
#define NVX_RS_CU8  1                        /* uint8 I, Q      (2 bytes per sample) */
#define NVX_RS_CS8  2                        /* int8 I, Q       (2 bytes per sample) */
#define NVX_RS_CF32 3                        /* float32 I, Q    (8 bytes per sample) */

typedef struct nvx_resampler nvx_resampler;

typedef struct nvx_resample_config {
    uint32_t struct_size;       /* sizeof(nvx_resample_config) of the caller's header: set by nvx_resample_config_default */
    int device;                 /* 0 */
    int n_streams;              /* 1 */
    uint32_t input_rate_hz;     /* 2048000 */
    int format;                 /* NVX_RS_CS16 */
} nvx_resample_config;

NVX_API void nvx_resample_config_default(nvx_resample_config *cfg);
NVX_API int  nvx_resample_create(const nvx_resample_config *cfg, nvx_resampler **out);
NVX_API void nvx_resample_destroy(nvx_resampler *r);

/* The plan's numbers and taps for input_rate_hz, without a device: *L, *M, *T, *S (each may be NULL) and, where taps is not
 * NULL and cap is large enough, the L * T taps in phase-major order taps[r * T + t].  Returns L * T (the capacity needed;
 * with taps == NULL or cap < L * T no tap is written), or NVX_ERR_ARG for a rate outside the supported range. */
NVX_API int nvx_resample_design(uint32_t input_rate_hz, int *L, int *M, int *T, int *S, int16_t *taps, int cap);
/* The number of outputs a call with n_in input samples writes for a stream that has consumed consumed_before samples:
 * ceil((consumed_before + n_in) L / M) - ceil(consumed_before L / M).  -1 for an unsupported rate or a sum beyond 2^63. */
NVX_API int64_t nvx_resample_out_count(uint32_t input_rate_hz, uint64_t consumed_before, uint64_t n_in);

/* Every stream of the plan, n_in input samples each (at most 2^30).  d_in: [n_streams][pitch_in_samples] samples in the
 * plan's format in device memory, 16-byte aligned, every row 16-byte aligned (pitch_in_samples times the sample size a
 * multiple of 16 where n_streams > 1).  The nvx_resample_out_count(...) outputs of every stream are written as packed
 * words (I in the low half) to d_out[stream * pitch_out_samples + out_first ...]; *n_out (may be NULL) receives their
 * number.  All streams must stand at the same position (NVX_ERR_STATE otherwise).  Both spans are computed without
 * wrapping and held against the allocations they lie in before anything is launched (NVX_ERR_ARG, no launch).  The work is
 * ordered on hip_stream (a hipStream_t; NULL = the null stream) and NOT waited for.  n_in = 0 is valid and launches
 * nothing. */
NVX_API int nvx_resample_resident(nvx_resampler *r, const void *d_in, size_t pitch_in_samples, size_t n_in,
                                  void *d_out, size_t pitch_out_samples, size_t out_first, size_t *n_out, void *hip_stream);
/* One stream from host memory to host memory: n_in samples in the plan's format at `in`; the outputs as interleaved int16
 * (I, Q) at out_iq, ready for nvx_push_iq; *n_out (may be NULL) their number.  cap_samples smaller than the number of
 * outputs: NVX_ERR_ARG, nothing consumed.  Returns when done. */
NVX_API int nvx_resample_push(nvx_resampler *r, int stream, const void *in, size_t n_in, int16_t *out_iq,
                              size_t cap_samples, size_t *n_out);

/* A stream (-1: every stream) starts anew: position 0, silence in front.  */
NVX_API int nvx_resample_reset(nvx_resampler *r, int stream);
/* Input samples consumed and outputs produced by `stream` since its reset (either pointer may be NULL). */
NVX_API int nvx_resample_position(nvx_resampler *r, int stream, uint64_t *consumed, uint64_t *produced);
/* The plan's own numbers (each pointer may be NULL). */
NVX_API int nvx_resample_plan(nvx_resampler *r, int *L, int *M, int *T, int *n_streams, int *format);

/* Which kernel form nvx_resample_resident launches: 0 = by shape (the default), 1 = one workgroup per stream walking its
 * tiles, 2 = a stream's tiles spread over several workgroups (few streams).  Both give the same bits; the switch exists
 * for tests and measurements. */
NVX_API int nvx_resample_set_form(nvx_resampler *r, int form);

/* HIP-event time of the resampler's kernel, per launch, while enabled (nvx_resample_time_stats waits for the launches
 * still in flight). */
NVX_API int nvx_resample_timing(nvx_resampler *r, int enable);
NVX_API int nvx_resample_time_stats(nvx_resampler *r, double *sum_ms, uint64_t *launches, int reset);
NVX_API const char *nvx_resample_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
