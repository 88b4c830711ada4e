/* navtex_amd_real.h -- real-input converter: real samples at rate fr in any of four formats -> packed int16 IQ at fr / 2,
 * centred on fr / 4.  The interface of the companion library libnavtex_amd_real.so (none of the other libraries is needed
 * to use it).
 *
 * A direct-sampling receiver -- an ADC on the antenna -- delivers real samples, and every other stage of this project takes
 * complex IQ.  The converter is the first stage of the front end for such a radio:
 *     real -> (blank) -> DDC / resample -> scan -> tune -> decode
 * It is the classical fs/4 converter: multiply by (-j)^n, half-band low-pass of gain 2, keep every second sample.  The I
 * branch is then a delayed, sign-alternated even sample, the Q branch one antisymmetric FIR over the odd samples; no multiply
 * meets a zero tap.  Input frequency fr/4 + d comes out at +d.  A real signal's negative-frequency half lands, behind the
 * shift, on the mirrored output frequency: a station at +d has its image at -d, and the filter's stop band is the only thing
 * that removes it.  The library has no notion of rate: everything below is in samples.  To feed the
 * down-converter bank or the resampler (navtex_amd_ddc.h, navtex_amd_resample.h: 96 kS/s .. 3.2 MS/s) fr is 192 kS/s ..
 * 6.4 MS/s; a faster ADC's IQ goes through the zoom bank first (navtex_amd_zoom.h).
 *
 * THE ARITHMETIC, operation by operation.  Integer arithmetic except the one float32 conversion of F32 input.  The GPU
 * result equals a restatement of this text word for word (==, no tolerance).
 *
 * Conversion.  One real component per sample, to an integer in the int16 range, exactly as the other headers convert a
 *   component of IQ:
 *   NVX_REAL_S16   int16:    the value itself
 *   NVX_REAL_U8    uint8 u:  (2 u - 255) * 128
 *   NVX_REAL_S8    int8 s:   s * 256
 *   NVX_REAL_F32   float f:  y = f * 32768 in float32, rounded to the nearest integer with ties to even, clamped to
 *                            [-32768, 32767]; NaN -> 0
 * Indexing.    x[k] is sample k of a stream since its reset, x[k] = 0 for k < 0;  e[i] = x[2 i], o[i] = x[2 i + 1].
 * Filter.      K = 13, S = 14, and fourteen taps
 *       A[0 .. 13] = 10376, 3314, 1825, 1144, 745, 486, 310, 191, 111, 60, 30, 13, 4, 1
 *   (a 55-tap Kaiser half-band, tools/real_taps.py).  Three properties hold:
 *     sum (-1)^j A[j] = 2^13 exactly: unity gain at the band centre and an exact zero at its image;
 *     2 sum A[j] = 37220 <= 65535, so |acc| <= 18610 * 65535 = 1 219 606 350 < 2^31;
 *     a real tone of amplitude a comes out as a complex tone of amplitude a.
 * Output m of a stream since its reset, m = 0, 1, ...:
 *     s   = +1 if (m - K) is even, -1 otherwise
 *     acc = sum over j = 0 .. K of A[j] * (o[m-K-1-j] - o[m-K+j])      exact in int32 (|o| <= 32768: each term is two
 *                                                                       products of at most 10376 * 32768 < 2^29)
 *     q   = (acc + 2^(S-1)) >> S                                       arithmetic shift; |q| <= 74 439
 *     I   = clamp16(s * e[m-K])                                        (-(-32768) clamps to 32767)
 *     Q   = clamp16(s * q), or clamp16(-s * q) when the plan's `invert` is 1
 *     out[m] = (I & 0xffff) | (Q << 16)
 *   invert = 1 conjugates the output: for even Nyquist zones and high-side converters, whose spectrum arrives mirrored.
 * Counts.      Output m needs samples up to x[2 m + 1]: after N samples floor(N / 2) outputs exist.  The delay is K = 13
 *   outputs.  Only the parity of m enters s, so a position beyond 2^32 changes nothing but that.
 * Response.    Computed from the taps: within +-0.001 dB for |f| <= 0.2 fr and at most -79.0 dB for |f| >= 0.3 fr (f the
 *   output frequency; the output spans +-0.25 fr).  Documented: +-0.01 dB over the inner 80 % of the output band (input
 *   0.05 fr .. 0.45 fr), and at most -76 dB for what folds onto it.
 * A stream's output does not depend on how its input was cut into calls, at either entry point.
 * Carried state.  Per stream, in device memory, in two rows used alternately (a launch reads one and writes the other): the
 *   last 2 K + 2 = 28 converted sample pairs (e, o).  The 64-bit position lives on the host, and so does the odd trailing
 *   sample of a push.  Calls on one plan are ordered by the caller: successive calls go on the same hip_stream, or are
 *   synchronised by the caller.
 * Cost.  Memory-bound by design: S16 reads 4 bytes and writes 4 per output.
 *
 * Errors.  Without a HIP device nvx_real_create returns NVX_ERR_NODEV; NULL or nonsense arguments, an odd n_in at
 * nvx_real_resident and spans that leave their allocation return NVX_ERR_ARG (checked before anything is launched);
 * nvx_real_last_error() has the sentence.
 */
#ifndef NAVTEX_AMD_REAL_H
#define NAVTEX_AMD_REAL_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_REAL_S16 0                       /* int16      (2 bytes per sample) */
#define NVX_REAL_U8  1                       /* uint8      (1 byte per sample) */
#define NVX_REAL_S8  2                       /* int8       (1 byte per sample) */
#define NVX_REAL_F32 3                       /* float32    (4 bytes per sample) */

typedef struct nvx_real_converter nvx_real_converter;

typedef struct nvx_real_config {
    uint32_t struct_size;       /* sizeof(nvx_real_config) of the caller's header: set by nvx_real_config_default */
    int device;                 /* 0 */
    int format;                 /* NVX_REAL_S16 */
    int n_streams;              /* 1 */
    int invert;                 /* 0; 1 conjugates the output */
} nvx_real_config;

NVX_API void nvx_real_config_default(nvx_real_config *cfg);
NVX_API int  nvx_real_create(const nvx_real_config *cfg, nvx_real_converter **out);
NVX_API void nvx_real_destroy(nvx_real_converter *c);

/* Every stream of the plan, n_in samples each: n_in is even (an odd n_in is NVX_ERR_ARG) and at most 2^31.  d_in:
 * [n_streams][pitch_in_samples] samples in the plan's format in device memory, 16-byte aligned, every row 16-byte aligned
 * (pitch_in_samples times the sample size a multiple of 16 where n_streams > 1).  The n_in / 2 words of every stream are
 * written (I in the low half) to d_out[stream * pitch_out_samples + out_first ...], 4-byte aligned.  Where every row's first
 * word is 16-byte aligned (the address of d_out[out_first], and with more than one stream pitch_out_samples a multiple of 4)
 * they are written with aligned 16-byte stores; otherwise the same words go out unaligned, slower.  All streams must stand
 * at the same position, and none may hold the odd sample of a push (NVX_ERR_STATE otherwise).  Both spans are computed
 * without wrapping and held against the allocations they lie in before anything is launched (NVX_ERR_ARG, no launch).  The
 * work is ordered on hip_stream (a hipStream_t; NULL = the null stream) and NOT waited for.  n_in = 0 is valid and launches
 * nothing. */
NVX_API int nvx_real_resident(nvx_real_converter *c, const void *d_in, size_t pitch_in_samples, size_t n_in, void *d_out,
                              size_t pitch_out_samples, size_t out_first, void *hip_stream);
/* One stream from host memory to host memory: n_in samples in the plan's format at `in`, any number (at most 2^31); the
 * outputs that exist then, as interleaved int16 (I, Q), to out_iq, which holds cap_samples of them (NVX_ERR_ARG where that
 * is too few: nothing is consumed); *n_out is their number.  An odd trailing sample is held on the host and goes in front
 * of the stream's next push.  Returns when done. */
NVX_API int nvx_real_push(nvx_real_converter *c, int stream, const void *in, size_t n_in, int16_t *out_iq, size_t cap_samples,
                          size_t *n_out);

/* A stream (-1: every stream) starts anew: position 0, silence in front of it, no sample held.  Waits for the launches still
 * in flight. */
NVX_API int nvx_real_reset(nvx_real_converter *c, int stream);
/* Samples consumed by `stream` since its reset (a held one included) and outputs produced (each pointer may be NULL). */
NVX_API int nvx_real_position(nvx_real_converter *c, int stream, uint64_t *consumed, uint64_t *produced);
/* The plan's own numbers (each pointer may be NULL). */
NVX_API int nvx_real_plan(nvx_real_converter *c, int *format, int *n_streams, int *invert);
/* The filter: K, S, and the K + 1 taps A[0 .. K] to taps[0 ...] where taps is not NULL (cap is what it holds: fewer than
 * K + 1 is NVX_ERR_ARG).  Needs no device.  Returns the number of taps. */
NVX_API int nvx_real_taps(int16_t *taps, int cap, int *K, int *S);

/* HIP-event time of the converter's kernel, per call, while enabled (nvx_real_time_stats waits for the launches still in
 * flight). */
NVX_API int nvx_real_timing(nvx_real_converter *c, int enable);
NVX_API int nvx_real_time_stats(nvx_real_converter *c, double *sum_ms, uint64_t *calls, int reset);
NVX_API const char *nvx_real_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
