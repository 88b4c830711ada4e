/* navtex_amd_iqc.h -- IQ corrector: IQ at any rate and in any of the resampler's sample formats -> packed int16 IQ at the
 * same rate, with the DC offset removed and the gain and phase error of the Q branch against the I branch taken out.
 * The interface of the companion library libnavtex_amd_iqc.so (none of the other libraries is needed to use it).
 *
 * A zero-IF radio delivers I and Q through two analogue branches that differ by a few percent in gain and a few degrees in
 * phase, and both carry a DC offset.  Gain and phase error put a mirror image of every signal at the negated frequency,
 * about 30 dB down: the image of a strong station at +14 kHz lies on the chain at -14 kHz, and behind the mixers it is
 * co-channel interference that nothing can remove.  The corrector is the first stage of the front end:
 *     IQ-correct -> blank -> DDC / resample -> scan -> tune -> decode
 * (in front of the blanker: the blanker's zeros would bias the statistics).  It has no notion of rate: everything below is
 * in samples.
 *
 * THE ARITHMETIC, operation by operation.  Integer arithmetic except the one float32 conversion of CF32 input; every shift
 * and every division below is a floor shift or floor division of signed 64-bit integers.  The GPU result equals a
 * restatement of this text word for word (==, no tolerance).
 *
 * Conversion.  Exactly as in navtex_amd_blank.h, per component, to an integer in the int16 range:
 *   NVX_IQC_CS16   int16:    the value itself
 *   NVX_IQC_CU8    uint8 u:  (2 u - 255) * 128
 *   NVX_IQC_CS8    int8 s:   s * 256
 *   NVX_IQC_CF32   float f:  y = f * 32768 in float32, rounded to the nearest integer with ties to even, clamped to
 *                            [-32768, 32767]; NaN -> 0
 *   x[n] = (I, Q); n counts a stream's samples since its reset.  Samples are interleaved I, Q in every format.
 * Blocks.      NVX_IQC_BLOCK = 65536 samples by absolute index, b = n div 65536.  A block has five exact sums in int64:
 *   SI, SQ, SII, SQQ, SIQ = the sums of I, Q, I^2, Q^2 and I Q over its samples (|SI| <= 2^31, SII <= 2^46).
 * Window.      W = 4, 16 or 64 blocks (window_log2 = 2, 4 or 6; default 4), N = W * 65536 = 2^(16 + window_log2) samples.
 *   TI, TQ, TII, TQQ, TIQ are the sums over the last W complete blocks (|TI| <= 2^37, TII <= 2^52, |TIQ| <= 2^52).
 * Solve.       At the first sample of every block in front of which W blocks are complete since the reset (from a reset at
 *   0: every block b >= W), in NVX_IQC_TRACK mode:
 *    1. dI = (TI + N/2) >> log2 N, dQ likewise                                  (-32768 .. 32767)
 *    2. CII = TII - 2 dI TI + N dI^2                                            (each term <= 2^54; CII = sum (I - dI)^2 >= 0)
 *    3. CQQ = TQQ - 2 dQ TQ + N dQ^2
 *    4. CIQ = TIQ - dI TQ - dQ TI + N dI dQ                                     (each term <= 2^53; |CIQ| <= max(CII, CQQ) < 2^54)
 *    5. if CII < 16 N or CQQ < 16 N: the result is (dI, dQ, 0, 16384), reason 1: too little signal
 *    6. s = max(0, bitlength(max(CII, CQQ)) - 30);  cii, cqq, ciq = CII >> s, CQQ >> s, CIQ >> s   (cii, cqq < 2^30, |ciq| <= 2^30)
 *    7. a = floor((-ciq * 32768 + cii) / (2 cii))                               (Q14; the numerator stays below 2^46; cii >= 4, as CII >= 16 N)
 *       if |a| > 4096: reason 2
 *    8. v = cqq + ((2 a ciq) >> 14) + ((a a cii) >> 28)                         (2 a ciq <= 2^43, a a cii <= 2^54)
 *       if v <= 0: reason 3
 *    9. g = isqrt(floor((cii << 28) / v))                                       (cii << 28 < 2^58)
 *       if g < 12288 or g > 21845: reason 4
 *   10. otherwise c_q = g, c_i = (a g + 8192) >> 14 (|c_i| <= 5462), reason 0
 *   A reason other than 0 keeps dI and dQ, sets c_i = 0 and c_q = 16384, and counts a rejected block; reason 0 counts a
 *   solved one.  a is minus the coherence of the branches (the phase error), g the ratio of their levels once that is out.
 * Apply.       i = I - dI, q = Q - dQ;  outI = clamp16(i);  outQ = clamp16((c_q q + c_i i + 8192) >> 14)
 *   (the sum fits int32: 21845 * 65535 + 5462 * 65535 + 8192 < 2^31);  out[n] = (outI & 0xffff) | (outQ << 16).
 *   The identity (0, 0, 0, 16384) gives the conversion word for word.
 * Until W blocks are complete, and in NVX_IQC_HOLD mode, the coefficients stay what they are: the identity after create or
 *   reset, the last solved or set ones otherwise.
 * A stream's output does not depend on how its input was cut into calls.
 * Carried state.  Per stream, in device memory, in two rows used alternately (a launch reads one and writes the other): the
 *   ring of the last W block sums, the open block's partial sums, the blocks complete since the reset saturated at W, the
 *   current coefficients, the mode and the last reason.  The 64-bit position lives on the host.  Calls on one plan are
 *   ordered by the caller: successive calls go on the same hip_stream, or are synchronised by the caller.
 * Known limit.  The estimate is blind: it takes the correlation of I and Q, and the difference of their levels, over the
 *   window for the radio's error.  Two strong stations at mirrored frequencies are correlated over a finite window, and the
 *   coefficients wander with them (DESIGN 3.10 has figures); the image this makes of a station is the residual coherence
 *   times the station's own amplitude on the mirrored channel.  That is why W defaults to 16 and why NVX_IQC_HOLD exists: a
 *   calibrated radio is "track for a while, then hold".
 * Cost.  The input is read twice and 4 bytes written per sample (CS16: 12 bytes against the blanker's 8).
 *
 * Errors.  Without a HIP device nvx_iqc_create returns NVX_ERR_NODEV; NULL or nonsense arguments and spans that leave their
 * allocation return NVX_ERR_ARG (checked before anything is launched); nvx_iqc_last_error() has the sentence.
 */
#ifndef NAVTEX_AMD_IQC_H
#define NAVTEX_AMD_IQC_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_IQC_BLOCK 65536                  /* samples per block */
#define NVX_IQC_WINDOW_LOG2_DEFAULT 4        /* W = 16 blocks; 2 and 6 are the other values */
#define NVX_IQC_CQ_IDENTITY 16384            /* 1.0 in Q14 */
#define NVX_IQC_CQ_MIN 12288                 /* 0.75 */
#define NVX_IQC_CQ_MAX 21845                 /* 1.3333 */
#define NVX_IQC_CI_MAX 5462                  /* |c_i| of a solved or set correction */

#define NVX_IQC_TRACK 0                      /* solve at every block start once the window is full */
#define NVX_IQC_HOLD 1                       /* keep the coefficients; the sums go on */

#define NVX_IQC_CS16 0                       /* int16 I, Q      (4 bytes per sample) */
#define NVX_IQC_CU8  1                       /* uint8 I, Q      (2 bytes per sample) */
#define NVX_IQC_CS8  2                       /* int8 I, Q       (2 bytes per sample) */
#define NVX_IQC_CF32 3                       /* float32 I, Q    (8 bytes per sample) */

typedef struct nvx_iq_corrector nvx_iq_corrector;

typedef struct nvx_iqc_config {
    uint32_t struct_size;       /* sizeof(nvx_iqc_config) of the caller's header: set by nvx_iqc_config_default */
    int device;                 /* 0 */
    int format;                 /* NVX_IQC_CS16 */
    int n_streams;              /* 1 */
    int window_log2;            /* 4 */
} nvx_iqc_config;

/* What nvx_iqc_get returns about one stream. */
typedef struct nvx_iqc_status {
    int32_t dI, dQ, c_i, c_q;   /* the current coefficients: those of the stream's last sample, or set since */
    int32_t mode;               /* NVX_IQC_TRACK or NVX_IQC_HOLD */
    int32_t last_reason;        /* of the last block solved or rejected since the reset: 0 .. 4 */
    int64_t sums[5];            /* TI, TQ, TII, TQQ, TIQ over the complete blocks of the window */
    uint64_t samples;           /* consumed since creation */
    uint64_t blocks_solved;     /* block starts with reason 0 since creation */
    uint64_t blocks_rejected;   /* ... with another reason */
} nvx_iqc_status;

NVX_API void nvx_iqc_config_default(nvx_iqc_config *cfg);
NVX_API int  nvx_iqc_create(const nvx_iqc_config *cfg, nvx_iq_corrector **out);
NVX_API void nvx_iqc_destroy(nvx_iq_corrector *c);

/* Every stream of the plan, n_in samples each (at most 2^30).  d_in: [n_streams][pitch_in_samples] samples in the plan's
 * format in device memory, 16-byte aligned, every row 16-byte aligned (pitch_in_samples times the sample size a multiple of
 * 16 where n_streams > 1).  The n_in words of every stream are written (I in the low half) to
 * d_out[stream * pitch_out_samples + out_first ...], 4-byte aligned.  Where every row's first word is 16-byte aligned (the
 * address of d_out[out_first], and with more than one stream pitch_out_samples a multiple of 4) they are written with
 * aligned 16-byte stores; otherwise the same words go out unaligned, slower.  All streams must stand at the same position
 * (NVX_ERR_STATE otherwise).  Both spans are computed without wrapping and held against the allocations they lie in before
 * anything is launched (NVX_ERR_ARG, no launch).  The work is ordered on hip_stream (a hipStream_t; NULL = the null stream)
 * and NOT waited for.  n_in = 0 is valid and launches nothing. */
NVX_API int nvx_iqc_resident(nvx_iq_corrector *c, const void *d_in, size_t pitch_in_samples, size_t n_in, void *d_out,
                             size_t pitch_out_samples, size_t out_first, void *hip_stream);
/* One stream from host memory to host memory: n_in samples in the plan's format at `in`, n_in samples of interleaved int16
 * (I, Q) to out_iq.  Returns when done. */
NVX_API int nvx_iqc_push(nvx_iq_corrector *c, int stream, const void *in, size_t n_in, int16_t *out_iq);

/* A stream (-1: every stream) starts anew: position 0, no block complete, the identity.  Its mode and counters stay.  Waits
 * for the launches still in flight, as the three calls below do. */
NVX_API int nvx_iqc_reset(nvx_iq_corrector *c, int stream);
/* The coefficients of `stream` (-1: every stream) from the next call's first sample on: dI, dQ in -32768 .. 32767, |c_i| <=
 * NVX_IQC_CI_MAX, c_q in NVX_IQC_CQ_MIN .. NVX_IQC_CQ_MAX.  In NVX_IQC_TRACK mode the next solve replaces them. */
NVX_API int nvx_iqc_set(nvx_iq_corrector *c, int stream, int dI, int dQ, int c_i, int c_q);
/* NVX_IQC_TRACK or NVX_IQC_HOLD for `stream` (-1: every stream) from the next call's first sample on. */
NVX_API int nvx_iqc_set_mode(nvx_iq_corrector *c, int stream, int mode);
NVX_API int nvx_iqc_get(nvx_iq_corrector *c, int stream, nvx_iqc_status *out);
/* Samples consumed by `stream` since its reset. */
NVX_API int nvx_iqc_position(nvx_iq_corrector *c, int stream, uint64_t *consumed);
/* The plan's own numbers (each pointer may be NULL). */
NVX_API int nvx_iqc_plan(nvx_iq_corrector *c, int *format, int *n_streams, int *window_log2);

/* HIP-event time of the corrector's two kernels, per call, while enabled (nvx_iqc_time_stats waits for the launches still
 * in flight). */
NVX_API int nvx_iqc_timing(nvx_iq_corrector *c, int enable);
NVX_API int nvx_iqc_time_stats(nvx_iq_corrector *c, double *sum_ms, uint64_t *calls, int reset);
NVX_API const char *nvx_iqc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
