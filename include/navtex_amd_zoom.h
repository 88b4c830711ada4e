/* navtex_amd_zoom.h -- zoom bank: one wide IQ input in any of four formats -> n_zooms rows of packed int16 IQ at 1 / 2^k of
 * the input rate, each centred on a frequency of the caller's choice.  The interface of the companion library
 * libnavtex_amd_zoom.so (none of the other libraries is needed to use it).
 *
 * The resampler, the down-converter bank and every same-rate companion take IQ at 96 kS/s .. 3.2 MS/s; above that
 * navtex_amd_resample.h says "out of scope -- decimate in the radio".  The zoom bank is that decimation, on the GPU: the
 * first stage of the front end for a radio that delivers more than 3.2 MS/s,
 *     (real ->) zoom -> IQ-correct / blank / notch -> DDC / resample -> scan -> tune -> decode
 * Its rows are what nvx_ddc_*, nvx_resample_* and the same-rate companions take as CS16; where the input rate is
 * 252 000 * 2^k they are what a raw_rate = 0 handle and the scan take directly.  Like navtex_amd_real.h the library has no
 * notion of rate: everything below is in samples and table steps, and one helper (nvx_zoom_grid, no device) turns Hz at a
 * given rate into a table step and back.
 * A plan has n_inputs inputs of one format, n_zooms zooms per input and one k; output row input * n_zooms + zoom.
 *
 * THE ARITHMETIC, operation by operation.  Integer arithmetic except the one float32 conversion of CF32 input.  The GPU
 * result equals a restatement of this text word for word (==, no tolerance).
 *
 * Conversion.  The resampler's four formats and rules (NVX_RS_CS16, NVX_RS_CU8, NVX_RS_CS8, NVX_RS_CF32 of
 *   navtex_amd_resample.h), giving x[n] = (I, Q) in the int16 range.  n counts the input's samples since its reset;
 *   x[n] = 0 for n < 0.
 * Mixer.  The bank's (navtex_amd_ddc.h), verbatim: N = 4096, W[j] = (c, s) its table, j = (kz * n) mod N over the integers,
 *       I' = clamp16((I * c + Q * s + 2^14) >> 15)
 *       Q' = clamp16((Q * c - I * s + 2^14) >> 15)         (arithmetic shifts; the sums are exact in 32 bits)
 *   kz is any integer in -2048 .. 2047: the shift in cycles per input sample times 4096; the input's frequency kz / 4096
 *   lands at 0 of the zoom.  kz = 0 bypasses the mixer: x' = x exactly.  The residue of a wanted frequency is at most
 *   1 / 8192 cycle per input sample; nvx_zoom_grid reports it, and the bank's nvx_ddc_set_shift or nvx_set_carrier takes it
 *   up downstream.  The mixer's worst spur is the bank's -99.8 dBc.
 * Stages.  k identical half-band stages, on I and Q separately, u_0 = x'.  The taps are the real-input converter's fourteen,
 *   A[0 .. 13] = 10376, 3314, 1825, 1144, 745, 486, 310, 191, 111, 60, 30, 13, 4, 1 (nvx_zoom_taps hands them out), here as
 *   a unity-gain low-pass of 55 taps at scale 2^15 with centre tap 2^14 and odd taps (-1)^j A[j]:
 *       acc    = 2^14 * u_{s-1}[2m - 26] + sum over j = 0 .. 13 of (-1)^j A[j] * (u_{s-1}[2m - 27 - 2j] + u_{s-1}[2m - 25 + 2j])
 *       u_s[m] = clamp16((acc + 2^14) >> 15)                arithmetic shift
 *   The newest sample a stage output touches is 2m + 1, the oldest 2m - 53.  The taps sum to exactly 2^15 (DC gain 1); their
 *   magnitudes sum to 16384 + 37220 = 53604, so |acc| <= 53604 * 32768 = 1 756 495 872 and acc + 2^14 < 2^31: the sum is
 *   exact in int32.  The clamp is real: a stage's output can reach +-53604 in front of it.
 * Output.  y[m] = u_k[m], as (I & 0xffff) | (Q << 16).
 * Counts.  D = 2^k.  y[m] needs x up to D m + D - 1: after Nin samples floor(Nin / D) outputs exist.  The group delay is
 *   26 (D - 1) input samples.  A call's outputs depend on the H = 53 (D - 1) input samples in front of it (3339 for k = 6).
 * Response.  Computed from the taps, over the inner 80 % of the output band (|f| <= 0.4 of the output rate), k = 1 .. 6:
 *   ripple -0.0006 .. +0.0037 dB, and everything that folds onto that band at most -78.99 dB.  Documented: +-0.01 dB over the
 *   inner 80 %, and at most -76 dB for what folds onto it.
 * Carried state.  Per input (not per zoom) the last H converted, UNMIXED samples, in two rows used alternately.  The 64-bit
 *   position lives on the host (only n mod 4096 enters the phase), and so do the up to D - 1 trailing samples of a push.  A
 *   new shift applies from the next call on, to every sample that call touches, history included: the H samples in front of
 *   the call are re-mixed with the new kz, as if the zoom had always had it.  The shift is configuration: nvx_zoom_reset
 *   leaves it alone.  An input's output does not depend on how it was cut into calls, at either entry point.  Calls on one
 *   plan are ordered by the caller: on one hip_stream, or synchronised.
 *
 * Errors.  Without a HIP device nvx_zoom_create returns NVX_ERR_NODEV; NULL or nonsense arguments, a kz outside the range, an
 * n_in at nvx_zoom_resident that is no multiple of D and spans that leave their allocation return NVX_ERR_ARG (checked before
 * anything is launched); inputs at different positions return NVX_ERR_STATE; nvx_zoom_last_error() has the sentence.
 * nvx_zoom_grid and nvx_zoom_taps need no device.
 */
#ifndef NAVTEX_AMD_ZOOM_H
#define NAVTEX_AMD_ZOOM_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_ZOOM_GRID 4096                   /* N: the bank's table */
#define NVX_ZOOM_KZ_MIN (-2048)
#define NVX_ZOOM_KZ_MAX 2047
#define NVX_ZOOM_MAX_ZOOMS 8
#define NVX_ZOOM_MIN_LOG2 1
#define NVX_ZOOM_MAX_LOG2 6
#define NVX_ZOOM_STAGE_REACH 53              /* samples in front of its newest pair a stage output reaches over */
#define NVX_ZOOM_STAGE_DELAY 26              /* a stage's group delay, in its input's samples */

#define NVX_ZOOM_CS16 0                      /* the resampler's formats, by the resampler's numbers */
#define NVX_ZOOM_CU8  1
#define NVX_ZOOM_CS8  2
#define NVX_ZOOM_CF32 3

typedef struct nvx_zoom nvx_zoom;

typedef struct nvx_zoom_config {
    uint32_t struct_size;       /* sizeof(nvx_zoom_config) of the caller's header: set by nvx_zoom_config_default */
    int device;                 /* 0 */
    int n_inputs;               /* 1 */
    int n_zooms;                /* 1; 1 .. 8, n_inputs * n_zooms <= 65535 */
    int log2_decim;             /* 1; k = 1 .. 6 */
    int format;                 /* NVX_ZOOM_CS16 */
} nvx_zoom_config;

NVX_API void nvx_zoom_config_default(nvx_zoom_config *cfg);
NVX_API int  nvx_zoom_create(const nvx_zoom_config *cfg, nvx_zoom **out);
NVX_API void nvx_zoom_destroy(nvx_zoom *z);

/* The grid rule without a device: *kz (may be NULL) = rint(hz * N / rate_hz), ties to even; *applied_hz (may be NULL) =
 * kz * rate_hz / N.  NVX_ERR_ARG for a rate that is not positive and finite, a hz that is not finite, or a kz outside
 * NVX_ZOOM_KZ_MIN .. NVX_ZOOM_KZ_MAX. */
NVX_API int nvx_zoom_grid(double rate_hz, double hz, int *kz, double *applied_hz);

/* The shift of `zoom` of `input` (-1: of every input), as a table step.  All shifts start at 0.  Applies from the next call
 * of nvx_zoom_resident / nvx_zoom_push on, and waits for nothing. */
NVX_API int nvx_zoom_set_shift(nvx_zoom *z, int input, int zoom, int kz);
NVX_API int nvx_zoom_get_shift(nvx_zoom *z, int input, int zoom, int *kz);

/* Every input of the plan, n_in samples each: n_in is a multiple of D (NVX_ERR_ARG otherwise) and at most 2^30.  d_in:
 * [n_inputs][pitch_in_samples] samples in the plan's format in device memory, 16-byte aligned, every row 16-byte aligned.
 * The n_in / D words of every zoom are written (I in the low half) to d_out[(input * n_zooms + zoom) * pitch_out_samples +
 * out_first ...], 4-byte aligned; *n_out (may be NULL) receives their number per zoom.  Where every output row's first word is
 * 16-byte aligned (the address of d_out[out_first], and with more than one row pitch_out_samples a multiple of 4) they are
 * written with aligned 16-byte stores; otherwise the same words go out unaligned, slower.  All inputs must stand at the same
 * position, and none may hold samples of a push (NVX_ERR_STATE otherwise).  Both spans are computed without wrapping and held
 * against the allocations they lie in before anything is launched (NVX_ERR_ARG, no launch).  The work is ordered on
 * hip_stream (a hipStream_t; NULL = the null stream) and NOT waited for.  n_in = 0 is valid and launches nothing. */
NVX_API int nvx_zoom_resident(nvx_zoom *z, const void *d_in, size_t pitch_in_samples, size_t n_in, void *d_out,
                              size_t pitch_out_samples, size_t out_first, size_t *n_out, void *hip_stream);
/* One input from host memory to host memory: n_in samples in the plan's format at `in`, any number (at most 2^30); zoom s's
 * outputs that exist then as interleaved int16 (I, Q) at out_iq + s * cap_samples * 2; *n_out (may be NULL) their number per
 * zoom.  cap_samples smaller than that number: NVX_ERR_ARG, nothing consumed.  Up to D - 1 trailing samples are held on the
 * host and go in front of the input's next push.  Returns when done. */
NVX_API int nvx_zoom_push(nvx_zoom *z, int input, const void *in, size_t n_in, int16_t *out_iq, size_t cap_samples, size_t *n_out);

/* An input (-1: every input) starts anew: position 0, silence in front, no sample held.  Shifts stay.  Waits for the
 * launches still in flight. */
NVX_API int nvx_zoom_reset(nvx_zoom *z, int input);
/* Samples consumed by `input` since its reset (held ones included) and outputs produced per zoom (either pointer may be NULL). */
NVX_API int nvx_zoom_position(nvx_zoom *z, int input, uint64_t *consumed, uint64_t *produced);
/* The plan's own numbers (each pointer may be NULL): history is H. */
NVX_API int nvx_zoom_plan(nvx_zoom *z, int *format, int *n_inputs, int *n_zooms, int *log2_decim, int *history);
/* The stage filter: the fourteen taps A[0 .. 13] to taps[0 ...] where taps is not NULL (cap is what it holds: fewer than
 * fourteen is NVX_ERR_ARG); *reach = 53, *shift = 15.  Needs no device.  Returns the number of taps. */
NVX_API int nvx_zoom_taps(int16_t *taps, int cap, int *reach, int *shift);

/* HIP-event time of the zoom's kernel, per call, while enabled (nvx_zoom_time_stats waits for the launches in flight). */
NVX_API int nvx_zoom_timing(nvx_zoom *z, int enable);
NVX_API int nvx_zoom_time_stats(nvx_zoom *z, double *sum_ms, uint64_t *calls, int reset);
NVX_API const char *nvx_zoom_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
