/* navtex_amd_ddc.h -- down-converter bank: one wide input -> many 252 kS/s slices, each centred where the caller wants it.
 * The interface of the companion library libnavtex_amd_ddc.so (none of the other libraries is needed to use it).
 *
 * The resampler (navtex_amd_resample.h) only changes the rate: its low-pass is centred on the input's own centre, so a
 * station decodes only if the radio was tuned to within 25 kHz of it.  The bank shifts a chosen frequency of the input to
 * the centre first, then filters and resamples with the resampler's own taps:
 *     ddc -> nvx_scan_* / nvx_set_carrier / nvx_push_iq / nvx_process_resident of a raw_rate = 0 handle.
 * A plan has n_inputs inputs of one rate and format and n_slices slices per input; output row input * n_slices + slice.
 *
 * THE ARITHMETIC, operation by operation.  Everything is integer arithmetic except the one float32 conversion of CF32
 * input.  The GPU result equals a restatement of this text word for word (==, no tolerance).
 *
 * Conversion.  The resampler's four formats and rules (NVX_RS_CS16, NVX_RS_CU8, NVX_RS_CS8, NVX_RS_CF32 of
 *   navtex_amd_resample.h), giving x[n] = (I, Q) in the int16 range.  n counts the input's samples since its reset;
 *   x[n] = 0 for n < 0.
 * Grid.  N = 4096, fi = input_rate_hz.  A slice's shift is k * fi / N Hz with k = rint(hz * N / fi) (ties to even): the
 *   frequency hz of the input lands at 0 Hz of the slice, up to the residue hz - k * fi / N, at most fi / 8192 in size
 *   (293 Hz at 2.4 MS/s), which nvx_ddc_grid and nvx_ddc_set_shift report and nvx_set_carrier takes up.
 *   Allowed: |k * fi / N| <= fi / 2 - 25000, so that the slice's +-25 kHz lies inside the input's band; NVX_ERR_ARG otherwise.
 * Table.  W[j] = (c, s) = (rint(32767 cos(2 pi j / N)), rint(32767 sin(2 pi j / N))), j = 0 .. N-1 (nvx_ddc_table hands
 *   it out).  W[j + N/2] = -W[j] and W[j + N/4] = (-s, c) hold exactly; no entry is -32768.
 * Mixer.  j = (k * n) mod N over the integers (the phase is an exact function of the sample index: there is no
 *   accumulator to carry and no phase-truncation spur), (c, s) = W[j],
 *       I' = clamp16((I * c + Q * s + 2^14) >> 15)
 *       Q' = clamp16((Q * c - I * s + 2^14) >> 15)         (arithmetic shifts; the sums are exact in 32 bits)
 *   The clamp is real: rails on both components rotated by 45 degrees reach +-46340.
 *   A slice with k = 0 bypasses the mixer: x' = x exactly (multiplying by 32767 / 32768 is not the identity), so a k = 0
 *   slice equals the resampler's output word for word.
 * Filter, counts, taps.  The resampler's, on x':  pos = n_out * M, q = pos div L, r = pos mod L,
 *       acc = sum over t of h[r][t] * x'[q - t],   out = clamp16((acc + 2^14) >> 15),
 *   with L, M, T and h from nvx_resample_design's rule for fi (the same code is compiled into this library).  After Nin
 *   input samples an input has produced ceil(Nin * L / M) outputs per slice; the output does not depend on how the input
 *   was cut into calls.  Supported rates are the resampler's.
 * Carried state.  Per input (not per slice) the last T-1 converted, UNMIXED samples, in two rows used alternately; they
 *   are mixed when they are staged, with their true index n.  A new shift applies from the next call on, to every sample
 *   that call's windows touch, history included: the phase is NOT continuous across a retune (the T-1 samples in front of
 *   the call are re-mixed with the new k, as if the slice had always had it).  The shift is configuration: nvx_ddc_reset
 *   leaves it alone.  Calls on one plan are ordered by the caller: on one hip_stream, or synchronised.
 *
 * Errors.  Without a HIP device nvx_ddc_create returns NVX_ERR_NODEV; NULL or nonsense arguments, shifts outside the
 * range and spans that leave their allocation return NVX_ERR_ARG (checked before anything is launched);
 * nvx_ddc_last_error() has the sentence.  nvx_ddc_grid and nvx_ddc_table need no device.
 */
#ifndef NAVTEX_AMD_DDC_H
#define NAVTEX_AMD_DDC_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_DDC_OUTPUT_RATE 252000
#define NVX_DDC_GRID 4096                    /* N */
#define NVX_DDC_SCALE 32767                  /* of the table */
#define NVX_DDC_GUARD_HZ 25000               /* a slice's half width: the shift stays this far inside the input's band */

#define NVX_DDC_CS16 0                       /* the resampler's formats, by the resampler's numbers */
#define NVX_DDC_CU8  1
#define NVX_DDC_CS8  2
#define NVX_DDC_CF32 3

typedef struct nvx_ddc nvx_ddc;

typedef struct nvx_ddc_config {
    uint32_t struct_size;       /* sizeof(nvx_ddc_config) of the caller's header: set by nvx_ddc_config_default */
    int device;                 /* 0 */
    int n_inputs;               /* 1 */
    int n_slices;               /* 1; n_inputs * n_slices <= 65535 */
    uint32_t input_rate_hz;     /* 2400000 */
    int format;                 /* NVX_DDC_CU8 */
} nvx_ddc_config;

NVX_API void nvx_ddc_config_default(nvx_ddc_config *cfg);
NVX_API int  nvx_ddc_create(const nvx_ddc_config *cfg, nvx_ddc **out);
NVX_API void nvx_ddc_destroy(nvx_ddc *d);

/* The grid rule without a device: *k (may be NULL) = rint(hz * N / input_rate_hz), *applied_hz (may be NULL) = k *
 * input_rate_hz / N.  NVX_ERR_ARG for an unsupported rate, a hz that is not finite, or a k outside the allowed range. */
NVX_API int nvx_ddc_grid(uint32_t input_rate_hz, double hz, int *k, double *applied_hz);
/* The full turn of the table: cs[2 j] = c, cs[2 j + 1] = s of W[j].  Returns N (the pairs needed); writes only where
 * cs is not NULL and cap_pairs >= N. */
NVX_API int nvx_ddc_table(int16_t *cs, int cap_pairs);

/* The shift of `slice` of `input` (-1: of every input): the frequency hz of the input becomes the slice's centre.
 * *applied_hz (may be NULL) receives the grid frequency actually applied; the residue hz - *applied_hz is nvx_set_carrier's.
 * All shifts start at 0.  Applies from the next call of nvx_ddc_resident / nvx_ddc_push on. */
NVX_API int nvx_ddc_set_shift(nvx_ddc *d, int input, int slice, double hz, double *applied_hz);
NVX_API int nvx_ddc_get_shift(nvx_ddc *d, int input, int slice, int *k, double *applied_hz);

/* Every input of the plan, n_in samples each (at most 2^30).  d_in: [n_inputs][pitch_in_samples] samples in the plan's
 * format in device memory, 16-byte aligned, every row 16-byte aligned.  Every slice's outputs are written as packed words
 * (I in the low half) to d_out[(input * n_slices + slice) * pitch_out_samples + out_first ...]; *n_out (may be NULL)
 * receives their number per slice.  All inputs must stand at the same position (NVX_ERR_STATE otherwise).  Both spans are
 * computed without wrapping and held against the allocations they lie in before anything is launched (NVX_ERR_ARG, no
 * launch).  The work is ordered on hip_stream (a hipStream_t; NULL = the null stream) and NOT waited for.  n_in = 0 is
 * valid and launches nothing. */
NVX_API int nvx_ddc_resident(nvx_ddc *d, const void *d_in, size_t pitch_in_samples, size_t n_in, void *d_out,
                             size_t pitch_out_samples, size_t out_first, size_t *n_out, void *hip_stream);
/* One input from host memory to host memory: n_in samples in the plan's format at `in`; slice s's outputs as interleaved
 * int16 (I, Q) at out_iq + s * cap_samples * 2; *n_out (may be NULL) their number per slice.  cap_samples smaller than
 * that number: NVX_ERR_ARG, nothing consumed.  Returns when done. */
NVX_API int nvx_ddc_push(nvx_ddc *d, int input, const void *in, size_t n_in, int16_t *out_iq, size_t cap_samples, size_t *n_out);

/* An input (-1: every input) starts anew: position 0, silence in front.  Shifts stay. */
NVX_API int nvx_ddc_reset(nvx_ddc *d, int input);
/* Input samples consumed and outputs produced per slice by `input` since its reset (either pointer may be NULL). */
NVX_API int nvx_ddc_position(nvx_ddc *d, int input, uint64_t *consumed, uint64_t *produced);
/* The plan's own numbers (each pointer may be NULL). */
NVX_API int nvx_ddc_plan(nvx_ddc *d, int *L, int *M, int *T, int *n_inputs, int *n_slices, int *format);

/* HIP-event time of the bank's kernel, per launch, while enabled (nvx_ddc_time_stats waits for the launches in flight). */
NVX_API int nvx_ddc_timing(nvx_ddc *d, int enable);
NVX_API int nvx_ddc_time_stats(nvx_ddc *d, double *sum_ms, uint64_t *launches, int reset);
NVX_API const char *nvx_ddc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
