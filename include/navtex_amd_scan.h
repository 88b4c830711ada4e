/* navtex_amd_scan.h -- band scan: where in a stream's +-25 kHz are the carriers a chain can be tuned to?
 * The interface of the companion library libnavtex_amd_scan.so (libnavtex_amd.so itself is not needed to use it).
 *
 * nvx_set_carrier (navtex_amd_tune.h) needs an offset; a signal report's offset_hz (navtex_amd_signal.h) exists only
 * once the demodulator has caught the signal, within about 75 Hz.  The scan closes the gap: per stream an averaged
 * power spectrum of FIR1's output -- FIR1's passband, the range the tuned mixer reaches -- and a host function that
 * turns such a row into a list of FSK carriers:   scan -> nvx_set_carrier(hit.offset_hz) -> decode -> report.
 *
 * THE SPECTRUM, operation by operation (all arithmetic IEEE fp64, every product and every sum rounded on its own: no
 * fused multiply-add anywhere).  The GPU result equals a restatement of this text bit for bit.
 *
 * Input chain.  int16 IQ at 2.016 MS/s passes through stage 0 of order 1 or 3 exactly as a handle's cascade does it
 *   (order 1: x[m] = floor((sum of raw[8m .. 8m+7] + 4) / 8); order 3: x[m] = floor((sum_j w[j] raw[8m+7-j] + 256) / 512),
 *   w = three 8-sample boxcars convolved, 22 taps); the result, or 252 kS/s input directly, goes through FIR1 (37 taps,
 *   decimation 4):  y1[o] = sum over i = 0 .. 36, in that order, of h[i] * x[4 o + 3 - i], starting from 0.0
 *   (acc = acc + h[i] * x), one accumulator per output and component.  y1 runs at 63 kS/s; a frame holds 20160 outputs.
 * Slots.  A frame is cut into NVX_SCAN_SLOTS_PER_FRAME = 9 slots of 2240 FIR1 outputs.  The segment of slot j of frame f
 *   is y1[f * 20160 + j * 2240 + 16 + n], n = 0 .. 2047.  The lead-in of 16 outputs (64 samples at 252 kS/s, 512 raw
 *   samples) is longer than FIR1's reach (36 samples) plus the third-order stage 0's (21 raw samples): no segment value
 *   depends on anything in front of its own slot, so the values are the streaming FIR1 outputs at those indices, and
 *   a scan of frames [f0, f0 + n) depends on nothing before f0.
 * Window.  Hann from the twiddle table: w[n] = 0.5 - 0.5 * C[n], C[n] = cos(2 pi n / 2048) (the product is exact: one
 *   rounding); v[n] = (w[n] * I[n], w[n] * Q[n]).
 * Transform.  2048-point radix-2 decimation in time: x = v in bit-reversed order, then stages len = 2, 4, .., 2048; for
 *   a = x[i], b = x[i + len/2], position j of i in its block of len, (wr, wi) = (C[j * 2048 / len], -S[j * 2048 / len]):
 *       t.re = b.re * wr - b.im * wi;   t.im = b.re * wi + b.im * wr;   x[i] = a + t;   x[i + len/2] = a - t.
 *   C and S are the table of navtex_amd/scan/nvx_scan_table.h (first octant correctly rounded, the rest of the turn by
 *   exact swaps and sign flips).
 * Power and averaging.  p[b] = re * re + im * im (two products, one sum).  A frame's row is the sum of its 9 slots'
 *   p in ascending slot order, starting from 0.0; the scan's row is the sum of the frame rows in ascending frame
 *   order, starting from 0.0.  (The two levels let a workgroup per stream and a workgroup per (stream, frame) plus an
 *   ordered fold give the same bits.)  No scaling: a row grows with the number of frames.
 * Output.  [stream][NVX_SCAN_FFT] doubles; index i holds FFT bin (i + 1024) mod 2048, i.e. the frequency
 *   (i - 1024) * NVX_SCAN_BIN_HZ from the stream's centre, with the sign of nvx_set_carrier's offset_hz and the
 *   synthetic source's freq_hz.
 *
 * Errors.  Without a HIP device the device entry points return NVX_ERR_NODEV; NULL or nonsense arguments and spans
 * that leave their allocation return NVX_ERR_ARG (checked before anything is launched); nvx_scan_last_error() has the
 * sentence.  nvx_scan_find needs no device.
 */
#ifndef NAVTEX_AMD_SCAN_H
#define NAVTEX_AMD_SCAN_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_SCAN_FFT 2048
#define NVX_SCAN_BIN_HZ 30.76171875          /* 63000 / 2048 */
#define NVX_SCAN_SLOTS_PER_FRAME 9
#define NVX_SCAN_SLOT_OUTPUTS 2240           /* FIR1 outputs per slot: 9 * 2240 = 20160 */
#define NVX_SCAN_LEAD_IN 16                  /* FIR1 outputs of a slot in front of its segment */

/* d_iq: [n_streams][pitch_samples] packed IQ in device memory as nvx_process_resident takes it (4 bytes per sample, I in
 * the low half; 16-byte aligned, pitch_samples a multiple of 4); frames [first_frame, first_frame + n_frames) of every
 * stream are scanned (a frame: 645120 samples at raw_rate 1, 80640 at raw_rate 0).  stage0_order 1 or 3 (0 = 1) at
 * raw_rate 1, 0 or 1 otherwise.  d_power: [n_streams][2048] doubles in device memory.  The work is ordered on hip_stream
 * (a hipStream_t; NULL = the null stream) and NOT waited for. */
NVX_API int nvx_scan_resident(int device, const void *d_iq, size_t pitch_samples, size_t first_frame, int n_frames,
                              int n_streams, int raw_rate, int stage0_order, void *d_power, void *hip_stream);
/* One stream from host memory: the whole frames among the n samples are scanned (n < one frame: NVX_ERR_ARG; a partial
 * last frame is ignored), *frames_used (may be NULL) receives their number; power: host [2048].  Returns when done. */
NVX_API int nvx_scan_iq(int device, const int16_t *iq_interleaved, size_t n, int raw_rate, int stage0_order,
                        double *power, int *frames_used);

/* Which kernel form nvx_scan_resident launches: 0 = by shape (the default), 1 = one workgroup per stream walking its
 * frames, 2 = one workgroup per (stream, frame) and an ordered fold, wherever its frame rows fit the scratch limit
 * (16384 rows).  Both give the same bits; the switch exists for tests and measurements. */
NVX_API int nvx_scan_set_form(int form);

/* HIP-event time of the scan's kernels, per nvx_scan_resident call, while enabled (nvx_scan_time_stats waits for the
 * launches still in flight). */
NVX_API void nvx_scan_timing(int enable);
NVX_API int  nvx_scan_time_stats(double *sum_ms, uint64_t *launches, int reset);
NVX_API const char *nvx_scan_last_error(void);

/* ---- the detector: a power row -> FSK carriers (host only) ----------------------------------------------------------
 * With N = 2048 and P the row (indices wrap around):
 *  1. band sum   B[i] = sum over d = -band_half .. +band_half, ascending, of P[i + d], from 0.0;
 *  2. floor      F[i] = (2 band_half + 1) * median of the 2 floor_half + 1 values P[i - floor_half .. i + floor_half];
 *  3. score[i] = 10 log10(B[i] / F[i]); a bin whose F or B is not positive is no candidate;
 *  4. candidates are walked by descending score, lower bin first on ties, down to min_score_db;
 *  5. one within guard_bins (circular distance <=) of a peak kept before it is skipped; else it is a peak;
 *  6. a peak is dropped if a peak kept before it within shadow_bins has a band sum more than shadow_db above its own
 *     (a strong FSK signal's own side lobes); a dropped peak guards nothing: a weaker station beside it is still found;
 *  7. refinement: refine_iters times k = c + (sum_d d P[c + d]) / (sum_d P[c + d]), d = -refine_half .. refine_half,
 *     c = the bin, then floor(k + 0.5); the lower tone is the first largest P in [c - refine_half, c - 1], the upper one
 *     in [c + 1, c + refine_half]; each is refined by the vertex of the parabola through ln P of the bin and its two
 *     neighbours (no shift where a value is not positive or the three are not concave; at most one bin); the carrier
 *     is the midpoint of the two tones and shift_hz their distance (NAVTEX: about 170; an unmodulated carrier: small);
 *  8. a peak whose carrier lies beyond max_offset_hz is kept for rule 6 but not reported; neither is a single line at the
 *     stream's centre -- carrier within dc_guard_hz of it and tones less than dc_max_shift_hz apart: the input's DC
 *     offset, not a station (an FSK carrier tuned exactly to the centre has its tones 170 Hz apart and is reported);
 *  9. hits are reported in the order found: descending score.
 * A plain power centroid is not enough: SITOR-B characters are 4 'B' : 3 'Y', which pulls it tens of Hz. */
typedef struct nvx_scan_params {
    uint32_t struct_size;     /* sizeof(nvx_scan_params) of the caller's header: set by nvx_scan_params_default */
    int band_half;            /* 5   */
    int floor_half;           /* 32  */
    int guard_bins;           /* 13  */
    int shadow_bins;          /* 33  */
    int refine_half;          /* 6   */
    int refine_iters;         /* 4   */
    double min_score_db;      /* 6.0 */
    double shadow_db;         /* 25.0 */
    double max_offset_hz;     /* 25000.0: nvx_set_carrier's range */
    double dc_guard_hz;       /* 60.0  */
    double dc_max_shift_hz;   /* 120.0 */
} nvx_scan_params;

typedef struct nvx_scan_hit {
    double offset_hz;         /* the carrier, from the stream's centre: what nvx_set_carrier takes */
    double score_db;          /* band sum over local floor at the peak bin */
    double shift_hz;          /* distance of the two tones */
    double band_power_db;     /* 10 log10 of the band sum (the row's own scale) */
    int bin;                  /* the peak's index in the row */
} nvx_scan_hit;

NVX_API void nvx_scan_params_default(nvx_scan_params *p);
/* power: [2048]; p may be NULL (the defaults); at most cap hits are written.  Returns the number of hits found (which
 * may exceed cap), or NVX_ERR_ARG. */
NVX_API int  nvx_scan_find(const double *power, const nvx_scan_params *p, nvx_scan_hit *hits, int cap);

#ifdef __cplusplus
}
#endif
#endif
