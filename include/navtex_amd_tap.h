/* navtex_amd_tap.h -- channel tap: any carrier of a packed int16 IQ row at 252 kS/s comes out again as a narrow signal, low-rate
 * IQ at 2 .. 96 kS/s or the audio of an upper-sideband receiver at 8 .. 48 kS/s.  The interface of the companion library
 * libnavtex_amd_tap.so (none of the other libraries is needed to use it).  It is the inverse of the narrowband interpolator
 * (navtex_amd_narrow.h), whose two kinds read exactly what the two kinds here write:
 *     252 kS/s row -> tap -> file / ear / another decoder          tap -> file -> narrow -> scan -> tune -> decode
 *
 * THE ARITHMETIC, operation by operation.  Everything is integer arithmetic; there is no float in this library's signal path.
 * The GPU result equals a restatement of this text word for word (==, no tolerance).
 *
 * Plan.  n_inputs rows of packed int16 IQ words (I in the low half) at fi = 252000 S/s; n_taps taps per input; output row
 *   input * n_taps + tap; n_inputs * n_taps <= 65535.  One output rate fo (an integer, S/s) and one kind per plan.
 * Kinds.
 *   NVX_TAP_IQ     2000 <= fo <= 96000; packed int16 IQ words out (I in the low half).
 *   NVX_TAP_REAL   audio, 8000 <= fo <= 48000; one int16 per output sample.
 * Rate.  L / M = fo / 252000 in lowest terms; supported where L * T <= 32768 (T below).
 * Shift.  Per output row, the down-converter bank's rule (navtex_amd_ddc.h) at N = 4096 and fi = 252000 on the bank's table
 *   W[j] = (c, s) = (rint(32767 cos(2 pi j / N)), rint(32767 sin(2 pi j / N))), which nvx_tap_table hands out:
 *       k = rint(hz N / fi), ties to even;  allowed where |k fi / N| <= 126000 - fp  (fp: the pass edge below)
 *       j = (k n) mod N          (n: the input's sample index since its reset;  floor modulo: 0 .. N-1)
 *       I' = clamp16((I c + Q s + 2^14) >> 15)          Q' = clamp16((Q c - I s + 2^14) >> 15)        (arithmetic shifts)
 *   k = 0 bypasses the mixer: x' = x exactly.  nvx_tap_set_shift returns the applied grid frequency k fi / N; the residue
 *   hz - applied (at most 30.8 Hz in magnitude) is the caller's to pass on, e.g. to nvx_set_carrier behind the interpolator.
 *   A new shift applies from the next call on, the carried samples included (they are kept unmixed and mixed with their
 *   true index by every call).  A reset leaves shifts and pitches alone.
 * Filter.  A plan owns T taps per phase, int32 taps h[r][t], r = 0 .. L-1, t = 0 .. T-1, and S = 21.  With x'[q] = 0 for
 *   q < 0, output n of a row since its input's reset is, per component,
 *       pos = n * M;   q = pos div L;   r = pos mod L;
 *       acc = sum over t = 0 .. T-1 of h[r][t] * x'[q - t]             (exact: it needs up to 38 bits)
 *       y = clamp16((acc + 2^20) >> 21)                                (arithmetic shift)
 *   NVX_TAP_IQ writes word[n] = (y_I & 0xffff) | (y_Q << 16).
 * Pitch (NVX_TAP_REAL only).  The complex sample (y_I, y_Q) is turned up by kp fo / N Hz and its real part is the audio:
 *       kp = rint(pitch_hz N / fo), ties to even;  allowed where 800 <= kp fo / N <= fo / 2 - 800
 *       jp = (kp m) mod N        (m: the row's output index since its input's reset);  (c, s) = W[jp]
 *       a[m] = clamp16((y_I c - y_Q s + 2^14) >> 15)
 *   Default 1000 Hz (its grid value).  The station then sits at pitch_applied + (hz - applied_hz) in the audio, its tones
 *   -+85 Hz around that in their own order: upper-sideband audio.  Nothing that survives the filter (|f| < 800 Hz) folds
 *   at 0 or fo / 2.
 * Counts.  After an input has consumed N samples in total each of its taps has produced exactly ceil(N * L / M) outputs: every
 *   n with n * M < N * L.  The output does not depend on how the input was cut into calls; calls of zero samples and of one
 *   sample count.
 * Taps.  Computed once per plan on the host (nvx_tap_design hands out the same numbers without a device), by the resampler's
 *   recipe.  Edges for IQ: pass fp = min(25000, 0.4 fo), stop fo - fp (the interpolator's band: what a tap writes is exactly
 *   what nvx_nb accepts).  Edges for REAL: pass fp = 400 Hz, stop 800 Hz, whatever fo is.  The prototype runs at L * 252000;
 *   its cut-off is the middle of the transition.  Kaiser's estimate N of the order for 90 dB and that transition;
 *   T = ceil((N + 1) / L) rounded up to even, at least 8; beta = 0.1102 (90 - 8.7); the window reaches zero half a sample
 *   beyond the ends; prototype p[k] = h[k mod L][k div L]; each phase scaled to sum 2^S, rounded, the rounding residue put
 *   on the phase's largest tap.
 *   S = 21, not the siblings' 14 or 15: a decimator's stop band stands on the taps' rounding noise, about
 *   0.29 sqrt(L T) / (L 2^S) relative to DC, and with L = 1 .. 25 and T in the hundreds or thousands int16 taps leave it at
 *   -46 .. -62 dB.  The kernel splits h = 256 hh + hl, hl in [0, 255], into two int16 operands; the design refuses a phase
 *   with Sum |h >> 8| > 65535 (arithmetic shift), so that the hh sum stays inside int32.  What holds for every supported
 *   rate and kind, and is what callers and tests may rely on:
 *     every phase sums to exactly 2^21 (a constant input c comes out as c through a tap with k = 0);   T is even;
 *     sum over t of |h[r][t]| < 2^24 for every phase, so |acc| + 2^20 < 2^24 * 2^15 + 2^20 < 2^40;
 *     sum over t of |h[r][t] >> 8| <= 65535 for every phase;
 *     response of the prototype relative to DC: within +-0.1 dB for |f| <= fp and <= -76 dB for every |f| from the stop
 *     edge up to L * 126000.
 * Supported.  The rate ranges above, L * T <= 32768; anything else is NVX_ERR_ARG at plan creation and from nvx_tap_design,
 *   with a sentence in nvx_tap_last_error().
 * Carried state.  Per input, not per tap: the last T - 1 unmixed input words live in device memory, in two rows used
 *   alternately (a launch reads one and writes the other); the 64-bit positions live on the host.  Calls on one plan are
 *   ordered by the caller: successive calls go on the same hip_stream, or are synchronised by the caller.
 *
 * Errors.  Without a HIP device nvx_tap_create returns NVX_ERR_NODEV; NULL or nonsense arguments and spans that leave their
 * allocation return NVX_ERR_ARG (checked before anything is launched); nvx_tap_last_error() has the sentence.
 * nvx_tap_design, nvx_tap_grid and nvx_tap_table need no device.
 */
#ifndef NAVTEX_AMD_TAP_H
#define NAVTEX_AMD_TAP_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_TAP_INPUT_RATE 252000
#define NVX_TAP_SHIFT 21                     /* S */
#define NVX_TAP_GRID 4096                    /* N */
#define NVX_TAP_MIN_RATE 2000
#define NVX_TAP_MAX_RATE 96000
#define NVX_TAP_MIN_AUDIO_RATE 8000
#define NVX_TAP_MAX_AUDIO_RATE 48000
#define NVX_TAP_MAX_TAPS 32768               /* L * T */
#define NVX_TAP_AUDIO_PASS_HZ 400
#define NVX_TAP_AUDIO_STOP_HZ 800
#define NVX_TAP_DEFAULT_PITCH_HZ 1000

#define NVX_TAP_IQ   0                       /* packed int16 IQ words out */
#define NVX_TAP_REAL 1                       /* one int16 of audio per sample out */

typedef struct nvx_tap nvx_tap;

typedef struct nvx_tap_config {
    uint32_t struct_size;       /* sizeof(nvx_tap_config) of the caller's header: set by nvx_tap_config_default */
    int device;                 /* 0 */
    int n_inputs;               /* 1 */
    int n_taps;                 /* 1 (n_inputs * n_taps <= 65535) */
    uint32_t output_rate_hz;    /* 12000 */
    int kind;                   /* NVX_TAP_IQ */
} nvx_tap_config;

NVX_API void nvx_tap_config_default(nvx_tap_config *cfg);
NVX_API int  nvx_tap_create(const nvx_tap_config *cfg, nvx_tap **out);
NVX_API void nvx_tap_destroy(nvx_tap *c);

/* The plan's numbers and taps for fo and kind, without a device: *L, *M, *T (each may be NULL) and, where taps is not NULL
 * and cap is large enough, the L * T taps in phase-major order taps[r * T + t].  Returns L * T (the capacity needed; with
 * taps == NULL or cap < L * T no tap is written), or NVX_ERR_ARG for a rate or kind outside the supported range. */
NVX_API int nvx_tap_design(uint32_t output_rate_hz, int kind, int *L, int *M, int *T, int32_t *taps, int cap);
/* The shift rule without a plan: *k and *applied_hz (each may be NULL) for hz at fo and kind; NVX_ERR_ARG where the rule
 * forbids it. */
NVX_API int nvx_tap_grid(uint32_t output_rate_hz, int kind, double hz, int *k, double *applied_hz);
/* W as interleaved (c, s) pairs; returns N = 4096 (the capacity needed, in pairs; nothing is written into less). */
NVX_API int nvx_tap_table(int16_t *cs, int cap_pairs);

/* The shift of tap `tap` of `input` (-1: of every input).  *applied_hz (may be NULL) receives k fi / N. */
NVX_API int nvx_tap_set_shift(nvx_tap *c, int input, int tap, double hz, double *applied_hz);
NVX_API int nvx_tap_get_shift(nvx_tap *c, int input, int tap, int *k, double *applied_hz);
/* The pitch of an NVX_TAP_REAL plan's tap (NVX_ERR_ARG on an NVX_TAP_IQ plan).  *applied_hz receives kp fo / N. */
NVX_API int nvx_tap_set_pitch(nvx_tap *c, int input, int tap, double pitch_hz, double *applied_hz);
NVX_API int nvx_tap_get_pitch(nvx_tap *c, int input, int tap, int *kp, double *applied_hz);

/* Every input of the plan, n_in samples each (at most 2^30).  d_in: [n_inputs][pitch_in_samples] packed words in device
 * memory, 4-byte aligned.  The ceil((N + n_in) L / M) - ceil(N L / M) outputs of every row (N: what its input had consumed)
 * are written to d_out[row * pitch_out_samples + out_first ...], in output samples (4-byte words for NVX_TAP_IQ, int16 for
 * NVX_TAP_REAL), aligned to their size; *n_out (may be NULL) receives their number.  All inputs must stand at the same
 * position (NVX_ERR_STATE otherwise).  Both spans are computed without wrapping and held against the allocations they lie in
 * before anything is launched (NVX_ERR_ARG, no launch).  The work is ordered on hip_stream (a hipStream_t; NULL = the null
 * stream) and NOT waited for.  n_in = 0 is valid and launches nothing. */
NVX_API int nvx_tap_resident(nvx_tap *c, const void *d_in, size_t pitch_in_samples, size_t n_in, void *d_out,
                             size_t pitch_out_samples, size_t out_first, size_t *n_out, void *hip_stream);
/* One input from host memory, all of its taps to host memory: n_in packed words at `in`; tap t's outputs at
 * out + t * cap_samples output samples (int16 pairs for NVX_TAP_IQ, ready for nvx_wav_write and nvx_nb_push; int16 for
 * NVX_TAP_REAL); *n_out (may be NULL) their number per tap.  cap_samples smaller than that: NVX_ERR_ARG, nothing consumed.
 * Returns when done. */
NVX_API int nvx_tap_push(nvx_tap *c, int input, const void *in, size_t n_in, int16_t *out, size_t cap_samples, size_t *n_out);

/* An input (-1: every input) starts anew: position 0, silence in front.  Waits for the launches still in flight. */
NVX_API int nvx_tap_reset(nvx_tap *c, int input);
/* Input samples consumed by `input` and outputs produced by each of its taps since its reset (either pointer may be NULL). */
NVX_API int nvx_tap_position(nvx_tap *c, int input, uint64_t *consumed, uint64_t *produced);
/* The plan's own numbers (each pointer may be NULL). */
NVX_API int nvx_tap_plan(nvx_tap *c, int *L, int *M, int *T, int *n_inputs, int *n_taps, int *kind);

/* HIP-event time of the tap's kernel, per call, while enabled (nvx_tap_time_stats waits for the launches still in flight). */
NVX_API int nvx_tap_timing(nvx_tap *c, int enable);
NVX_API int nvx_tap_time_stats(nvx_tap *c, double *sum_ms, uint64_t *calls, int reset);
NVX_API const char *nvx_tap_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
