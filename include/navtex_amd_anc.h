/* navtex_amd_anc.h -- antenna noise canceller: two coherent rows of IQ (a main antenna and a sense antenna) at any rate and
 * in any of the resampler's sample formats -> one row of packed int16 IQ at the same rate, with what the two rows share
 * subtracted from the main row.  The interface of the companion library libnavtex_amd_anc.so (none of the other libraries
 * is needed to use it).
 *
 * Local broadband noise (switching supplies, PLC, LED drivers, plasma screens) lies 20 to 30 dB above an MF station and
 * nothing behind one antenna removes it.  A second, coherent receiver on a sense antenna that hears the local noise well and
 * the station badly delivers the same noise with another amplitude and phase; the sense row times the complex weight
 * c = sum(a conj b) / sum(b conj b) is the part of the main row the two have in common, and it is subtracted.  (Two coherent
 * dongles, a two-channel direct-sampling ADC, or the second tuner of a two-tuner radio give the pair of rows.)  The canceller
 * sits between the IQ corrector and the blanker:
 *     IQ-correct (each row) -> cancel -> blank -> DDC / resample -> scan -> tune -> decode
 * It has no notion of rate: everything below is in samples.
 *
 * THE ARITHMETIC, operation by operation.  Integer arithmetic except the one float32 conversion of CF32 input; every shift
 * and every division below is a floor shift or floor division of signed 64-bit integers.  The GPU result equals a
 * restatement of this text word for word (==, no tolerance), whatever way the input is cut into calls.
 *
 * Conversion.  Exactly as in navtex_amd_iqc.h, per component, to an integer in the int16 range:
 *   NVX_ANC_CS16   int16:    the value itself
 *   NVX_ANC_CU8    uint8 u:  (2 u - 255) * 128
 *   NVX_ANC_CS8    int8 s:   s * 256
 *   NVX_ANC_CF32   float f:  y = f * 32768 in float32, rounded to the nearest integer with ties to even, clamped to
 *                            [-32768, 32767]; NaN -> 0
 *   One plan has one format for both rows.  a[n] = (I1, Q1) is the main row, b[n] = (I2, Q2) the sense row; n counts a
 *   pair's samples since its reset.  Samples are interleaved I, Q in every format.
 * Blocks.      NVX_ANC_BLOCK = 65536 samples by absolute index, block = n div 65536.  A block has four exact sums in int64:
 *   SAA = sum (I1^2 + Q1^2)       SBB = sum (I2^2 + Q2^2)
 *   SRE = sum (I1 I2 + Q1 Q2)     SIM = sum (Q1 I2 - I1 Q2)
 *   SRE and SIM are the real and imaginary part of sum a conj(b).  Each term is at most 2^31, each block sum at most 2^47.
 * Window.      W = 4, 16 or 64 blocks (window_log2 = 2, 4 or 6; default 2), N = W * 65536 = 2^(16 + window_log2) samples.
 *   TAA, TBB, TRE, TIM are the sums over the last W complete blocks (at most 2^53).  Nothing is cancelled before the first
 *   window is complete: with W = 16 at 252 kS/s that is 4.2 s, in which a message's start is lost; hence the default.
 * Solve.       At the first sample of every block in front of which W blocks are complete since the reset (from a reset at
 *   0: every block >= W), in NVX_ANC_TRACK mode:
 *    1. if TBB < 16 N: c = (0, 0), coherence 0, reason 1: the sense row is silent
 *    2. s = max(0, bitlength(max(TAA, TBB)) - 30);  taa, tbb, tre, tim = TAA >> s, TBB >> s, TRE >> s, TIM >> s
 *       (taa, tbb < 2^30; |tre|, |tim| <= 2^30, as |sum a conj b| <= max(TAA, TBB))
 *    3. if tbb < 1024: c = (0, 0), coherence 0, reason 2: the sense row lies 60 dB under the main row
 *    4. c_re = floor((tre * 16384 + tbb) / (2 tbb)),  c_im = floor((tim * 16384 + tbb) / (2 tbb))
 *       (Q13, rounded; the numerators stay below 2^45)
 *    5. den = (taa * tbb) >> 14 (taa tbb < 2^60);  coherence = den > 0 ? min(16384, floor((tre^2 + tim^2) / den)) : 0
 *       (Q14; tre^2 + tim^2 <= 2^61).  It is the share of the main row's power that the two rows have in common.  It is
 *       reported only and gates nothing.
 *    6. if max(|c_re|, |c_im|) > 32767: c = (0, 0), reason 3: more than 12 dB of gain would be needed (the coherence of
 *       step 5 stays).  Otherwise c = (c_re, c_im), reason 0.
 *   A reason other than 0 counts a rejected block; reason 0 counts a solved one.
 * Apply.       p = c_re I2 - c_im Q2 + 4096,  r = c_re Q2 + c_im I2 + 4096
 *   (|p|, |r| <= 2 * 32767 * 32768 + 4096 < 2^31: that is why the limit is 32767 and not 32768)
 *   outI = clamp16(I1 - (p >> 13)),  outQ = clamp16(Q1 - (r >> 13));  out[n] = (outI & 0xffff) | (outQ << 16).
 *   c = (0, 0) gives the main row's conversion word for word.
 * Until W blocks are complete, and in NVX_ANC_HOLD mode, the weight stays what it is: (0, 0) after create or reset, the last
 *   solved or set one otherwise.  In NVX_ANC_HOLD mode the sums go on.
 * A pair's output does not depend on how its input was cut into calls.
 * Carried state.  Per pair, in device memory, in two rows used alternately (a launch reads one and writes the other): the
 *   ring of the last W block sums, the open block's partial sums, the blocks complete since the reset saturated at W, c_re
 *   and c_im, the coherence of the last solve, the mode and the last reason.  The 64-bit position lives on the host.  Calls
 *   on one plan are ordered by the caller: successive calls go on the same hip_stream, or are synchronised by the caller.
 * Known limits.
 *   (a) It is one complex weight for the whole row.  Noise that reaches the two antennas with a delay difference tau is
 *       nulled to about 20 log10(2 pi f tau) at offset f from the row's centre.  For antennas a few tens of metres apart
 *       that is 30 dB or more at +-14 kHz.  A narrower row nulls deeper.  The two rows must be sample-aligned: rows that start
 *       any number of samples apart (two dongles on one clock) go through the row aligner first (navtex_amd_align.h), which
 *       measures the delay and removes it to 1/32 sample.
 *       Noise that arrives with echoes or over a frequency response wants more than one weight: the multi-tap canceller
 *       (navtex_amd_wanc.h) puts a short complex FIR on the sense row.
 *   (b) It is blind: it cancels the strongest component the two rows share.  A station that is itself that component is
 *       taken down to about the level of the sense row's own noise (DESIGN 3.14 has figures).  NVX_ANC_HOLD and nvx_anc_set
 *       are for calibrated set-ups, and the coherence tells the caller which case it is in.
 *   (c) A DC offset on both rows is a common component.  Take it out first, which the IQ corrector does.
 *   (d) It subtracts what the two rows share and cannot add it: a station that fades on two antennas at different times is
 *       the diversity combiner's (navtex_amd_div.h), which co-phases the two rows per station and adds them.
 * Cost.  Both rows are read twice and 4 bytes written per sample (CS16: 20 bytes per pair-sample against the IQ corrector's
 *   12 per sample).
 *
 * Errors.  Without a HIP device nvx_anc_create returns NVX_ERR_NODEV; NULL or nonsense arguments, spans that leave their
 * allocation and an output that overlaps an input return NVX_ERR_ARG (checked before anything is launched);
 * nvx_anc_last_error() has the sentence.
 */
#ifndef NAVTEX_AMD_ANC_H
#define NAVTEX_AMD_ANC_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_ANC_BLOCK 65536                  /* samples per block */
#define NVX_ANC_WINDOW_LOG2_DEFAULT 2        /* W = 4 blocks; 4 and 6 are the other values */
#define NVX_ANC_C_ONE 8192                   /* 1.0 in Q13 */
#define NVX_ANC_C_MAX 32767                  /* |c_re|, |c_im| of a solved or set weight: just under 4.0 */
#define NVX_ANC_COHERENCE_ONE 16384          /* 1.0 in Q14 */

#define NVX_ANC_TRACK 0                      /* solve at every block start once the window is full */
#define NVX_ANC_HOLD 1                       /* keep the weight; the sums go on */

#define NVX_ANC_CS16 0                       /* int16 I, Q      (4 bytes per sample) */
#define NVX_ANC_CU8  1                       /* uint8 I, Q      (2 bytes per sample) */
#define NVX_ANC_CS8  2                       /* int8 I, Q       (2 bytes per sample) */
#define NVX_ANC_CF32 3                       /* float32 I, Q    (8 bytes per sample) */

typedef struct nvx_noise_canceller nvx_noise_canceller;

typedef struct nvx_anc_config {
    uint32_t struct_size;       /* sizeof(nvx_anc_config) of the caller's header: set by nvx_anc_config_default */
    int device;                 /* 0 */
    int format;                 /* NVX_ANC_CS16, of both rows */
    int n_pairs;                /* 1 */
    int window_log2;            /* 2 */
} nvx_anc_config;

/* What nvx_anc_get returns about one pair. */
typedef struct nvx_anc_status {
    int32_t c_re, c_im;         /* the current weight (Q13): that of the pair's last sample, or set since */
    int32_t mode;               /* NVX_ANC_TRACK or NVX_ANC_HOLD */
    int32_t last_reason;        /* of the last block solved or rejected since the reset: 0 .. 3 */
    int32_t coherence_q14;      /* of that block: step 5 */
    int32_t reserved;           /* 0 */
    int64_t sums[4];            /* TAA, TBB, TRE, TIM over the complete blocks of the window */
    uint64_t samples;           /* consumed since creation */
    uint64_t blocks_solved;     /* block starts with reason 0 since creation */
    uint64_t blocks_rejected;   /* ... with another reason */
} nvx_anc_status;

NVX_API void nvx_anc_config_default(nvx_anc_config *cfg);
NVX_API int  nvx_anc_create(const nvx_anc_config *cfg, nvx_noise_canceller **out);
NVX_API void nvx_anc_destroy(nvx_noise_canceller *c);

/* Every pair of the plan, n_in samples each (at most 2^30).  d_main: [n_pairs][pitch_main_samples] samples in the plan's
 * format in device memory, 16-byte aligned, every row 16-byte aligned (pitch_main_samples times the sample size a multiple of
 * 16 where n_pairs > 1); d_sense with pitch_sense_samples likewise.  The n_in words of every pair are written (I in the low
 * half) to d_out[pair * pitch_out_samples + out_first ...], 4-byte aligned.  Where every row's first word is 16-byte aligned
 * (the address of d_out[out_first], and with more than one pair pitch_out_samples a multiple of 4) they are written with
 * aligned 16-byte non-temporal stores; otherwise the same words go out unaligned, slower.  All pairs must stand at the same
 * position (NVX_ERR_STATE otherwise).  All three spans are computed without wrapping and held against the allocations they
 * lie in before anything is launched, and the output span (from the first word written to the last, the gaps between its
 * rows included) must overlap neither input span (NVX_ERR_ARG, no launch).  The work is ordered on hip_stream (a
 * hipStream_t; NULL = the null stream) and NOT waited for.  n_in = 0 is valid and launches nothing. */
NVX_API int nvx_anc_resident(nvx_noise_canceller *c, const void *d_main, size_t pitch_main_samples, const void *d_sense,
                             size_t pitch_sense_samples, size_t n_in, void *d_out, size_t pitch_out_samples, size_t out_first,
                             void *hip_stream);
/* One pair from host memory to host memory: n_in samples in the plan's format at `main_in` and at `sense_in`, n_in samples of
 * interleaved int16 (I, Q) to out_iq.  Returns when done. */
NVX_API int nvx_anc_push(nvx_noise_canceller *c, int pair, const void *main_in, const void *sense_in, size_t n_in, int16_t *out_iq);

/* A pair (-1: every pair) starts anew: position 0, no block complete, the weight (0, 0), coherence and reason 0.  Its mode
 * and counters stay.  Waits for the launches still in flight, as the three calls below do. */
NVX_API int nvx_anc_reset(nvx_noise_canceller *c, int pair);
/* The weight of `pair` (-1: every pair) from the next call's first sample on: c_re and c_im within +-NVX_ANC_C_MAX.  In
 * NVX_ANC_TRACK mode the next solve replaces it. */
NVX_API int nvx_anc_set(nvx_noise_canceller *c, int pair, int c_re, int c_im);
/* NVX_ANC_TRACK or NVX_ANC_HOLD for `pair` (-1: every pair) from the next call's first sample on. */
NVX_API int nvx_anc_set_mode(nvx_noise_canceller *c, int pair, int mode);
NVX_API int nvx_anc_get(nvx_noise_canceller *c, int pair, nvx_anc_status *out);
/* Samples consumed by `pair` since its reset. */
NVX_API int nvx_anc_position(nvx_noise_canceller *c, int pair, uint64_t *consumed);
/* The plan's own numbers (each pointer may be NULL). */
NVX_API int nvx_anc_plan(nvx_noise_canceller *c, int *format, int *n_pairs, int *window_log2);

/* HIP-event time of the canceller's two kernels, per call, while enabled (nvx_anc_time_stats waits for the launches still
 * in flight). */
NVX_API int nvx_anc_timing(nvx_noise_canceller *c, int enable);
NVX_API int nvx_anc_time_stats(nvx_noise_canceller *c, double *sum_ms, uint64_t *calls, int reset);
NVX_API const char *nvx_anc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
