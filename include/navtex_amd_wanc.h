/* navtex_amd_wanc.h -- multi-tap antenna noise canceller: two coherent rows of IQ (a main antenna and a sense antenna) at
 * any rate and in any of the resampler's sample formats -> one row of packed int16 IQ at the same rate, with a short complex
 * FIR of the sense row subtracted from the main row.  The interface of the companion library libnavtex_amd_wanc.so (none of
 * the other libraries is needed to use it).
 *
 * The single-weight canceller (navtex_amd_anc.h) is right at one frequency.  Local noise reaches the two antennas over paths
 * that differ in more than a gain, a phase and one delay: it arrives with echoes and with a frequency response (a loop against
 * a whip, mains wiring that re-radiates, two receivers' different filters), and a 252 kS/s row carries 490 and 518 at +-14 kHz,
 * 0.7 rad of phase apart per sample of path difference.  K complex weights on K successive sense samples follow such a path;
 * they are the least-squares solution of the window's normal equations.  The place in the chain:
 *     IQ-correct (each row) -> align -> multi-tap cancel -> blank -> notch -> DDC / resample -> scan -> tune -> decode
 * in place of the single-weight canceller, which stays the cheaper tool for a true two-channel ADC on one antenna pair.  It has
 * no notion of rate: everything below is in samples.
 *
 * THE ARITHMETIC, operation by operation.  Integer arithmetic except the one float32 conversion of CF32 input and the fp64
 * solve; every shift below is a floor shift of signed integers.  The GPU result equals a restatement of this text word for
 * word (==, no tolerance), whatever way the input is cut into calls.
 *
 * Conversion.  Exactly as in navtex_amd_anc.h, per component, to an integer in the int16 range:
 *   NVX_WANC_CS16  int16:    the value itself
 *   NVX_WANC_CU8   uint8 u:  (2 u - 255) * 128
 *   NVX_WANC_CS8   int8 s:   s * 256
 *   NVX_WANC_CF32  float f:  y = f * 32768 in float32, rounded to the nearest integer with ties to even, clamped to
 *                            [-32768, 32767]; NaN -> 0
 *   One plan has one format for both rows.  a[n] = (I1, Q1) is the main row, b[n] = (I2, Q2) the sense row; n is a pair's
 *   position: its samples since its reset.  a[n] = b[n] = 0 in front of the reset.  Samples are interleaved I, Q.
 * Taps.        K = n_taps = 4, 8 or 16 (default 8), G = K / 2.  The weights w_0 .. w_(K-1) are complex Q13 integers.
 * Apply.       The output is the main row delayed by G samples, less the filtered sense row:
 *   p = sum_k (w_re,k I2[n-k] - w_im,k Q2[n-k]) + 4096,   r = sum_k (w_re,k Q2[n-k] + w_im,k I2[n-k]) + 4096   (k = 0 .. K-1)
 *   outI = clamp16(I1[n-G] - (p >> 13)),  outQ = clamp16(Q1[n-G] - (r >> 13));  out[n] = (outI & 0xffff) | (outQ << 16).
 *   Bounds: every weight component lies within +-32767 and L1 = sum_k (|w_re,k| + |w_im,k|) <= NVX_WANC_L1_MAX = 65534, so
 *   |p|, |r| and every partial sum of them stay within 65534 * 32768 + 4096 = 2^31 - 61440 < 2^31: the sums are exact in
 *   32 bits in any order.  Every call writes as many words as it reads.  Zero weights give the main row's conversion
 *   delayed by G, word for word.
 * Blocks.      NVX_WANC_BLOCK = 65536 samples by position, block = n div 65536.  With x conj(y) = (Ix Iy + Qx Qy,
 *   Qx Iy - Ix Qy), a block has 4 K + 1 exact sums in int64 over its n:
 *   r[d] = sum b[n] conj(b[n-d]), d = 0 .. K-1  (the imaginary part of r[0] is 0 and is carried as such)
 *   q[k] = sum a[n-G] conj(b[n-k]), k = 0 .. K-1
 *   SAA  = sum (I1[n-G]^2 + Q1[n-G]^2)
 *   They are taken on the full 16-bit components.  A real part lies within -2^31 + 65536 .. 2^31 (2^31 only where all four
 *   components are -32768), an imaginary part within +-(2^31 - 32768); a block sum within +-2^47, a window sum within +-2^53.
 * Window.      W = 4, 16 or 64 blocks (window_log2 = 2, 4 or 6; default 2), N = W * 65536 samples.  R[d], Q[k], TAA are the
 *   sums over the last W complete blocks.  Nothing is cancelled before the first window is complete.
 * Solve.       At the first sample of every block in front of which W blocks are complete since the reset, in
 *   NVX_WANC_TRACK mode.  fp64 is IEEE binary64, round to nearest even; every product, sum, difference and quotient below is
 *   rounded on its own (no fused multiply-add); the order is the written one, sums from left to right.
 *    1. R0 = Re R[0].  If R0 < 16 N: reason 1, the sense row is silent.
 *    2. lambda = (R0 >> load_log2) + 1 in integers (load_log2 = 8 .. 20, default 12).  diag = fp64(R0 + lambda), the sum in
 *       integers.  rr[d], ri[d], qr[k], qi[k] = fp64 of Re R[d], Im R[d], Re Q[k], Im Q[k] (exact: |.| <= 2^53).  The matrix
 *       is T[j][j] = diag, T[i][j] = (rr[i-j], ri[i-j]) for i > j, and its conjugate above the diagonal.
 *    3. T = L D L^H, column by column, j = 0 .. K-1:
 *         s = diag;  for m = 0 .. j-1:  s = s - (Lr[j][m] Lr[j][m] + Li[j][m] Li[j][m]) * d[m]
 *         d[j] = s.  Unless 0 < s < infinity: reason 2.   e[j] = 1.0 / s
 *         for i = j+1 .. K-1:  (sr, si) = (rr[i-j], ri[i-j])
 *            for m = 0 .. j-1:  ur = Lr[i][m] Lr[j][m] + Li[i][m] Li[j][m],  ui = Li[i][m] Lr[j][m] - Lr[i][m] Li[j][m]
 *                               sr = sr - ur * d[m],  si = si - ui * d[m]
 *            Lr[i][j] = sr * e[j],  Li[i][j] = si * e[j]
 *    4. L z = Q, j = 0 .. K-1:  (zr, zi) = (qr[j], qi[j]);  for m = 0 .. j-1:
 *            zr = zr - (Lr[j][m] zr[m] - Li[j][m] zi[m]),  zi = zi - (Lr[j][m] zi[m] + Li[j][m] zr[m])
 *       (zr[j], zi[j]) = (zr, zi);  then y[j] = (zr[j] * e[j], zi[j] * e[j])
 *    5. L^H x = y, j = K-1 .. 0:  (xr, xi) = y[j];  for i = j+1 .. K-1:
 *            xr = xr - (Lr[i][j] xr[i] + Li[i][j] xi[i]),  xi = xi - (Lr[i][j] xi[i] - Li[i][j] xr[i])
 *    6. coherence: c = 0;  for k = 0 .. K-1:  c = c + (xr[k] qr[k] + xi[k] qi[k]).  v = (16384.0 * c) / fp64(TAA) where
 *       TAA > 0.  coherence = 0 where TAA = 0 or not v >= 1, 16384 where v >= 16384, the integer part of v otherwise (Q14).  It
 *       is the share of the delayed main row's power that the filtered sense row explains; reported only, it gates nothing.
 *    7. w_re,k = rint(8192.0 * xr[k]), w_im,k = rint(8192.0 * xi[k]) (to the nearest integer, ties to even).  If a component
 *       is not within +-32767 (a NaN is not), or L1 > 65534: reason 3, the coherence of step 6 stays.  The first bound lets a
 *       weight and its negation stand in an int16 half of a dot-product operand; the second is the apply's.
 *   A reason other than 0 sets all weights to zero and counts a rejected block (reasons 1 and 2 with coherence 0); reason 0
 *   counts a solved one.
 * Until W blocks are complete, and in NVX_WANC_HOLD mode, the weights stay what they are: zero after create or reset, the
 *   last solved or set ones otherwise.  In NVX_WANC_HOLD mode the sums go on.
 * A pair's output does not depend on how its input was cut into calls.
 * Carried state.  Per pair, in device memory, in two rows used alternately (a launch reads one and writes the other): the
 *   ring of the last W blocks' sums, the open block's partial sums, the blocks complete since the reset saturated at W, the K
 *   weights, the coherence of the last solve, the mode and the last reason, the last K - 1 converted sense words and the last
 *   G converted main words.  The 64-bit position lives on the host.  Calls on one plan are ordered by the caller.
 * Known limits.
 *   (a) It is still blind (the canceller's limit (b)): it cancels what the two rows share, a strong station included.
 *       NVX_WANC_HOLD, nvx_wanc_set and the coherence are for that.
 *   (b) Loading caps the null.  On pure common noise with no echoes the null is about -70 dB at load_log2 = 12 and -76 dB at
 *       16, against the single-weight canceller's -76 dB (DESIGN 3.18 has the figures).
 *   (c) K taps reach echoes up to K/2 - 1 samples to either side.  Bulk delay belongs to the aligner (navtex_amd_align.h).
 *   (d) A window in which the path changes solves to a compromise.
 *   (e) The matrix is the Toeplitz one of r[d]: the few products at a window's edges that a full covariance matrix would
 *       place differently are not told apart.
 *   (f) It subtracts what the two rows share and cannot add it: a station that fades on two antennas at different times is
 *       the diversity combiner's (navtex_amd_div.h), which co-phases the two rows per station and adds them.
 * Cost.  Both rows are read twice and 4 bytes written per sample, as in navtex_amd_anc.h; 4 K + 1 sums per sample in the
 *   first pass and 2 K dot products in the second.
 *
 * Errors.  Without a HIP device nvx_wanc_create returns NVX_ERR_NODEV; NULL or nonsense arguments, spans that leave their
 * allocation and an output that overlaps an input return NVX_ERR_ARG (checked before anything is launched);
 * nvx_wanc_last_error() has the sentence.
 */
#ifndef NAVTEX_AMD_WANC_H
#define NAVTEX_AMD_WANC_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_WANC_BLOCK 65536                 /* samples per block */
#define NVX_WANC_WINDOW_LOG2_DEFAULT 2       /* W = 4 blocks; 4 and 6 are the other values */
#define NVX_WANC_TAPS_DEFAULT 8              /* K; 4 and 16 are the other values */
#define NVX_WANC_TAPS_MAX 16
#define NVX_WANC_LOAD_LOG2_DEFAULT 12        /* 8 .. 20 */
#define NVX_WANC_W_ONE 8192                  /* 1.0 in Q13 */
#define NVX_WANC_W_MAX 32767                 /* |w_re,k|, |w_im,k| */
#define NVX_WANC_L1_MAX 65534                /* sum of |w_re,k| + |w_im,k| over the K taps */
#define NVX_WANC_COHERENCE_ONE 16384         /* 1.0 in Q14 */

#define NVX_WANC_TRACK 0                     /* solve at every block start once the window is full */
#define NVX_WANC_HOLD 1                      /* keep the weights; the sums go on */

#define NVX_WANC_CS16 0                      /* int16 I, Q      (4 bytes per sample) */
#define NVX_WANC_CU8  1                      /* uint8 I, Q      (2 bytes per sample) */
#define NVX_WANC_CS8  2                      /* int8 I, Q       (2 bytes per sample) */
#define NVX_WANC_CF32 3                      /* float32 I, Q    (8 bytes per sample) */

typedef struct nvx_wide_canceller nvx_wide_canceller;

typedef struct nvx_wanc_config {
    uint32_t struct_size;       /* sizeof(nvx_wanc_config) of the caller's header: set by nvx_wanc_config_default */
    int device;                 /* 0 */
    int format;                 /* NVX_WANC_CS16, of both rows */
    int n_pairs;                /* 1 */
    int window_log2;            /* 2 */
    int n_taps;                 /* 8 */
    int load_log2;              /* 12 */
} nvx_wanc_config;

/* What nvx_wanc_get returns about one pair.  Entries from n_taps on are zero. */
typedef struct nvx_wanc_status {
    int32_t n_taps;             /* K */
    int32_t mode;               /* NVX_WANC_TRACK or NVX_WANC_HOLD */
    int32_t last_reason;        /* of the last block solved or rejected since the reset: 0 .. 3 */
    int32_t coherence_q14;      /* of that block: step 6 */
    int32_t w_re[NVX_WANC_TAPS_MAX], w_im[NVX_WANC_TAPS_MAX];   /* the current weights (Q13) */
    int64_t r_re[NVX_WANC_TAPS_MAX], r_im[NVX_WANC_TAPS_MAX];   /* R[d] over the complete blocks of the window */
    int64_t q_re[NVX_WANC_TAPS_MAX], q_im[NVX_WANC_TAPS_MAX];   /* Q[k] */
    int64_t saa;                /* TAA */
    uint64_t samples;           /* consumed since creation */
    uint64_t blocks_solved;     /* block starts with reason 0 since creation */
    uint64_t blocks_rejected;   /* ... with another reason */
} nvx_wanc_status;

NVX_API void nvx_wanc_config_default(nvx_wanc_config *cfg);
NVX_API int  nvx_wanc_create(const nvx_wanc_config *cfg, nvx_wide_canceller **out);
NVX_API void nvx_wanc_destroy(nvx_wide_canceller *c);

/* Every pair of the plan, n_in samples each (at most 2^30): the arguments and rules of nvx_anc_resident.  d_main:
 * [n_pairs][pitch_main_samples] samples in the plan's format in device memory, 16-byte aligned, every row 16-byte aligned;
 * d_sense with pitch_sense_samples likewise.  The n_in words of every pair are written (I in the low half) to
 * d_out[pair * pitch_out_samples + out_first ...], 4-byte aligned; with aligned 16-byte non-temporal stores where every row's
 * first word is 16-byte aligned.  All pairs must stand at the same position (NVX_ERR_STATE otherwise).  All three spans are
 * computed without wrapping and held against the allocations they lie in before anything is launched, and the output span
 * must overlap neither input span (NVX_ERR_ARG, no launch).  The work is ordered on hip_stream (a hipStream_t; NULL = the
 * null stream) and NOT waited for.  n_in = 0 is valid and launches nothing. */
NVX_API int nvx_wanc_resident(nvx_wide_canceller *c, const void *d_main, size_t pitch_main_samples, const void *d_sense,
                              size_t pitch_sense_samples, size_t n_in, void *d_out, size_t pitch_out_samples, size_t out_first,
                              void *hip_stream);
/* One pair from host memory to host memory: n_in samples in the plan's format at `main_in` and at `sense_in`, n_in samples of
 * interleaved int16 (I, Q) to out_iq.  Returns when done. */
NVX_API int nvx_wanc_push(nvx_wide_canceller *c, int pair, const void *main_in, const void *sense_in, size_t n_in, int16_t *out_iq);

/* A pair (-1: every pair) starts anew: position 0, no block complete, zero weights, silence in front, coherence and reason 0.
 * Its mode and counters stay.  Waits for the launches still in flight, as the three calls below do. */
NVX_API int nvx_wanc_reset(nvx_wide_canceller *c, int pair);
/* The n_taps weights of `pair` (-1: every pair) from the next call's first sample on: w_re[k], w_im[k] within
 * +-NVX_WANC_W_MAX and their L1 sum at most NVX_WANC_L1_MAX.  In NVX_WANC_TRACK mode the next solve replaces them. */
NVX_API int nvx_wanc_set(nvx_wide_canceller *c, int pair, const int32_t *w_re, const int32_t *w_im);
/* NVX_WANC_TRACK or NVX_WANC_HOLD for `pair` (-1: every pair) from the next call's first sample on. */
NVX_API int nvx_wanc_set_mode(nvx_wide_canceller *c, int pair, int mode);
NVX_API int nvx_wanc_get(nvx_wide_canceller *c, int pair, nvx_wanc_status *out);
/* Samples consumed by `pair` since its reset. */
NVX_API int nvx_wanc_position(nvx_wide_canceller *c, int pair, uint64_t *consumed);
/* The plan's own numbers (each pointer may be NULL). */
NVX_API int nvx_wanc_plan(nvx_wide_canceller *c, int *format, int *n_pairs, int *window_log2, int *n_taps, int *load_log2);

/* HIP-event time of the canceller's three kernels, per call, while enabled (nvx_wanc_time_stats waits for the launches
 * still in flight). */
NVX_API int nvx_wanc_timing(nvx_wide_canceller *c, int enable);
NVX_API int nvx_wanc_time_stats(nvx_wide_canceller *c, double *sum_ms, uint64_t *calls, int reset);
NVX_API const char *nvx_wanc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
