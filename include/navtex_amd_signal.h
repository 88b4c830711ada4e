/* navtex_amd_signal.h -- per-chain signal reports of libnavtex_amd.so (an addition to navtex_amd.h)
 *
 * A chain that yields no messages looks the same whether its station is off the air, the radio is dead, the radio has
 * drifted off frequency or the station is too weak.  A signal report tells these apart: the level at the demodulator's
 * input, where the carrier sits against its nominal frequency, and how open the discriminator's eye is.  The GPU sums
 * what the demodulator computes anyway; reports are off by default and change no bit and no message.
 *
 * Definition.  For one decoded (stream, chain), every 900 S/s sample t of every COLLECTED launch whose index g since the
 * stream's reset is >= 8 counts once (a stream's last, ragged launch: the samples it really had).  Per sample:
 *   P      = I*I + Q*Q of the channel filter's output y3 (fp64)
 *   phi    = the discriminator's delta-phi (radians per sample)
 *   d      = the mark/space decision of the five-sample window ENDING at t ('B' = 1; 'B' is the upper tone)
 *   hi, lo = the larger and the smaller of that window's two matched-filter energies
 * The record holds the count and the raw sums, so that reports can be merged; the derived fields are computed from
 * them in double and are NaN where their denominator is 0:
 *   power_db   = 10 log10(sum_power / samples)          (y3 units: comparable between handles of one rate and stage 0)
 *   b_hz, y_hz = class mean of phi * 900 / (2 pi)        (each tone's frequency against the chain's nominal carrier)
 *   offset_hz  = (b_hz + y_hz) / 2                       (the carrier's distance from its nominal frequency)
 *   shift_hz   = b_hz - y_hz                             (NAVTEX: positive, somewhat below 170: transitions pull inward)
 *   eye_snr_db = 10 log10(((muB - muY) / 2)^2 / ((varB + varY) / 2)), population variances of phi, clamped at 0
 *   contrast   = (sum_mf_hi - sum_mf_lo) / (sum_mf_hi + sum_mf_lo), in [0, 1]
 *
 * A chain under automatic frequency control (navtex_amd_afc.h) is measured launch by launch, each launch against the k
 * that launch ran with: its offset_hz is what the loop has not removed yet, not the carrier's distance from the centre.
 */
#ifndef NAVTEX_AMD_SIGNAL_H
#define NAVTEX_AMD_SIGNAL_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nvx_signal_report {
    /* counts and raw sums over the counted samples */
    uint64_t samples;            /* n                                    */
    uint64_t b_samples;          /* samples with d = 1                   */
    double sum_power;            /* sum P                                */
    double sum_dphi_b;           /* sum phi over samples with d = 1      */
    double sum_dphi2_b;          /* sum phi^2 over samples with d = 1    */
    double sum_dphi_y;           /* sum phi over samples with d = 0      */
    double sum_dphi2_y;          /* sum phi^2 over samples with d = 0    */
    double sum_mf_hi;            /* sum hi                               */
    double sum_mf_lo;            /* sum lo                               */
    /* derived (above) */
    double power_db, b_hz, y_hz, offset_hz, shift_hz, eye_snr_db, contrast;
} nvx_signal_report;

/* Reports on (on != 0) or off.  Waits for the handle's work in flight first (as nvx_enable_debug), so a report covers
 * whole launches: those launched while reports were on.  Off frees the buffers and drops every report.  Costs, while on,
 * one 64-byte record per chain and launch copied back with the bits (about 0.5 MB per launch at 8192 chains).          */
NVX_API int nvx_enable_signal_report(nvx_handle *h, int on);
/* The report of decoded stream `stream` (indexed as nvx_poll_bits), chain 0 (518) or 1 (490): takes in finished launches
 * without waiting (as nvx_poll), then fills *out; reset != 0 starts the report anew.  A chain outside its stream's mask
 * reports samples = 0.  nvx_stream_reset clears the stream's reports, nvx_reset every report.
 * NVX_ERR_ARG: NULL handle or out, bad stream or chain; NVX_ERR_STATE: reports off, or the handle needs nvx_reset.     */
NVX_API int nvx_signal_report_read(nvx_handle *h, int stream, int chain, nvx_signal_report *out, int reset);

#ifdef __cplusplus
}
#endif
#endif
