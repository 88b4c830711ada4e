/* navtex_amd_afc.h -- per-chain automatic frequency control of libnavtex_amd.so (an addition to navtex_amd.h)
 *
 * A chain whose carrier is more than about 75 Hz off decodes nothing (navtex_amd_tune.h), and the radios this library is
 * fed from drift by more than that while they warm up: 1 ppm of an upconverter's 125 MHz is 125 Hz.  nvx_set_carrier
 * follows such a drift only by waiting for the handle's work in flight on every call.  These calls leave the following
 * to the GPU: behind the demodulator of every launch a small kernel turns what that launch measured of a tracking
 * chain's carrier (the sums of navtex_amd_signal.h) into the chain's k two launches on.  Nothing comes back to the
 * host for it and nothing is waited for.  Tracking is off by default, per chain; while no chain of a handle tracks, its
 * launches are what they were without this header.
 *
 * What it is for.  AFC holds a carrier the chain already has.  It does not find one: acquisition is scan -> tune
 * (navtex_amd_scan.h, navtex_amd_tune.h).  The estimate it steers by is compressed beyond +-30 Hz, where one tone nears
 * the edge of the channel filter, so a carrier further off is pulled in slowly or not at all.
 *
 * Centre.  A tracking chain's k moves about its centre kc: the chain's configured carrier, i.e. what nvx_set_carrier set
 * or its nominal k.  nvx_get_carrier keeps its meaning: it reports the centre.  nvx_set_carrier on a tracking chain moves
 * the centre and restarts tracking there.
 *
 * The law.  L counts the handle's launches; K[L] is the k a chain runs launch L with (a launch's k holds for all its
 * frames).  After nvx_afc_enable, nvx_reset, nvx_stream_reset or nvx_set_carrier the chain's next two launches run with
 * kc.  From there on, K[L+2] follows from launch L:
 *   Hold: K[L+2] = K[L+1] when the chain does not track, when its stream took no part in launch L, or when the gate fails.
 *   Gate: with the chain's record of launch L (the counts and sums of navtex_amd_signal.h over that launch alone),
 *   nb = b_samples and ny = samples - nb, the gate passes only when all of
 *     1. samples >= min_samples
 *     2. 8 nb >= samples and 8 ny >= samples                                    (both tones were seen)
 *     3. (sum_mf_hi - sum_mf_lo) >= contrast_min * (sum_mf_hi + sum_mf_lo)      (no division; false for NaN)
 *   hold.
 *   Update, the gate passed:
 *     e = (sum_dphi_b / nb + sum_dphi_y / ny) * NVX_AFC_C          (the mean of the two tones' frequencies, in k units)
 *     r = e - (double)(K[L+1] - K[L])                              (what the loop has applied since the record was taken:
 *                                                                   the two launches of delay do not ring)
 *     d = rint(ldexp(r, -gain_shift))                              (ties to even); d not finite: hold
 *     d = min(max(d, -max_step), +max_step)
 *     K[L+2] = K[L+1] + (int)d, clamped to [kc - range_k, kc + range_k] and then to +-NVX_TUNE_MAX_HZ / NVX_TUNE_STEP_HZ.
 *   Every fp64 operation is rounded on its own (no fused multiply-add), the divisions are IEEE divisions; nb and ny are
 *   converted to double exactly.  The same code runs on the device and, as nvx_afc_step_host, on the host.
 *
 * Signal reports (navtex_amd_signal.h) of a tracking chain measure offset_hz launch by launch, each launch
 * against the k that launch ran with, not against the centre.  Tracking needs the sums whether or not the user's
 * reports are on; the user's reports stay off unless nvx_enable_signal_report turned them on.
 *
 * When.  nvx_afc_enable and nvx_afc_disable take in and wait for the handle's work in flight, as nvx_set_carrier waits;
 * they apply from the stream's next launch.  The configuration (on / off, parameters, centre) survives nvx_reset and
 * nvx_stream_reset; the tracked k returns to the centre and the counters and the trace start anew, because a reset is a
 * new stream.
 *
 * Errors.  NVX_ERR_ARG: NULL handle, group or out pointer, bad stream or chain, a chain outside its stream's mask,
 * nvx_afc_config.struct_size other than this header's, a field out of range.  NVX_ERR_STATE: a wideband handle (its
 * sub-band grid is the channeliser's), or a handle that needs nvx_reset.  NVX_ERR_NODEV: no GPU (there is no handle
 * then: nvx_create reports it).  In a group, global_stream is indexed as nvx_group_poll_bits and the call goes to the
 * member that owns the stream.
 */
#ifndef NAVTEX_AMD_AFC_H
#define NAVTEX_AMD_AFC_H

#include "navtex_amd.h"
#include "navtex_amd_tune.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 900 / (4 pi 3.125): (mean delta-phi of the B samples + mean delta-phi of the Y samples) -> their mean frequency in k units */
#define NVX_AFC_C 0x1.6eb167b830193p+4
#define NVX_AFC_TRACE_KEEP 1024       /* launches the host keeps per tracking chain for nvx_afc_trace */

typedef struct nvx_afc_config {
    uint32_t struct_size;        /* sizeof(nvx_afc_config) of the caller                                   */
    int gain_shift;              /* 0 .. 4: the step is the residual error / 2^gain_shift; default 1       */
    int max_step;                /* 1 .. 64 k units a launch may move k by; default 8 (25 Hz)               */
    int range_k;                 /* 1 .. 320 k units about the centre; default 48 (+-150 Hz)                */
    int min_samples;             /* >= 0: counted samples a launch's record needs; default 256              */
    double contrast_min;         /* 0 .. 1: matched-filter contrast the record needs; default 0.7 (noise    */
                                 /* alone measures 0.49, carriers 0.85 and more)                            */
} nvx_afc_config;

typedef struct nvx_afc_status {
    int enabled;                 /* the chain tracks                                                        */
    int centre_k;                /* kc                                                                      */
    int k_last;                  /* the k the newest collected launch of the chain ran with (kc before one) */
    int last_step;               /* K[L+2] - K[L+1] that launch decided                                     */
    double offset_hz;            /* k_last * NVX_TUNE_STEP_HZ                                               */
    uint64_t launches;           /* collected launches the chain took part in while tracking                */
    uint64_t updates;            /* ... whose gate passed (d finite)                                        */
    uint64_t held;               /* ... whose gate refused (or d was not finite)                            */
    uint64_t clamped;            /* ... where max_step or a range limit cut the step                        */
} nvx_afc_status;

NVX_API void nvx_afc_config_default(nvx_afc_config *cfg);
/* Track (stream, chain) about its centre; cfg NULL = the defaults.  On a chain that tracks already: new parameters, and
 * tracking restarts at the centre. */
NVX_API int nvx_afc_enable(nvx_handle *h, int stream, int chain, const nvx_afc_config *cfg);
/* Stop tracking.  keep != 0: the tracked k (what the chain's next launch would have run with) becomes the chain's
 * configured carrier; keep == 0: the chain returns to its centre.  Not tracking: nothing happens. */
NVX_API int nvx_afc_disable(nvx_handle *h, int stream, int chain, int keep);
/* Takes in finished launches without waiting (as nvx_signal_report_read), then fills *out. */
NVX_API int nvx_afc_read(nvx_handle *h, int stream, int chain, nvx_afc_status *out);
/* The k every collected launch ran with, for the launches the chain took part in while tracking since the previous call
 * (finished launches are taken in first, without waiting), oldest first, at most cap of them (the rest stay for the
 * next call); the host keeps the last NVX_AFC_TRACE_KEEP launches.  Returns how many were written, or an error (< 0). */
NVX_API int nvx_afc_trace(nvx_handle *h, int stream, int chain, int32_t *k, size_t cap);

NVX_API int nvx_group_afc_enable(nvx_group *g, int global_stream, int chain, const nvx_afc_config *cfg);
NVX_API int nvx_group_afc_disable(nvx_group *g, int global_stream, int chain, int keep);
NVX_API int nvx_group_afc_read(nvx_group *g, int global_stream, int chain, nvx_afc_status *out);
NVX_API int nvx_group_afc_trace(nvx_group *g, int global_stream, int chain, int32_t *k, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
