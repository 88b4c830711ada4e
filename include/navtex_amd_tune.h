/* navtex_amd_tune.h -- per-chain carrier tuning of libnavtex_amd.so (an addition to navtex_amd.h)
 *
 * Every chain mixes its carrier down from a fixed place: chain 0 ("518") from +14 kHz, chain 1 ("490") from -14 kHz of
 * its stream's centre -- the reference's wiring for a tuner at 504 kHz.  A radio whose frequency error moves the
 * carrier more than about 75 Hz, a tuner at another frequency or a station elsewhere in the band decodes nothing
 * there.  These calls move a chain's carrier anywhere within +-25 kHz of the stream's centre.
 *
 * Grid.  A chain's carrier offset is k * NVX_TUNE_STEP_HZ (3.125 Hz = 63 000 / 20 160), k an integer; a requested
 * offset is rounded to the nearest k (rint: ties to even) and the call reports back the offset it applied.
 * |offset| <= NVX_TUNE_MAX_HZ.
 *
 * Nominal chains.  Chain 0's nominal k is +4480 (+14 kHz), chain 1's -4480 (-14 kHz).  A chain that was never tuned,
 * or is tuned back to its nominal k, runs the reference mixer: its outputs, bits and messages are bit-identical to an
 * untuned handle's, whatever its sibling chain does.
 *
 * Tuned chains.  Any other k mixes FIR1 output o (counted since the stream's reset) with T[(k * o) mod N], N = 20160,
 * T[j] = (cos(2 pi j / N), -sin(2 pi j / N)) in fp64, correctly rounded (navtex_amd/csrc/nvx_tune_table.h):
 * u = (I*cr - Q*ci, I*ci + Q*cr), every product and sum rounded on its own (the reference's 518 expression form).
 * A frame holds N FIR1 outputs, so the phase depends on a sample's position in its frame alone.
 *
 * When.  A change applies from the first frame of that stream launched after the call returns (the call waits for the
 * handle's work in flight first); the filter histories are carried on, not cleared.  The setting is configuration:
 * it survives nvx_reset and nvx_stream_reset.
 *
 * Signal reports (navtex_amd_signal.h) of a tuned chain measure offset_hz against the tuned carrier.
 *
 * Errors.  NVX_ERR_ARG: NULL handle or group, bad stream or chain, a chain outside its stream's mask, an offset that
 * is not finite or out of range.  NVX_ERR_STATE: a wideband handle (its sub-band grid is the channeliser's).  In a
 * group, global_stream is indexed as nvx_group_poll_bits and the call goes to the member that owns the stream.
 */
#ifndef NAVTEX_AMD_TUNE_H
#define NAVTEX_AMD_TUNE_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_TUNE_N       20160
#define NVX_TUNE_STEP_HZ 3.125
#define NVX_TUNE_MAX_HZ  25000.0

/* Tune (stream, chain) to offset_hz from its stream's centre; *applied_hz (may be NULL) receives k * 3.125. */
NVX_API int nvx_set_carrier(nvx_handle *h, int stream, int chain, double offset_hz, double *applied_hz);
/* The chain's carrier offset (may be NULL) and whether it runs the reference mixer (1) or the tuned one (0). */
NVX_API int nvx_get_carrier(nvx_handle *h, int stream, int chain, double *offset_hz, int *reference_mixer);
NVX_API int nvx_group_set_carrier(nvx_group *g, int global_stream, int chain, double offset_hz, double *applied_hz);
NVX_API int nvx_group_get_carrier(nvx_group *g, int global_stream, int chain, double *offset_hz, int *reference_mixer);

#ifdef __cplusplus
}
#endif
#endif
