/* navtex_amd_soft.h -- soft-decision SITOR-B decoding of libnavtex_amd.so (an addition to navtex_amd.h)
 *
 * SITOR-B sends every character twice, 280 ms apart: in the DX slot and again in the RX slot.  The character layer of
 * navtex_amd.h uses that the way the reference does: the RX copy if it is a valid 4B/3Y code, else the DX copy, else '*'.
 * Two noisy copies that are both invalid give a '*'; a copy that noise turned into another valid code is taken as it is.
 * With soft decoding on, the GPU keeps what the hard decision throws away -- how far apart the two matched-filter
 * energies of every bit were -- and a second character layer per chain combines the two copies of a character by those
 * weights.  Off by default; the bits, the hard character layer, its messages (cfg.on_message / add_message) and its trace
 * are the same with it on or off.
 *
 * The soft value.  For every bit the demodulator decides, soft = Brot - Yrot: ONE float32 subtraction of the two float32
 * energies of the bit's own five-sample window (receiver/decoder.C:115-132, the expression whose comparison is the bit).
 * So soft > 0 <=> the bit is 'B', and a launch yields exactly as many soft values as bits, in the same order.
 *
 * The soft character layer (nvx_sitor_set_soft).  Everything that is control stays on the hard bits: the phasing
 * detector, slot tracking, end of emission, the 20-code error window and its abort, the 1100-bit mute.  Only the
 * character printed in the RX slot changes.  With rx[i], dx[i] the soft values of the RX code and of its DX twin (sent two
 * pairs earlier), i = 0 the first-received bit, all sums in double and in bit order:
 *   m[i] = rx[i] + dx[i]
 *   data hypothesis     the three smallest m[i] are 'Y' (code bit 1, first-received bit = MSB), the others 'B'; ties go to
 *                       the earlier bit.  This is the 4B/3Y code of maximum correlation.  sd = sum m[i] - 2 * (those three)
 *   phasing hypothesis  the slots differ by design, DX = beta 0x4C, RX = alpha 0x07:
 *                       sp = sum s_alpha[i] * rx[i] + sum s_beta[i] * dx[i], s = -1 on a code's 'Y' bits, +1 elsewhere
 *   sp > sd (strictly): alpha, which prints nothing; otherwise the data code.  This path never prints '*'.
 * The line framing (ZCZC / NNNN) is shared, so better characters also rescue message boundaries.
 *
 * nvx_group has no wrappers for these calls: a member's handle is reachable through nvx_group_member, and these calls
 * may be made on it.
 */
#ifndef NAVTEX_AMD_SOFT_H
#define NAVTEX_AMD_SOFT_H

#include "navtex_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NVX_SOFT_DECODE 1        /* soft values travel to the host with the bits; soft character layers run        */
#define NVX_SOFT_KEEP   2        /* (with NVX_SOFT_DECODE) the values are also kept for nvx_poll_soft                */

/* mode 0: off -- frees the buffers, the soft character layers and the kept values.  NVX_SOFT_DECODE (1): on.
 * NVX_SOFT_DECODE | NVX_SOFT_KEEP (3): on, and the values are kept for polling.  Waits for the handle's work in flight
 * first (as nvx_enable_signal_report), so whole launches are either soft or not: those launched while the mode was on.
 * The setting survives nvx_reset and nvx_stream_reset; they restart the soft character layers and drop the kept values of
 * the streams they reset.  Soft character layers exist where the hard ones do (cfg.char_layer).  Costs, while on, 4 bytes
 * per bit copied back with the bits.
 * NVX_ERR_ARG: NULL handle, another mode; NVX_ERR_STATE: the handle needs nvx_reset; NVX_ERR_NODEV: no device.          */
NVX_API int nvx_enable_soft(nvx_handle *h, int mode);
/* Where the soft character layers' messages go: fn(user, stream, bbbb, message, freq) -- called where cfg.on_message is
 * called for the hard layer's, in launch order, on the same threads, under the same rules, behind the hard layer's
 * messages of the same launch.  NULL (the default): they are dropped.  They never go to add_message.
 * nvx_store_on_message with a store as `user` is a valid fn.  May be set before or after nvx_enable_soft.               */
NVX_API int nvx_set_soft_message_fn(nvx_handle *h, nvx_message_fn fn, void *user);
/* Copies out and consumes up to `cap` soft values of decoded stream `stream` (indexed as nvx_poll_bits), chain 0 / 1:
 * its own cursor, the history rule of nvx_poll_bits (cfg.bit_history; a reader that fell behind resumes at the oldest
 * value held).  Value i of a chain since the mode was turned on belongs to bit i of the launches made since then.
 * Returns the number copied; 0 without NVX_SOFT_KEEP or on bad arguments.                                               */
NVX_API size_t nvx_poll_soft(nvx_handle *h, int stream, int chain, float *out, size_t cap);
/* Soft values of (stream, chain) taken in since create / reset / the mode was turned on: equals the growth of
 * nvx_bit_count over the launches made while the mode was on.  0 on bad arguments.                                      */
NVX_API uint64_t nvx_soft_count(nvx_handle *h, int stream, int chain);

/* ---- the character layer (plain C, no GPU) ------------------------------------------------------------------------- */
/* on != 0: the combining rule above; 0 (the default): the reference's.  Keeps the layer's state; survives nvx_sitor_reset. */
NVX_API void nvx_sitor_set_soft(nvx_sitor *s, int on);
/* n bits with their soft values: the bit is 'B' iff soft > 0.  With soft mode off this is nvx_sitor_receive_bits on the
 * signs: the same messages and the same trace.  (nvx_sitor_receive_bit(s) in soft mode weigh a bit +-1.)                */
NVX_API void nvx_sitor_receive_soft(nvx_sitor *s, const float *soft, size_t n);

#ifdef __cplusplus
}
#endif
#endif
