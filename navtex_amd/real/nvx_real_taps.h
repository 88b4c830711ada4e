/* nvx_real_taps.h -- the real-input converter's half-band taps (include/navtex_amd_real.h states them: these numbers are the
 * contract; tools/real_taps.py documents where they come from and reproduces them).  Shared by the host side, which hands
 * them out (nvx_real_taps), and the kernel, which folds them into immediates.  Internal. */
#ifndef NVX_REAL_TAPS_H
#define NVX_REAL_TAPS_H

#include <stdint.h>

#define NVX_REAL_K 13                       /* the delay in outputs; the Q branch has K + 1 taps a side */
#define NVX_REAL_S 14                       /* the taps are Q14 */
#define NVX_REAL_NTAPS (NVX_REAL_K + 1)
#define NVX_REAL_HISTORY (2 * NVX_REAL_K + 2)       /* sample pairs an output reaches back over, its own included */

#ifdef __cplusplus
constexpr
#else
static const
#endif
int16_t NVX_REAL_TAPS[NVX_REAL_NTAPS] = { 10376, 3314, 1825, 1144, 745, 486, 310, 191, 111, 60, 30, 13, 4, 1 };

#endif
