/* nvx_internal.h -- declarations shared between the translation units of
 * libnavtex_amd.so; not part of the public ABI.                              */
#ifndef NVX_INTERNAL_H
#define NVX_INTERNAL_H

#include "navtex_amd.h"
#include "nvx_synth.h"

#ifdef __cplusplus
extern "C" {
#endif

void nvx_set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

void nvx_synth_periods(const nvx_carrier *c, uint32_t sample_rate, uint64_t first, size_t count,
                       nvx_period *out);

/* Test / diagnostics hook, exported for the tests (tests/test_gpu_timing_filter.py) but not part of the public ABI: the
 * bit-timing filter (receiver/decoder.C:142-215) of a handle's last launch, per 900 S/s sample t: corr[t] = |corr| and
 * csum[t] = the class sum the sample writes (0 while the filter is priming: before g = 8 and g = 574), and per bit period
 * m the word the front kernel hands the FSM: bits 0..8 = the mark/space decision of a window ending at sample 9m + k
 * ('B' = 1), bits 12..15 = the arg-max of the period's timing evaluation before the slew limiter (15 = none).  corr and
 * csum hold cap values and need nvx_enable_debug; words (cap + 8) / 9.  Any pointer may be NULL.  Returns the sample
 * count, clipped as nvx_debug_y3's; 0 on a bad argument or when corr / csum are asked without the debug buffers.     */
NVX_API size_t nvx_debug_timing(nvx_handle *h, int stream, int chain, double *corr, double *csum, uint16_t *words, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
