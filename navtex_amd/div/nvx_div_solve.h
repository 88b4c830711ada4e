/* nvx_div_solve.h -- step 6 of the diversity combiner's contract (include/navtex_amd_div.h): the window's four sums -> lead,
 * weight, coherence and reason, in 64-bit integers.  Plain C++ that the fold kernel (nvx_div.hip) runs on the device and
 * tests/harness/div_solve.cpp runs on the host.  The quotients and the square root are formed by shifts and subtractions:
 * the device compiler's 64-bit division goes through float32 reciprocals, and nothing here is floating point.  Internal. */
#ifndef NVX_DIV_SOLVE_H
#define NVX_DIV_SOLVE_H

#include <stdint.h>

#include "navtex_amd_div.h"

#if defined(__HIPCC__)
#define NVX_DIV_HD __host__ __device__ __forceinline__
#else
#define NVX_DIV_HD static inline
#endif

/* n / d for d > 0 */
NVX_DIV_HD uint64_t nvx_div_udiv(uint64_t n, uint64_t d)
{
    uint64_t q = 0, r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int b = 63; b >= 0; b--) {
        r = (r << 1) | ((n >> b) & 1);
        if (r >= d) { r -= d; q |= (uint64_t)1 << b; }
    }
    return q;
}

/* floor(n / d) for d > 0 */
NVX_DIV_HD int64_t nvx_div_floor_div(int64_t n, int64_t d)
{
    return n >= 0 ? (int64_t)nvx_div_udiv((uint64_t)n, (uint64_t)d) : -(int64_t)nvx_div_udiv((uint64_t)(-n) + (uint64_t)d - 1, (uint64_t)d);
}

/* the largest r with r * r <= q, for q < 2^62: one bit of r per round, from bit 30 down */
NVX_DIV_HD uint64_t nvx_div_isqrt(uint64_t q)
{
    uint64_t r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int b = 30; b >= 0; b--) {
        const uint64_t t = r | ((uint64_t)1 << b);
        if (t * t <= q) r = t;
    }
    return r;
}

NVX_DIV_HD int nvx_div_bitlength(uint64_t v)
{
    int n = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    while (v) { n++; v >>= 1; }
    return n;
}

NVX_DIV_HD int64_t nvx_div_clamp_w(int64_t v) { return v < -NVX_DIV_W_ONE ? -NVX_DIV_W_ONE : (v > NVX_DIV_W_ONE ? NVX_DIV_W_ONE : v); }

/* Steps 6.1 .. 6.7 on TAA, TBB, TRE, TIM.  Returns the reason. */
NVX_DIV_HD int nvx_div_solve(int64_t TAA, int64_t TBB, int64_t TRE, int64_t TIM, int32_t *lead, int32_t *w_re, int32_t *w_im, int32_t *coherence)
{
    *lead = 0; *w_re = 0; *w_im = 0; *coherence = 0;
    if (TAA + TBB < 1024) return 1;
    const int bits = nvx_div_bitlength((uint64_t)(TAA > TBB ? TAA : TBB)), sh = bits > 29 ? bits - 29 : 0;
    const int64_t taa = TAA >> sh, tbb = TBB >> sh, tre = TRE >> sh, tim = TIM >> sh;
    const int64_t d = taa - tbb, cross = tre * tre + tim * tim;
    const int64_t r = (int64_t)nvx_div_isqrt((uint64_t)(d * d + 4 * cross));
    const int64_t den = r + (d >= 0 ? d : -d);
    if (den == 0) return 0;
    *lead = d >= 0 ? 0 : 1;
    *w_re = (int32_t)nvx_div_clamp_w(nvx_div_floor_div(tre * 32768 + den, 2 * den));
    *w_im = (int32_t)nvx_div_clamp_w(nvx_div_floor_div((d >= 0 ? tim : -tim) * 32768 + den, 2 * den));
    const int64_t m = (taa * tbb) >> 14;
    if (m > 0) {
        const uint64_t c = nvx_div_udiv((uint64_t)cross, (uint64_t)m);
        *coherence = c > NVX_DIV_COHERENCE_ONE ? NVX_DIV_COHERENCE_ONE : (int32_t)c;
    }
    return 0;
}

#endif
