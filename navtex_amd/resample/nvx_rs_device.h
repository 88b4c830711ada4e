// nvx_rs_device.h -- what the kernels of the resampler (nvx_resample.hip), of the down-converter bank
// (navtex_amd/ddc/nvx_ddc.hip), of the narrowband interpolator, of the channel tap and of the same-rate companions have
// word for word in common: the vector types, the small arithmetic, the formats' conversions, and the launch of a kernel
// family's eight instances.  The same-rate companions (blanker, IQ corrector, real-input converter, noise canceller, tone
// notch) include it through nvx_stream_device.h, which adds their streaming helpers: the step's shape, load and store, the
// wave sums, the 64-bit division, the dispatch on the format.  Internal; each library compiles its own copy.  The kernel
// bodies stay in their files: see DESIGN 3.8.
#ifndef NVX_RS_DEVICE_H
#define NVX_RS_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nvx_resample_plan.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef short rs_short2 __attribute__((ext_vector_type(2)));
// volatile: every access stays one ds_read_b64 (paired into ds_read2_b64 the LDS serves them at half the rate)
typedef __attribute__((address_space(3))) volatile u32x2 lds_vu2;

__device__ __forceinline__ int dot2(uint32_t x, uint32_t h, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(rs_short2, x), __builtin_bit_cast(rs_short2, h), acc, false);
}
// (a & 0xffff) | (b << 16) and (a >> 16) | (b & 0xffff0000) as one v_perm_b32 each: selector bytes 0-3 name a's bytes, 4-7 b's
__device__ __forceinline__ uint32_t lo_pair(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }
__device__ __forceinline__ uint32_t hi_pair(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }
// n = quot * d + rem for n < d << BITS, by shifts and subtractions
template <int BITS>
__device__ __forceinline__ void divmod(uint32_t n, uint32_t d, uint32_t &quot, uint32_t &rem)
{
    quot = 0;
#pragma unroll
    for (int b = BITS - 1; b >= 0; b--)
        if (n >= (d << b)) { n -= d << b; quot |= 1u << b; }
    rem = n;
}
__device__ __forceinline__ int clamp16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// CF32: times 32768 in float32, to the nearest integer with ties to even, clamped; NaN -> 0
__device__ __forceinline__ uint32_t cf32_to_i16(uint32_t bits)
{
    const float f = __builtin_bit_cast(float, bits);
    const float y = __builtin_amdgcn_fmed3f(__builtin_rintf(f * 32768.0f), -32768.0f, 32767.0f);     // the clamp: one v_med3_f32
    const int v = f != f ? 0 : (int)y;
    return (uint32_t)v & 0xffffu;
}

template <int FMT> struct Fmt;
// bytes per sample, 16-byte words per group of 8, and the groups a thread has in flight while staging: in the resampler
// (UNROLL) and in the bank, whose mixer needs the registers (UNROLL_MIXED)
template <> struct Fmt<NVX_RS_CS16> { static constexpr int BPS = 4, NV = 2, UNROLL = 4, UNROLL_MIXED = 4; };
template <> struct Fmt<NVX_RS_CU8>  { static constexpr int BPS = 2, NV = 1, UNROLL = 4, UNROLL_MIXED = 4; };
template <> struct Fmt<NVX_RS_CS8>  { static constexpr int BPS = 2, NV = 1, UNROLL = 4, UNROLL_MIXED = 4; };
template <> struct Fmt<NVX_RS_CF32> { static constexpr int BPS = 8, NV = 4, UNROLL = 2, UNROLL_MIXED = 1; };

// one sample of the row as a packed word (I low, Q high)
template <int FMT>
__device__ __forceinline__ uint32_t load_sample(const char *row, int idx)
{
    if constexpr (FMT == NVX_RS_CS16) {
        return ((const uint32_t *)row)[idx];
    } else if constexpr (FMT == NVX_RS_CU8) {
        const uint32_t w = ((const uint16_t *)row)[idx];
        return ((((w & 0xffu) << 8) | ((w & 0xff00u) << 16)) ^ 0x80808080u);
    } else if constexpr (FMT == NVX_RS_CS8) {
        const uint32_t w = ((const uint16_t *)row)[idx];
        return ((w & 0xffu) << 8) | ((w & 0xff00u) << 16);
    } else {
        const uint2 w = ((const uint2 *)row)[idx];
        return cf32_to_i16(w.x) | (cf32_to_i16(w.y) << 16);
    }
}

// the 8 samples from sample s (a multiple of 8) of the row: NV 16-byte words.  NONTEMPORAL: read once (the resampler);
// plain loads let the L2 and the infinity cache serve the workgroups of the bank's sibling slices
template <int FMT, bool NONTEMPORAL>
__device__ __forceinline__ void load_group(const char *row, int s, u32x4 (&v)[Fmt<FMT>::NV])
{
    const u32x4 *p = (const u32x4 *)(row + (size_t)s * Fmt<FMT>::BPS);
#pragma unroll
    for (int i = 0; i < Fmt<FMT>::NV; i++) {
        if constexpr (NONTEMPORAL) v[i] = __builtin_nontemporal_load(p + i);
        else v[i] = p[i];
    }
}

// ... converted: 8 int16 of I and 8 of Q
template <int FMT>
__device__ __forceinline__ void convert_group(const u32x4 (&v)[Fmt<FMT>::NV], u32x4 &I, u32x4 &Q)
{
    if constexpr (FMT == NVX_RS_CS16) {
        const uint32_t a0 = v[0].x, a1 = v[0].y, a2 = v[0].z, a3 = v[0].w, b0 = v[1].x, b1 = v[1].y, b2 = v[1].z, b3 = v[1].w;
        I.x = lo_pair(a0, a1); I.y = lo_pair(a2, a3); I.z = lo_pair(b0, b1); I.w = lo_pair(b2, b3);
        Q.x = hi_pair(a0, a1); Q.y = hi_pair(a2, a3); Q.z = hi_pair(b0, b1); Q.w = hi_pair(b2, b3);
    } else if constexpr (FMT == NVX_RS_CU8 || FMT == NVX_RS_CS8) {
        // a word holds I0 Q0 I1 Q1 as bytes: each becomes the high byte of its int16, and (2u - 255) * 128 = (u << 8) - 0x7f80
        // is (u << 8) ^ 0x8080 in 16 bits
        const uint32_t flip = FMT == NVX_RS_CU8 ? 0x80808080u : 0u;
        const uint32_t w0 = v[0].x, w1 = v[0].y, w2 = v[0].z, w3 = v[0].w;
        I.x = ((w0 << 8) & 0xff00ff00u) ^ flip; I.y = ((w1 << 8) & 0xff00ff00u) ^ flip;
        I.z = ((w2 << 8) & 0xff00ff00u) ^ flip; I.w = ((w3 << 8) & 0xff00ff00u) ^ flip;
        Q.x = (w0 & 0xff00ff00u) ^ flip; Q.y = (w1 & 0xff00ff00u) ^ flip;
        Q.z = (w2 & 0xff00ff00u) ^ flip; Q.w = (w3 & 0xff00ff00u) ^ flip;
    } else {
        uint32_t i[4], q[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t f0 = v[k].x, f1 = v[k].y, f2 = v[k].z, f3 = v[k].w;
            i[k] = cf32_to_i16(f0) | (cf32_to_i16(f2) << 16);
            q[k] = cf32_to_i16(f1) | (cf32_to_i16(f3) << 16);
        }
        I.x = i[0]; I.y = i[1]; I.z = i[2]; I.w = i[3];
        Q.x = q[0]; Q.y = q[1]; Q.z = q[2]; Q.w = q[3];
    }
}

template <bool NONTEMPORAL>
__device__ __forceinline__ u32x4 rs_load16(const u32x4 *p)
{
    if constexpr (NONTEMPORAL) return __builtin_nontemporal_load(p);
    else return *p;
}

// the 4 (CS16, CF32) or 8 (CU8, CS8) samples from sample s (a multiple of that) of the row, as packed words: one 16-byte load,
// two for CF32.  NONTEMPORAL as in load_group (the blanker reads once; the IQ corrector's first pass leaves the lines cached)
template <int FMT, bool NONTEMPORAL = true>
__device__ __forceinline__ void load_words(const char *row, int s, uint32_t *w)
{
    const u32x4 *p = (const u32x4 *)(row + (size_t)s * Fmt<FMT>::BPS);
    if constexpr (FMT == NVX_RS_CS16) {
        const u32x4 v = rs_load16<NONTEMPORAL>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else if constexpr (FMT == NVX_RS_CU8 || FMT == NVX_RS_CS8) {
        // a word holds I0 Q0 I1 Q1 as bytes: each becomes the high byte of its int16; (2u - 255) * 128 is (u << 8) ^ 0x8080
        const uint32_t flip = FMT == NVX_RS_CU8 ? 0x80808080u : 0u;
        const u32x4 v = rs_load16<NONTEMPORAL>(p);
        const uint32_t d[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            // one v_perm_b32 each: selector 0 .. 3 names a byte of d, 0x0c is a zero byte
            w[2 * k] = __builtin_amdgcn_perm(d[k], d[k], 0x010c000cu) ^ flip;
            w[2 * k + 1] = __builtin_amdgcn_perm(d[k], d[k], 0x030c020cu) ^ flip;
        }
    } else {
        const u32x4 v0 = rs_load16<NONTEMPORAL>(p), v1 = rs_load16<NONTEMPORAL>(p + 1);
        w[0] = cf32_to_i16(v0.x) | (cf32_to_i16(v0.y) << 16); w[1] = cf32_to_i16(v0.z) | (cf32_to_i16(v0.w) << 16);
        w[2] = cf32_to_i16(v1.x) | (cf32_to_i16(v1.y) << 16); w[3] = cf32_to_i16(v1.z) | (cf32_to_i16(v1.w) << 16);
    }
}

// A kernel family is a struct with `template <int FMT, bool TAPS_LDS> static constexpr auto kernel`, the __global__
// function of that instance, all taking one ARGS by value.
// once per process: the LDS limit of the instances that hold the tap table there
template <class FAMILY>
static void nvx_rs_family_prepare(size_t lds_max)
{
    const void *fns[] = { (const void *)FAMILY::template kernel<NVX_RS_CS16, true>, (const void *)FAMILY::template kernel<NVX_RS_CU8, true>,
                          (const void *)FAMILY::template kernel<NVX_RS_CS8, true>, (const void *)FAMILY::template kernel<NVX_RS_CF32, true> };
    // a runtime that does not know the attribute launches with whatever LDS the launch names; one that enforces it has it set
    for (const void *f : fns)
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max) != hipSuccess) (void)hipGetLastError();
}

template <class FAMILY, int FMT, bool TAPS_LDS, class ARGS>
static hipError_t nvx_rs_family_launch_one(const ARGS *a, dim3 grid, size_t lds_bytes, hipStream_t s)
{
    hipLaunchKernelGGL((FAMILY::template kernel<FMT, TAPS_LDS>), grid, dim3(NVX_RS_THREADS), lds_bytes, s, *a);
    return hipGetLastError();
}

template <class FAMILY, class ARGS>
static hipError_t nvx_rs_family_launch(const ARGS *a, int format, bool taps_in_lds, dim3 grid, size_t lds_bytes, size_t lds_max, hipStream_t s)
{
    if (lds_bytes > lds_max) return hipErrorInvalidValue;
    switch (format * 2 + (taps_in_lds ? 1 : 0)) {
    case NVX_RS_CS16 * 2 + 1: return nvx_rs_family_launch_one<FAMILY, NVX_RS_CS16, true>(a, grid, lds_bytes, s);
    case NVX_RS_CS16 * 2:     return nvx_rs_family_launch_one<FAMILY, NVX_RS_CS16, false>(a, grid, lds_bytes, s);
    case NVX_RS_CU8 * 2 + 1:  return nvx_rs_family_launch_one<FAMILY, NVX_RS_CU8, true>(a, grid, lds_bytes, s);
    case NVX_RS_CU8 * 2:      return nvx_rs_family_launch_one<FAMILY, NVX_RS_CU8, false>(a, grid, lds_bytes, s);
    case NVX_RS_CS8 * 2 + 1:  return nvx_rs_family_launch_one<FAMILY, NVX_RS_CS8, true>(a, grid, lds_bytes, s);
    case NVX_RS_CS8 * 2:      return nvx_rs_family_launch_one<FAMILY, NVX_RS_CS8, false>(a, grid, lds_bytes, s);
    case NVX_RS_CF32 * 2 + 1: return nvx_rs_family_launch_one<FAMILY, NVX_RS_CF32, true>(a, grid, lds_bytes, s);
    case NVX_RS_CF32 * 2:     return nvx_rs_family_launch_one<FAMILY, NVX_RS_CF32, false>(a, grid, lds_bytes, s);
    }
    return hipErrorInvalidValue;
}

#endif
