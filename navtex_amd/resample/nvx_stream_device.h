// nvx_stream_device.h -- what the kernels of the same-rate companions have word for word in common beyond the formats' loads
// (nvx_rs_device.h, included here): the blanker (navtex_amd/blank/nvx_blank.hip), the IQ corrector (navtex_amd/iqc/nvx_iqc.hip),
// the real-input converter (navtex_amd/real/nvx_real.hip), the noise canceller (navtex_amd/anc/nvx_anc.hip) and the tone notch
// (navtex_amd/notch/nvx_notch.hip).  All of them walk tiles of a row in steps of 64 lanes x SPT samples, counted from the
// call's first sample: the step's shape, its load and its store, the wave sums over DPP, the 64-bit division of the block
// solves, and the host side's dispatch on the format.  The zoom bank (navtex_amd/zoom/nvx_zoom.hip) takes the lane's group and
// the dispatch from here; the row aligner (navtex_amd/align/nvx_align.hip) the step's store, the wave sums and the dispatch; the multi-tap noise
// canceller (navtex_amd/wanc/nvx_wanc.hip) the step's shape and load, the wave sums and the dispatch; the diversity combiner
// (navtex_amd/div/nvx_div.hip) the step's shape, load and store, the wave sums, in_vector_registers and the dispatch.  Internal; each library
// compiles its own copy and nothing is linked.
// The kernel bodies stay in their files, and so does what a kernel compiles differently through a helper: the
// blanker's step load, the converter's and the notch's one-group stores ("What the same-rate kernels share").
#ifndef NVX_STREAM_DEVICE_H
#define NVX_STREAM_DEVICE_H

#include <type_traits>

#include "nvx_rs_device.h"

typedef int64_t i64;
typedef unsigned long long u64;

// samples per lane and step, samples of a wave's step, steps per region
template <int FMT> struct StreamLane { static constexpr int SPT = (FMT == NVX_RS_CU8 || FMT == NVX_RS_CS8) ? 8 : 4, STEP = 64 * SPT; };
template <int FMT, int REGION> struct StreamShape : StreamLane<FMT> { static constexpr int STEPS = REGION / StreamLane<FMT>::STEP; };

// step j of a thread's samples of the tile (`base` is its first sample of the tile, counted from the call's first) as packed
// words; those behind the call's end are zero
template <int FMT, bool FULL, bool NONTEMPORAL>
__device__ __forceinline__ void load_step(const char *src, int base, int j, int n_in, uint32_t *w)
{
    constexpr int SPT = StreamLane<FMT>::SPT;
    if (FULL || base + j * 64 * SPT + SPT <= n_in) load_words<FMT, NONTEMPORAL>(src, j * 64 * SPT, w);
    else {
#pragma unroll
        for (int k = 0; k < SPT; k++) w[k] = base + j * 64 * SPT + k < n_in ? load_sample<FMT>(src, j * 64 * SPT + k) : 0u;
    }
}
// float32 brings twice the bytes: a step is loaded when its turn comes, or a tile's worth of registers waits for the loads;
// the other formats have a tile's loads in flight at once
template <int FMT> struct Ahead { static constexpr bool value = FMT != NVX_RS_CF32; };

// step j of a thread's words of the tile, as load_step reads them (`dst`: where the word of sample `base` goes): 16-byte
// non-temporal stores where the output rows are 16-byte aligned (`out_vec`: the int of the args struct, as it is) and the step
// is whole, word by word under the call's end otherwise
template <int FMT, bool FULL>
__device__ __forceinline__ void store_step(uint32_t *dst, int out_vec, int base, int j, int n_in, const uint32_t *w)
{
    constexpr int SPT = StreamLane<FMT>::SPT;
    if (out_vec && (FULL || base + j * 64 * SPT + SPT <= n_in)) {
#pragma unroll
        for (int k = 0; k < SPT; k += 4) {
            const u32x4 v = { w[k], w[k + 1], w[k + 2], w[k + 3] };
            __builtin_nontemporal_store(v, (u32x4 *)&dst[j * 64 * SPT + k]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < SPT; k++)
            if (FULL || base + j * 64 * SPT + k < n_in) dst[j * 64 * SPT + k] = w[k];
    }
}

// DPP: lanes without a source, and rows masked out, receive `old`
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false); }
enum { ROW_SHR1 = 0x111, ROW_SHR2 = 0x112, ROW_SHR4 = 0x114, ROW_SHR8 = 0x118, WAVE_SHR1 = 0x138, ROW_BCAST15 = 0x142, ROW_BCAST31 = 0x143 };

// the wave's sum, in lane 63: for a kernel that has vector registers to spare and few scalar ones
__device__ __forceinline__ int wave_sum_in_last_lane(int v)
{
    v += dpp<ROW_SHR1, 0xf>(0, v); v += dpp<ROW_SHR2, 0xf>(0, v); v += dpp<ROW_SHR4, 0xf>(0, v); v += dpp<ROW_SHR8, 0xf>(0, v);
    v += dpp<ROW_BCAST15, 0xa>(0, v); v += dpp<ROW_BCAST31, 0xc>(0, v);
    return v;
}
// ... uniform
__device__ __forceinline__ int wave_sum(int v) { return __builtin_amdgcn_readlane(wave_sum_in_last_lane(v), 63); }
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return (uint32_t)wave_sum((int)v); }
// ... of 64-bit values, in three limbs of 22, 22 and 20 bits, whose sums over 64 lanes stay inside 32 bits
__device__ __forceinline__ i64 wave_sum64_in_last_lane(i64 v)
{
    const int l0 = (int)((uint32_t)v & 0x3fffffu), l1 = (int)((uint32_t)(v >> 22) & 0x3fffffu), l2 = (int)(v >> 44);
    return (i64)wave_sum_in_last_lane(l0) + ((i64)wave_sum_in_last_lane(l1) << 22) + (i64)wave_sum_in_last_lane(l2) * ((i64)1 << 44);
}
__device__ __forceinline__ i64 wave_sum64(i64 v)
{
    const int l0 = (int)((uint32_t)v & 0x3fffffu), l1 = (int)((uint32_t)(v >> 22) & 0x3fffffu), l2 = (int)(v >> 44);
    return (i64)wave_sum(l0) + ((i64)wave_sum(l1) << 22) + (i64)wave_sum(l2) * ((i64)1 << 44);
}

// a uniform value through vector registers: what is computed from it then is vector code too
__device__ __forceinline__ i64 in_vector_registers(i64 v)
{
    int lo = (int)v, hi = (int)(v >> 32);
    asm volatile("" : "+v"(lo), "+v"(hi));
    return ((i64)hi << 32) | (uint32_t)lo;
}

// n / d for d > 0, by shifts and subtractions: the compiler's 64-bit division goes through float32 reciprocals
__device__ __forceinline__ u64 udiv64(u64 n, u64 d)
{
    u64 q = 0, r = 0;
#pragma unroll 1
    for (int b = 63; b >= 0; b--) {
        r = (r << 1) | ((n >> b) & 1);
        if (r >= d) { r -= d; q |= (u64)1 << b; }
    }
    return q;
}
__device__ __forceinline__ i64 floor_div(i64 n, i64 d) { return n >= 0 ? (i64)udiv64((u64)n, (u64)d) : -(i64)udiv64((u64)(-n) + (u64)d - 1, (u64)d); }

// the host side: f(std::integral_constant<int, NVX_RS_...>) for a format of the resampler's numbering, which each library's
// static_assert says its own is; an unknown format launches nothing
template <class F>
static hipError_t nvx_for_format(int format, F &&f)
{
    switch (format) {
    case NVX_RS_CS16: return f(std::integral_constant<int, NVX_RS_CS16>{});
    case NVX_RS_CU8:  return f(std::integral_constant<int, NVX_RS_CU8>{});
    case NVX_RS_CS8:  return f(std::integral_constant<int, NVX_RS_CS8>{});
    case NVX_RS_CF32: return f(std::integral_constant<int, NVX_RS_CF32>{});
    }
    return hipErrorInvalidValue;
}

#endif
