// nvx_tap.hip -- the channel tap's kernel (include/navtex_amd_tap.h states the arithmetic; this file arranges it).
//
//   nvx_tap_kernel<KIND, UNIFORM>   grid (tiles, taps, inputs); 256 or 128 threads: the tile's outputs, one per thread
//   (nvx_tap_plan.h takes 128 where 256 outputs do not stage within its LDS budget: M / L beyond about 70).  Output-stationary: a decimator's neighbouring
//   outputs share most of their T input samples but none of their products, so a workgroup stages the input span of its
//   tile once and every lane runs the T taps of its own output over it.
//
//   stage    the tile's span of input words (about tile M / L + T), from the input's state row in front of the call's first
//            sample, from the input itself elsewhere (a pure FIR: no tile waits for another), zeros behind the call's end;
//            mixed with the row's shift and the sample's true index while staging (the bank's mixer: two v_dot2 per
//            sample; k = 0 passes the word through), and kept in the LDS as two planes of int16, I and Q, so that four
//            consecutive dwords of a plane are eight consecutive samples of one component.             -- the one barrier
//   filter   per group of 8 taps a lane reads 16 bytes of each plane as two ds_read_b64 (its window starts at a multiple of
//            4 samples: the tap row for its offset e = 0 .. 3 has e zeros in front; a ds_read_b128 would need a multiple
//            of 8, and two ds_read_b64 move the same bytes per LDS cycle) and the group's 32 bytes of the tap table: 8
//            int16 of hh = h >> 8 and 8 of hl = h & 255.  Four v_dot2 per half and component: 16 per group, 4 per LDS
//            read.  Both chains run in int32; every NVX_TAP_BLOCK_GROUPS groups (256 taps: 255 * 32768 * 256 < 2^31)
//            they are folded into the component's 64-bit sum, 256 hh + hl.  UNIFORM (L = 1 and waves * M a multiple of
//            4): wave w takes the tile's outputs w, w + waves, ..., so its lanes share phase and offset, the row's address
//            is wave-uniform and the taps come through the scalar cache into SGPRs.  Otherwise each lane reads its own
//            row through the vector cache.  The table (up to 560 KB) is never copied to the LDS.
//   finish   y = clamp16((acc + 2^20) >> 21) per component in 64-bit; IQ stores the packed word, REAL turns (y_I, y_Q) up
//            by the row's pitch and stores the real part as one int16.  A lane stores its own output: the lanes of a
//            workgroup's waves fill consecutive samples between them.
// The workgroup of an input's last tile of tap 0 writes the other state row: the input's last T - 1 unmixed words, from the
// input, or from the state row read where the call is shorter than that.
// Integers only.  nvx_tap_plan.h's functions give every position; nothing here divides.
#include "nvx_tap_plan.h"
#include "nvx_rs_device.h"

typedef const __attribute__((address_space(4))) u32x4 *const_u4;      // the constant address space: uniform loads are scalar loads

// the packed sample x = (I, Q) times W[j] = (c, s):  I' = (I c + Q s + 2^14) >> 15,  Q' = (Q c - I s + 2^14) >> 15, clamped
__device__ __forceinline__ uint32_t tap_mix(uint32_t x, uint32_t w)
{
    const rs_short2 cs = __builtin_bit_cast(rs_short2, w);
    const rs_short2 sc = { (short)-cs.y, cs.x };                                // (-s, c): no entry of W is -32768
    const int yi = clamp16(dot2(x, w, 1 << 14) >> 15);
    const int yq = clamp16(dot2(x, __builtin_bit_cast(uint32_t, sc), 1 << 14) >> 15);
    return ((uint32_t)yi & 0xffffu) | ((uint32_t)yq << 16);
}

__device__ __forceinline__ int tap_finish(long long hh, long long hl)
{
    const long long acc = hh * 256 + hl + (1ll << (NVX_TAP_SHIFT - 1));
    const long long y = acc >> NVX_TAP_SHIFT;
    return (int)(y < -32768 ? -32768 : (y > 32767 ? 32767 : y));
}

template <int KIND, bool UNIFORM>
__global__ __launch_bounds__(NVX_TAP_THREADS) void nvx_tap_kernel(const nvx_tap_args a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t tap_lds[];
    const int tid = threadIdx.x, threads = a.tile_out, tap = blockIdx.y, input = blockIdx.z, tile = blockIdx.x;
    const int rowid = input * a.n_taps + tap;
    uint32_t *const plane_i = tap_lds, *const plane_q = tap_lds + a.stage_len / 2;
    const uint32_t *const in = a.in + (size_t)input * a.pitch_in;
    const uint32_t *const st = a.state_in + (size_t)input * a.state_pitch;
    const int n_in = a.n_in, T = a.T;
    const uint32_t kk = (uint32_t)a.k[rowid] & (NVX_TAP_GRID - 1);              // k mod N; uniform
    const bool mixing = kk != 0;

    uint32_t qt, rt;                                                            // the tile's first output
    nvx_tap_tile_start(a, (uint32_t)tile, &qt, &rt);
    const int lo = nvx_tap_stage_first(a, qt);

    // ---- stage: pair v of the planes is input samples lo + 2 v and lo + 2 v + 1
    for (int v = tid; v < a.stage_len / 2; v += threads) {
        uint32_t w[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int idx = lo + 2 * v + c;
            uint32_t x = 0;
            if (idx >= 0) { if (idx < n_in) x = in[idx]; }
            else if (idx >= 1 - T) x = st[T - 1 + idx];
            if (mixing) x = tap_mix(x, a.w[(kk * ((a.n0 + (uint32_t)idx) & (NVX_TAP_GRID - 1))) & (NVX_TAP_GRID - 1)]);     // zero stays zero
            w[c] = x;
        }
        plane_i[v] = lo_pair(w[0], w[1]);
        plane_q[v] = hi_pair(w[0], w[1]);
    }
    __syncthreads();

    // ---- this lane's output: its q and phase, and where its window starts in the planes
    const int o = nvx_tap_thread_output(a.tile_out, tid);
    uint32_t dq, r;
    divmod<18>(rt + (uint32_t)(o * a.M), (uint32_t)a.L, dq, r);
    const int u0 = (int)(qt + dq) - (T - 1) - lo;                               // at least 0
    const int e = u0 & 3, pair0 = (u0 - e) >> 1;                                // pair0 is even: 8-byte aligned
    const uint32_t i = (uint32_t)tile * (uint32_t)a.tile_out + (uint32_t)o;     // the output's index in the call

    if (i < (uint32_t)a.n_out) {
        const int G = a.G;
        const lds_vu2 *xi = (const lds_vu2 *)(plane_i + pair0), *xq = (const lds_vu2 *)(plane_q + pair0);
        const u32x4 *taps_v = nullptr;
        const_u4 taps_s = nullptr;
        if constexpr (UNIFORM) {
            const int eu = __builtin_amdgcn_readfirstlane(e);                   // the wave's lanes share it
            taps_s = (const_u4)(uintptr_t)(a.table + (size_t)eu * G * 16);
        } else {
            taps_v = (const u32x4 *)(a.table + ((size_t)r * NVX_TAP_OFFSETS + e) * G * 16);
        }
        long long sum_i_h = 0, sum_i_l = 0, sum_q_h = 0, sum_q_l = 0;
        for (int g0 = 0; g0 < G; g0 += NVX_TAP_BLOCK_GROUPS) {
            const int g1 = g0 + NVX_TAP_BLOCK_GROUPS < G ? g0 + NVX_TAP_BLOCK_GROUPS : G;
            int ih = 0, il = 0, qh = 0, ql = 0;
#pragma unroll 2
            for (int g = g0; g < g1; g++) {
                u32x4 hh, hl;
                if constexpr (UNIFORM) { hh = taps_s[2 * g]; hl = taps_s[2 * g + 1]; }
                else { hh = taps_v[2 * g]; hl = taps_v[2 * g + 1]; }
                const u32x2 i0 = xi[2 * g], i1 = xi[2 * g + 1], q0 = xq[2 * g], q1 = xq[2 * g + 1];
                ih = dot2(i0.x, hh.x, ih); ih = dot2(i0.y, hh.y, ih); ih = dot2(i1.x, hh.z, ih); ih = dot2(i1.y, hh.w, ih);
                il = dot2(i0.x, hl.x, il); il = dot2(i0.y, hl.y, il); il = dot2(i1.x, hl.z, il); il = dot2(i1.y, hl.w, il);
                qh = dot2(q0.x, hh.x, qh); qh = dot2(q0.y, hh.y, qh); qh = dot2(q1.x, hh.z, qh); qh = dot2(q1.y, hh.w, qh);
                ql = dot2(q0.x, hl.x, ql); ql = dot2(q0.y, hl.y, ql); ql = dot2(q1.x, hl.z, ql); ql = dot2(q1.y, hl.w, ql);
            }
            sum_i_h += ih; sum_i_l += il; sum_q_h += qh; sum_q_l += ql;
        }
        const int yi = tap_finish(sum_i_h, sum_i_l), yq = tap_finish(sum_q_h, sum_q_l);
        const size_t at = (size_t)rowid * a.pitch_out + a.out_first + i;
        if constexpr (KIND == NVX_TAP_IQ) {
            ((uint32_t *)a.out)[at] = ((uint32_t)yi & 0xffffu) | ((uint32_t)yq << 16);
        } else {
            const uint32_t kp = (uint32_t)a.kp[rowid] & (NVX_TAP_GRID - 1);
            const uint32_t w = a.w[(kp * ((a.m0 + i) & (NVX_TAP_GRID - 1))) & (NVX_TAP_GRID - 1)];
            const rs_short2 cs = __builtin_bit_cast(rs_short2, w);
            const rs_short2 cn = { cs.x, (short)-cs.y };                        // (c, -s)
            const uint32_t y = ((uint32_t)yi & 0xffffu) | ((uint32_t)yq << 16);
            ((int16_t *)a.out)[at] = (int16_t)clamp16(dot2(y, __builtin_bit_cast(uint32_t, cn), 1 << 14) >> 15);
        }
    }

    // the input's state for the next call: by the workgroup of its last tile of tap 0, into the row this launch does not read
    if (tap == 0 && tile == (int)gridDim.x - 1)
        for (int t = tid; t < T - 1; t += threads) {
            const int at = n_in - (T - 1) + t;
            a.state_out[(size_t)input * a.state_pitch + t] = at >= 0 ? in[at] : st[T - 1 + at];
        }
}

typedef void (*tap_kernel)(const nvx_tap_args);
static const tap_kernel TAP_FAMILY[4] = { nvx_tap_kernel<NVX_TAP_IQ, false>, nvx_tap_kernel<NVX_TAP_IQ, true>, nvx_tap_kernel<NVX_TAP_REAL, false>,
                                          nvx_tap_kernel<NVX_TAP_REAL, true> };

void nvx_tap_prepare(void)
{
    // a runtime that does not know the attribute launches with whatever LDS the launch names; one that enforces it has it set
    for (const tap_kernel k : TAP_FAMILY)
        if (hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, NVX_TAP_LDS_BUDGET) != hipSuccess) (void)hipGetLastError();
}

hipError_t nvx_tap_launch(const nvx_tap_args *a, int kind, int n_inputs, hipStream_t s)
{
    if (kind < NVX_TAP_IQ || kind > NVX_TAP_REAL || nvx_tap_lds_bytes(a) > NVX_TAP_LDS_BUDGET || a->tiles < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a->tiles, (unsigned)a->n_taps, (unsigned)n_inputs);
    hipLaunchKernelGGL(TAP_FAMILY[kind * 2 + (a->uniform ? 1 : 0)], grid, dim3((unsigned)a->tile_out), nvx_tap_lds_bytes(a), s, *a);
    return hipGetLastError();
}
