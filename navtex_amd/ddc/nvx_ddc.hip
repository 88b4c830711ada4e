// nvx_ddc.hip -- the down-converter bank's kernel (include/navtex_amd_ddc.h states the arithmetic; this file arranges it).
//
//   nvx_ddc_bank<FMT, TAPS_LDS>   grid (chunks, slices, inputs), 256 threads.  The resampler's kernel with a mixer
//   in its staging step: a workgroup walks tiles of 256 K consecutive outputs of one slice of one input; the workgroups of
//   an input's sibling slices stage the same input span, each through its own mixer.
//
// Per tile:
//   stage   the input span the tile needs, widened to multiples of 8 samples, is read with plain 16-byte loads (cached:
//           the sibling slices read the same bytes), converted, mixed, and written to the LDS as two planes of int16 (one
//           ds_write_b128 each per 8 samples).  The mixer: a thread's group of 8 starts at table index
//           j = (k * (n mod N)) mod N of its first sample and steps j by k; W[j] comes from the half turn held in the LDS
//           (one 4-byte read, negated as a packed pair for j >= N/2), a component is one v_dot2_i32_i16 of the packed
//           sample with (c, s) or (-s, c) on top of the rounding constant, then a shift and a clamp.  A slice with k = 0
//           takes the resampler's staging unchanged (a workgroup-uniform branch) and does not load the table.
//           Samples in front of the call come from the input's history row -- unmixed, mixed here with their true index
//           -- samples behind its end are zeros; only the groups at those two edges take the sample-by-sample path.
//   FIR     the resampler's: three ds_read_b64 (taps, I, Q) and four v_dot2c_i32_i16 per loop step.
// The LDS holds the planes, the half turn of the table (8448 bytes with its padding) and the tap table (up to 60 KB; a
// larger one is read from global memory).  No fp64, float32 only in CF32's conversion, no atomics, no division.
// The types, the small arithmetic, the formats' conversions and the launch of the eight instances are the resampler's
// (navtex_amd/resample/nvx_rs_device.h); the kernel body is this file's own (DESIGN 3.8 says why).
#include "nvx_ddc_plan.h"
#include "nvx_rs_device.h"

static constexpr uint32_t GRID_MASK = NVX_DDC_GRID - 1;

// ... converted, as 8 packed samples (I low, Q high): what the mixer takes
template <int FMT>
__device__ __forceinline__ void unpack_group(const u32x4 (&v)[Fmt<FMT>::NV], uint32_t (&x)[NVX_RS_GROUP])
{
    if constexpr (FMT == NVX_RS_CS16) {
        x[0] = v[0].x; x[1] = v[0].y; x[2] = v[0].z; x[3] = v[0].w; x[4] = v[1].x; x[5] = v[1].y; x[6] = v[1].z; x[7] = v[1].w;
    } else if constexpr (FMT == NVX_RS_CU8 || FMT == NVX_RS_CS8) {
        // bytes I0 Q0 I1 Q1 -> (0 I0 0 Q0) and (0 I1 0 Q1): one v_perm_b32 each (selector 0x0c is a zero byte)
        const uint32_t flip = FMT == NVX_RS_CU8 ? 0x80808080u : 0u;
        const uint32_t w[4] = { v[0].x, v[0].y, v[0].z, v[0].w };
#pragma unroll
        for (int i = 0; i < 4; i++) {
            x[2 * i] = __builtin_amdgcn_perm(w[i], w[i], 0x010c000cu) ^ flip;
            x[2 * i + 1] = __builtin_amdgcn_perm(w[i], w[i], 0x030c020cu) ^ flip;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            x[2 * i] = cf32_to_i16(v[i].x) | (cf32_to_i16(v[i].y) << 16);
            x[2 * i + 1] = cf32_to_i16(v[i].z) | (cf32_to_i16(v[i].w) << 16);
        }
    }
}

// W[j] as a packed (c, s), j in [0, N): the half turn's word, negated as a packed pair in the other half (no entry is -32768)
__device__ __forceinline__ uint32_t table_word(const uint32_t *tab, uint32_t j)
{
    const uint32_t h = j & (NVX_DDC_HALF - 1);
    const uint32_t w = tab[NVX_DDC_SLOT(h)];
    const rs_short2 neg = -__builtin_bit_cast(rs_short2, w);
    return (j & NVX_DDC_HALF) ? __builtin_bit_cast(uint32_t, neg) : w;
}

// the packed sample x = (I, Q) times W[j] = (c, s):  I' = (I c + Q s + 2^14) >> 15,  Q' = (Q c - I s + 2^14) >> 15, clamped
__device__ __forceinline__ uint32_t mix(uint32_t x, uint32_t w)
{
    const rs_short2 cs = __builtin_bit_cast(rs_short2, w);
    const rs_short2 sc = { (short)-cs.y, cs.x };                                // (-s, c)
    const int yi = clamp16(dot2(x, w, 1 << 14) >> 15);
    const int yq = clamp16(dot2(x, __builtin_bit_cast(uint32_t, sc), 1 << 14) >> 15);
    return ((uint32_t)yi & 0xffffu) | ((uint32_t)yq << 16);
}

template <int FMT, bool TAPS_LDS>
__global__ __launch_bounds__(NVX_RS_THREADS) void nvx_ddc_bank(const nvx_ddc_args d)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t *const plane_i = lds, *const plane_q = lds + NVX_RS_PLANE / 2, *const lds_tab = lds + NVX_RS_PLANE,
                   *const lds_taps = lds + NVX_RS_PLANE + NVX_DDC_TAB_DW;
    constexpr int BPS = Fmt<FMT>::BPS, NV = Fmt<FMT>::NV, UNROLL = Fmt<FMT>::UNROLL_MIXED;
    const nvx_rs_args &a = d.rs;

    const int tid = threadIdx.x, slice = blockIdx.y, input = blockIdx.z;
    const char *const row = (const char *)a.in + (size_t)input * a.pitch_in * BPS;
    uint32_t *const out = a.out + ((size_t)input * d.n_slices + slice) * a.pitch_out + a.out_first;
    const uint32_t *const hist_in = a.hist_in + (size_t)input * a.hist_pitch;
    const int L = a.L, T = a.T, n_in = a.n_in;
    const uint32_t kk = (uint32_t)d.k[input * d.n_slices + slice] & GRID_MASK;          // k mod N; uniform
    const bool mixing = kk != 0;

    if constexpr (TAPS_LDS)
        for (int i = tid * 4; i < a.tap_dw; i += NVX_RS_THREADS * 4) *(u32x4 *)&lds_taps[i] = *(const u32x4 *)&a.taps[i];
    if (mixing)
        for (int i = tid * 4; i < NVX_DDC_TAB_DW; i += NVX_RS_THREADS * 4) *(u32x4 *)&lds_tab[i] = *(const u32x4 *)&d.table[i];
    __syncthreads();

    const int tile_out = NVX_RS_THREADS * a.K;
    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;

    // The first output of the chunk's first tile (uniform), then this thread's first output: positions as (q, r) = (pos
    // div L, pos mod L), advanced by host-computed steps (the resampler's scheme: the kernel divides nowhere).
    uint32_t rt, r, quot;
    divmod<12>(a.r0 + (uint32_t)blockIdx.x * a.chunk_dr, (uint32_t)L, quot, rt);
    int qt = a.qoff + (int)((uint32_t)blockIdx.x * a.chunk_dq + quot);
    divmod<8>(rt + (uint32_t)tid * a.m_mod, (uint32_t)L, quot, r);
    int q = qt + (int)((uint32_t)tid * a.m_div + quot);

    for (int tile = tile0; tile < tile1; tile++) {
        const int first = tile * tile_out;
        const int tile_n = a.n_out - first < tile_out ? a.n_out - first : tile_out;
        const int q_last = qt + (int)a.span_q + (rt + a.span_r >= (uint32_t)L ? 1 : 0);     // of a full tile: a bound for the last one
        const int lo = (qt - (T - 1)) & ~(NVX_RS_GROUP - 1);                    // floor, below zero too
        const int hi = (q_last + 2 * NVX_RS_GROUP - 1) & ~(NVX_RS_GROUP - 1);   // the windows' zero taps reach up to 6 samples beyond q_last
        const int groups = (hi - lo) / NVX_RS_GROUP;
        // the groups that lie wholly inside the call's input
        int g0 = lo < 0 ? -lo / NVX_RS_GROUP : 0;
        int g1 = (n_in - lo) / NVX_RS_GROUP;
        g0 = g0 < groups ? g0 : groups;
        g1 = g1 < g0 ? g0 : (g1 < groups ? g1 : groups);

        for (int g = g0 + tid; g < g1; g += NVX_RS_THREADS * UNROLL) {
            u32x4 v[UNROLL][NV];
#pragma unroll
            for (int u = 0; u < UNROLL; u++)
                if (g + u * NVX_RS_THREADS < g1) load_group<FMT, false>(row, lo + (g + u * NVX_RS_THREADS) * NVX_RS_GROUP, v[u]);
#pragma unroll
            for (int u = 0; u < UNROLL; u++)
                if (g + u * NVX_RS_THREADS < g1) {
                    const int gg = g + u * NVX_RS_THREADS;
                    u32x4 I, Q;
                    if (mixing) {
                        uint32_t x[NVX_RS_GROUP];
                        unpack_group<FMT>(v[u], x);
                        // n mod N of the group's first sample (lo may be negative: the sum wraps consistently, N divides 2^32)
                        uint32_t j = (kk * ((d.n0 + (uint32_t)(lo + gg * NVX_RS_GROUP)) & GRID_MASK)) & GRID_MASK;
#pragma unroll
                        for (int i = 0; i < NVX_RS_GROUP; i++) {
                            x[i] = mix(x[i], table_word(lds_tab, j));
                            j = (j + kk) & GRID_MASK;
                        }
                        u32x4 m[2];
                        m[0].x = x[0]; m[0].y = x[1]; m[0].z = x[2]; m[0].w = x[3];
                        m[1].x = x[4]; m[1].y = x[5]; m[1].z = x[6]; m[1].w = x[7];
                        convert_group<NVX_RS_CS16>(m, I, Q);
                    } else {
                        convert_group<FMT>(v[u], I, Q);
                    }
                    *(u32x4 *)&plane_i[gg * 4] = I;
                    *(u32x4 *)&plane_q[gg * 4] = Q;
                }
        }
        // the edges, sample by sample: history (or silence) in front of the call, zeros behind it
        const int edge = (g0 + (groups - g1)) * NVX_RS_GROUP;
        for (int e = tid; e < edge; e += NVX_RS_THREADS) {
            const int li = e < g0 * NVX_RS_GROUP ? e : e + (g1 - g0) * NVX_RS_GROUP;
            const int idx = lo + li;
            uint32_t w = 0;
            if (idx >= 0) { if (idx < n_in) w = load_sample<FMT>(row, idx); }
            else if (a.hist_valid && idx >= -(T - 1)) w = hist_in[T - 1 + idx];
            if (mixing) w = mix(w, table_word(lds_tab, (kk * ((d.n0 + (uint32_t)idx) & GRID_MASK)) & GRID_MASK));     // zero stays zero
            ((uint16_t *)plane_i)[li] = (uint16_t)w;
            ((uint16_t *)plane_q)[li] = (uint16_t)(w >> 16);
        }
        __syncthreads();

        for (int k = 0; k < a.K; k++) {
            const int jl = tid + k * NVX_RS_THREADS;
            if (jl < tile_n) {
                const int ws = q - (T - 1) - lo;                               // the window's first sample in the planes: >= 0
                const int sh = ws & (NVX_RS_ALIGN - 1);
                const int xw = (ws - sh) >> 1;                                 // ... as a word index, even
                const int tw = (sh * L + (int)r) * a.row_dw;
                int acc_i = 1 << (NVX_RS_SHIFT - 1), acc_q = 1 << (NVX_RS_SHIFT - 1);
#pragma unroll 2
                for (int c = 0; c < a.Tp / 2; c += 2) {
                    u32x2 h;
                    if constexpr (TAPS_LDS) h = *(lds_vu2 *)&lds_taps[tw + c];
                    else h = *(const u32x2 *)&a.taps[tw + c];
                    const u32x2 xi = *(lds_vu2 *)&plane_i[xw + c];
                    const u32x2 xq = *(lds_vu2 *)&plane_q[xw + c];
                    const uint32_t h0 = h.x, h1 = h.y, i0 = xi.x, i1 = xi.y, q0 = xq.x, q1 = xq.y;
                    acc_i = dot2(i0, h0, acc_i); acc_q = dot2(q0, h0, acc_q);
                    acc_i = dot2(i1, h1, acc_i); acc_q = dot2(q1, h1, acc_q);
                }
                const int yi = clamp16(acc_i >> NVX_RS_SHIFT), yq = clamp16(acc_q >> NVX_RS_SHIFT);
                out[first + jl] = ((uint32_t)yi & 0xffffu) | ((uint32_t)yq << 16);
            }
            q += (int)a.dq; r += a.dr;
            if (r >= (uint32_t)L) { r -= (uint32_t)L; q++; }
        }
        __syncthreads();
        qt += (int)a.tile_dq; rt += a.tile_dr;
        if (rt >= (uint32_t)L) { rt -= (uint32_t)L; qt++; }
    }

    // the input's last T-1 converted, unmixed samples for the next call: by the last chunk of slice 0, into the row this
    // launch does not read
    if (blockIdx.x == gridDim.x - 1 && slice == 0) {
        uint32_t *const hist_out = a.hist_out + (size_t)input * a.hist_pitch;
        for (int k = tid; k < T - 1; k += NVX_RS_THREADS) {
            const int idx = n_in - (T - 1) + k;
            hist_out[k] = idx >= 0 ? load_sample<FMT>(row, idx) : (a.hist_valid ? hist_in[T - 1 + idx] : 0u);
        }
    }
}

struct ddc_family {
    template <int FMT, bool TAPS_LDS> static constexpr auto kernel = nvx_ddc_bank<FMT, TAPS_LDS>;
};

static const size_t LDS_MAX = (NVX_RS_PLANE + NVX_DDC_TAB_DW) * 4 + NVX_RS_TAPS_LDS_MAX;

void nvx_ddc_prepare(void) { nvx_rs_family_prepare<ddc_family>(LDS_MAX); }

size_t nvx_ddc_lds_bytes(const nvx_ddc_args *a, bool taps_in_lds)
{
    return (size_t)(NVX_RS_PLANE + NVX_DDC_TAB_DW) * 4 + (taps_in_lds ? (size_t)a->rs.tap_dw * 4 : 0);
}

hipError_t nvx_ddc_launch(const nvx_ddc_args *a, int format, int n_inputs, int chunks, bool taps_in_lds, hipStream_t s)
{
    const dim3 grid((unsigned)chunks, (unsigned)a->n_slices, (unsigned)n_inputs);
    return nvx_rs_family_launch<ddc_family>(a, format, taps_in_lds, grid, nvx_ddc_lds_bytes(a, taps_in_lds), LDS_MAX, s);
}
