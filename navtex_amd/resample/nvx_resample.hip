// nvx_resample.hip -- the resampler's kernel (include/navtex_amd_resample.h states the arithmetic; this file arranges it).
//
//   nvx_resample<FMT, TAPS_LDS>   grid (chunks, streams), 256 threads.  A workgroup walks tiles of 256 K consecutive
//   outputs of one stream; the chunks of a stream split its tiles (one chunk per stream when there are thousands of streams,
//   several when there are few: the same kernel, the same bits).
//
// Per tile:
//   stage   the input span the tile needs, [q_first - (T-1), q_last] widened to multiples of 8 samples, is read once with
//           16-byte non-temporal loads, converted, and written to the LDS as two planes of int16, I and Q apart (one
//           ds_write_b128 each per 8 samples).  Samples in front of the call come from the stream's history row, samples
//           behind its end are zeros; only the groups at those two edges take the sample-by-sample path.
//   FIR     thread t owns outputs t, t + 256, .. of the tile, both components; the accumulators start from the rounding
//           constant.  A window must start at a multiple of 4 samples to be read by ds_read_b64, so the tap table holds
//           four copies of every phase, behind 0 .. 3 zero taps: the window start is rounded down and the copy chosen by
//           what was cut off.  One loop step: three ds_read_b64 (taps, I, Q) and four v_dot2_i32_i16.
//   The thread's (q, r) advance by (256 M) div L and (256 M) mod L from output to output, across tiles too; the steps
//   come from the host, and the prologue's two small quotients from shifts and subtractions: the kernel divides nowhere.
// The tap table (up to 60 KB) sits in the LDS behind the planes; a larger one (L large) is read from global memory
// (TAPS_LDS = false), the same words at the same indices.  No fp64, float32 only in CF32's conversion, no atomics.
// The types, the small arithmetic, the formats' conversions and the launch of the eight instances live in
// nvx_rs_device.h, which the down-converter bank's kernel file includes too.
#include "nvx_rs_device.h"

template <int FMT, bool TAPS_LDS>
__global__ __launch_bounds__(NVX_RS_THREADS) void nvx_resample(const nvx_rs_args a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t *const plane_i = lds, *const plane_q = lds + NVX_RS_PLANE / 2, *const lds_taps = lds + NVX_RS_PLANE;
    constexpr int BPS = Fmt<FMT>::BPS, NV = Fmt<FMT>::NV, UNROLL = Fmt<FMT>::UNROLL;

    const int tid = threadIdx.x, stream = blockIdx.y;
    const char *const row = (const char *)a.in + (size_t)stream * a.pitch_in * BPS;
    uint32_t *const out = a.out + (size_t)stream * a.pitch_out + a.out_first;
    const uint32_t *const hist_in = a.hist_in + (size_t)stream * a.hist_pitch;
    const int L = a.L, T = a.T, n_in = a.n_in;

    if constexpr (TAPS_LDS)
        for (int i = tid * 4; i < a.tap_dw; i += NVX_RS_THREADS * 4) *(u32x4 *)&lds_taps[i] = *(const u32x4 *)&a.taps[i];

    const int tile_out = NVX_RS_THREADS * a.K;
    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;

    // The first output of the chunk's first tile (uniform), then this thread's first output.  Positions are kept as
    // (q, r) = (pos div L, pos mod L) and advanced by host-computed steps; the two quotients needed here are small and
    // come from a shift-and-subtract division: no division instruction sequence, no float, anywhere in the kernel.
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
                if (g + u * NVX_RS_THREADS < g1) load_group<FMT, true>(row, lo + (g + u * NVX_RS_THREADS) * NVX_RS_GROUP, v[u]);
#pragma unroll
            for (int u = 0; u < UNROLL; u++)
                if (g + u * NVX_RS_THREADS < g1) {
                    u32x4 I, Q;
                    convert_group<FMT>(v[u], I, Q);
                    *(u32x4 *)&plane_i[(g + u * NVX_RS_THREADS) * 4] = I;
                    *(u32x4 *)&plane_q[(g + u * NVX_RS_THREADS) * 4] = Q;
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

    // the stream's last T-1 converted samples for the next call: by the last chunk, into the row this launch does not read
    if (blockIdx.x == gridDim.x - 1) {
        uint32_t *const hist_out = a.hist_out + (size_t)stream * a.hist_pitch;
        for (int k = tid; k < T - 1; k += NVX_RS_THREADS) {
            const int idx = n_in - (T - 1) + k;
            hist_out[k] = idx >= 0 ? load_sample<FMT>(row, idx) : (a.hist_valid ? hist_in[T - 1 + idx] : 0u);
        }
    }
}

struct resample_family {
    template <int FMT, bool TAPS_LDS> static constexpr auto kernel = nvx_resample<FMT, TAPS_LDS>;
};

static const size_t LDS_MAX = NVX_RS_PLANE * 4 + NVX_RS_TAPS_LDS_MAX;

void nvx_rs_prepare(void) { nvx_rs_family_prepare<resample_family>(LDS_MAX); }

size_t nvx_rs_lds_bytes(const nvx_rs_args *a, bool taps_in_lds)
{
    return (size_t)NVX_RS_PLANE * 4 + (taps_in_lds ? (size_t)a->tap_dw * 4 : 0);
}

hipError_t nvx_rs_launch(const nvx_rs_args *a, int format, int n_streams, int chunks, bool taps_in_lds, hipStream_t s)
{
    const dim3 grid((unsigned)chunks, (unsigned)n_streams);
    return nvx_rs_family_launch<resample_family>(a, format, taps_in_lds, grid, nvx_rs_lds_bytes(a, taps_in_lds), LDS_MAX, s);
}
