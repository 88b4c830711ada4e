// nvx_zoom.hip -- the zoom bank's kernel (include/navtex_amd_zoom.h states the arithmetic; this file arranges it).
//
//   nvx_zoom_bank<FMT>   grid (chunks, inputs), 256 threads, all k stages and all zooms of an input fused: no intermediate rate
//   touches memory.  A workgroup walks consecutive blocks of 1024 input samples of one input, counted from the call's first
//   (rows are 16-byte aligned there); a block gives a tile of T = 1024 >> k outputs per zoom.  Every stage of every zoom has a
//   line in the LDS: its input's samples of the block behind the last 28 pairs of the block before.  So a block costs its own
//   samples only; a chunk pays the filters' history once, by walking NVX_ZOOM_WARM(k) blocks in front of its first tile
//   without storing (1 block for k <= 4, 2 for k = 5, 4 for k = 6, which cover H = 53 (2^k - 1) samples).
//
// Per block:
//   load     the block's samples, once whatever n_zooms is: 16-byte non-temporal loads by the first 256 (128 for the 8-bit
//            formats) threads, converted (nvx_rs_device.h), to the LDS as packed words.  In front of the call: the input's
//            state row, and zeros in front of that; behind the call's end: zeros.                            -- barrier
//   mix      a thread takes four consecutive samples and, for every zoom, mixes them with the table in the LDS (the bank's
//            mix: two v_dot2_i32_i16 and two clamps; kz = 0 copies) and writes them to the zoom's stage-1 line: the even and
//            the odd samples of I and of Q are four planes of int16.                                         -- barrier
//   stages   s = 1 .. k.  A work item is four consecutive outputs of one zoom, I and Q: for each component the 31 odd
//            samples they reach over come with eight ds_read_b64 (lane stride 8 bytes), fifteen funnel shifts (v_perm_b32 here) make the words
//            displaced by one sample, and the symmetric 28-tap row is fourteen packed immediates: fourteen
//            v_dot2_i32_i16 / v_dot2c_i32_i16 per output on the centre sample times 2^14.  Outputs 0 and 2 are two even
//            samples of the next stage's line and 1 and 3 two odd ones: one word each.  The last stage packs I and Q and
//            stores: 16 bytes, non-temporal, where the output rows are 16-byte aligned; word by word otherwise and for the
//            group the call's end cuts.                                              -- barrier behind every stage but the last
//   carry    one thread per plane (zooms * k * 4 <= 192) moves its last 28 entries to the front: fourteen words through
//            registers, a barrier between the reads and the writes (a short plane's source and destination overlap).
// The workgroup of an input's last sample writes the other state row: the last H samples of the input, from the call, or
// from the state row read where the call is shorter than that.
// Integers only, except CF32's conversion.
#include "nvx_zoom_plan.h"
#include "nvx_stream_device.h"

static_assert(NVX_ZOOM_CS16 == NVX_RS_CS16 && NVX_ZOOM_CU8 == NVX_RS_CU8 && NVX_ZOOM_CS8 == NVX_RS_CS8 && NVX_ZOOM_CF32 == NVX_RS_CF32, "formats");
static_assert(NVX_REAL_HISTORY == 28 && NVX_REAL_HISTORY <= NVX_ZOOM_LINE_AT && NVX_ZOOM_LINE_AT % 8 == 0, "the carried entries");
static_assert(NVX_ZOOM_STAGE_REACH == 2 * NVX_REAL_HISTORY - 3 && NVX_ZOOM_STAGE_DELAY == 2 * NVX_REAL_K, "the stage is the converter's row");
static_assert(NVX_ZOOM_BLOCK == 4 * NVX_ZOOM_THREADS && NVX_ZOOM_TILE(NVX_ZOOM_MAX_LOG2) % 4 == 0, "four samples per thread; groups of four outputs");
static_assert(NVX_ZOOM_WARM(NVX_ZOOM_MAX_LOG2) * NVX_ZOOM_BLOCK >= NVX_ZOOM_HISTORY(NVX_ZOOM_MAX_LOG2), "the warm-up covers the history");
static_assert(NVX_ZOOM_MAX_ZOOMS * NVX_ZOOM_MAX_LOG2 * 4 <= NVX_ZOOM_THREADS, "a thread per plane");
static_assert(NVX_ZOOM_LDS_STATIC + NVX_ZOOM_LDS_DYNAMIC(NVX_ZOOM_MAX_LOG2, NVX_ZOOM_MAX_ZOOMS) <= NVX_ZOOM_LDS_MAX, "the LDS");
static_assert(NVX_ZOOM_GRID == 4096, "the table");

static constexpr uint32_t GRID_MASK = NVX_ZOOM_GRID - 1;

// element t of the row over the odd samples o[m - 27 + t] = u[2m - 53 + 2t]: the taps (-1)^j A[j], j = 13 .. 0, 0 .. 13
constexpr int tap_signed(int j) { return j & 1 ? -NVX_REAL_TAPS[j] : NVX_REAL_TAPS[j]; }
constexpr int tap_row(int t) { return t < NVX_REAL_NTAPS ? tap_signed(NVX_REAL_K - t) : tap_signed(t - NVX_REAL_NTAPS); }
constexpr uint32_t tap_pair(int u) { return ((uint32_t)tap_row(2 * u) & 0xffffu) | ((uint32_t)tap_row(2 * u + 1) << 16); }

// a stage's output from fourteen words of odd samples and its centre sample
__device__ __forceinline__ int stage_sum(const uint32_t *x, int centre)
{
    constexpr uint32_t H[NVX_REAL_NTAPS] = { tap_pair(0), tap_pair(1), tap_pair(2), tap_pair(3), tap_pair(4), tap_pair(5), tap_pair(6),
                                             tap_pair(7), tap_pair(8), tap_pair(9), tap_pair(10), tap_pair(11), tap_pair(12), tap_pair(13) };
    int acc = centre * (1 << 14) + (1 << 14);
#pragma unroll
    for (int u = 0; u < NVX_REAL_NTAPS; u++) acc = dot2(x[u], H[u], acc);
    return clamp16(acc >> 15);
}

// outputs i0 .. i0 + 3 (i0 a multiple of 4, counted from the block's first) of a stage from the planes of the even and the
// odd samples of its input
__device__ __forceinline__ void stage4(const uint16_t *pe_plane, const uint16_t *po_plane, int i0, int (&v)[4])
{
    // the odd samples of pairs i0 - 28 .. i0 + 3: x[d] holds those of pairs i0 - 28 + 2 d and the next
    uint32_t x[16], y[15];
    const lds_vu2 *const po = (const lds_vu2 *)&po_plane[NVX_ZOOM_LINE_AT - NVX_REAL_HISTORY + i0];
#pragma unroll
    for (int d = 0; d < 8; d++) { const u32x2 w = po[d]; x[2 * d] = w.x; x[2 * d + 1] = w.y; }
    // the even samples of pairs i0 - 14 .. i0 - 9: output r has its centre at pair i0 + r - 13
    const uint32_t *const pe = (const uint32_t *)&pe_plane[NVX_ZOOM_LINE_AT - NVX_REAL_K - 1 + i0];
    const uint32_t e0 = pe[0], e1 = pe[1], e2 = pe[2];
#pragma unroll
    for (int d = 0; d < 15; d++) y[d] = __builtin_amdgcn_alignbit(x[d + 1], x[d], 16);
    // output r reaches over pairs i0 + r - 27 .. i0 + r
    v[0] = stage_sum(&y[0], (int)e0 >> 16);
    v[1] = stage_sum(&x[1], (int)(e1 << 16) >> 16);
    v[2] = stage_sum(&y[1], (int)e1 >> 16);
    v[3] = stage_sum(&x[2], (int)(e2 << 16) >> 16);
}

// the packed sample x = (I, Q) times W[j] = (c, s): the bank's mix
__device__ __forceinline__ uint32_t mix(uint32_t x, uint32_t w)
{
    const rs_short2 cs = __builtin_bit_cast(rs_short2, w);
    const rs_short2 sc = { (short)-cs.y, cs.x };                                // (-s, c): no entry is -32768
    const int yi = clamp16(dot2(x, w, 1 << 14) >> 15);
    const int yq = clamp16(dot2(x, __builtin_bit_cast(uint32_t, sc), 1 << 14) >> 15);
    return ((uint32_t)yi & 0xffffu) | ((uint32_t)yq << 16);
}

__device__ __forceinline__ uint32_t pack16(int lo, int hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }

template <int FMT>
__global__ __launch_bounds__(NVX_ZOOM_THREADS) void nvx_zoom_bank(const nvx_zoom_args a)
{
    constexpr int SPT = StreamLane<FMT>::SPT;
    __shared__ __attribute__((aligned(16))) uint32_t tab[NVX_ZOOM_GRID];
    __shared__ __attribute__((aligned(16))) uint32_t raw[NVX_ZOOM_BLOCK];
    extern __shared__ __attribute__((aligned(16))) uint16_t lines[];

    const int tid = threadIdx.x, input = blockIdx.y;
    const int k = a.log2_decim, Z = a.n_zooms, H = a.hist, n_in = a.n_in, n_out = a.n_out;
    const int zoom_entries = NVX_ZOOM_ZOOM_ENTRIES(k);
    const char *const row = (const char *)a.in + (size_t)input * a.pitch_in * Fmt<FMT>::BPS;
    uint32_t *const out = a.out + (size_t)input * Z * a.pitch_out + a.out_first;
    const uint32_t *const st = a.state_in + (size_t)input * H;
    const int *const kz = a.kz + (size_t)input * Z;
    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;

    // the table, and every line empty
    for (int t = tid; t < NVX_ZOOM_GRID / 4; t += NVX_ZOOM_THREADS) ((u32x4 *)tab)[t] = ((const u32x4 *)a.table)[t];
    for (int t = tid; t < Z * zoom_entries / 2; t += NVX_ZOOM_THREADS) ((uint32_t *)lines)[t] = 0u;
    // the plane this thread carries from block to block: plane `p` of stage `cs` of zoom `cz`
    const bool carries = tid < Z * k * 4;
    uint32_t *carry_from = nullptr, *carry_to = nullptr;
    if (carries) {
        const int p = tid & 3, q = tid >> 2, cz = q / k, cs = q - cz * k + 1;
        uint16_t *const plane = lines + cz * zoom_entries + NVX_ZOOM_STAGE_AT(cs) + p * NVX_ZOOM_PLANE(cs);
        carry_to = (uint32_t *)&plane[NVX_ZOOM_LINE_AT - NVX_REAL_HISTORY];
        carry_from = (uint32_t *)&plane[NVX_ZOOM_PLANE(cs) - NVX_REAL_HISTORY];
    }
    __syncthreads();

    for (int tile = tile0 - a.warm_tiles; tile < tile1; tile++) {
        const int base = tile * NVX_ZOOM_BLOCK;                     // of the call; negative in front of it
        // ---- load and convert
        if (tid < NVX_ZOOM_BLOCK / SPT) {
            const int s0 = base + tid * SPT;
            uint32_t w[SPT];
            if (s0 >= 0 && s0 + SPT <= n_in) load_words<FMT, true>(row, s0, w);
            else {
#pragma unroll
                for (int t = 0; t < SPT; t++) {
                    const int i = s0 + t;
                    uint32_t v = 0u;
                    if (i >= 0) { if (i < n_in) v = load_sample<FMT>(row, i); }
                    else if (i >= -H) v = st[H + i];
                    w[t] = v;
                }
            }
#pragma unroll
            for (int t = 0; t < SPT; t += 4) *(u32x4 *)&raw[tid * SPT + t] = u32x4{ w[t], w[t + 1], w[t + 2], w[t + 3] };
        }
        __syncthreads();

        // ---- mix: samples 4 tid .. 4 tid + 3 of the block, for every zoom, into its stage-1 line
        {
            const u32x4 v = *(const u32x4 *)&raw[tid * 4];
            const uint32_t x[4] = { v.x, v.y, v.z, v.w };
            const uint32_t n = a.n0 + (uint32_t)(base + tid * 4);   // the sample's position, mod 2^32: mod 4096 it is exact
            for (int z = 0; z < Z; z++) {
                const uint32_t kk = (uint32_t)kz[z] & GRID_MASK;    // uniform
                uint32_t m[4];
#pragma unroll
                for (int t = 0; t < 4; t++) m[t] = kk ? mix(x[t], tab[(kk * ((n + t) & GRID_MASK)) & GRID_MASK]) : x[t];
                uint16_t *const l1 = lines + z * zoom_entries + NVX_ZOOM_LINE_AT + 2 * tid;
                *(uint32_t *)&l1[0 * NVX_ZOOM_PLANE(1)] = lo_pair(m[0], m[2]);
                *(uint32_t *)&l1[1 * NVX_ZOOM_PLANE(1)] = lo_pair(m[1], m[3]);
                *(uint32_t *)&l1[2 * NVX_ZOOM_PLANE(1)] = hi_pair(m[0], m[2]);
                *(uint32_t *)&l1[3 * NVX_ZOOM_PLANE(1)] = hi_pair(m[1], m[3]);
            }
        }
        __syncthreads();

        // ---- the stages
        for (int s = 1; s <= k; s++) {
            const int outs = NVX_ZOOM_BLOCK >> s, log2_groups = 8 - s, plane = NVX_ZOOM_PLANE(s);      // outs / 4 groups per zoom
            const bool last = s == k;
            if (last && tile < tile0) break;                        // a warm-up block: nothing to store
            for (int w = tid; w < (Z << log2_groups); w += NVX_ZOOM_THREADS) {
                const int z = w >> log2_groups, i0 = (w & ((1 << log2_groups) - 1)) * 4;
                const uint16_t *const l = lines + z * zoom_entries + NVX_ZOOM_STAGE_AT(s);
                int vi[4], vq[4];
                stage4(l, l + plane, i0, vi);
                stage4(l + 2 * plane, l + 3 * plane, i0, vq);
                if (!last) {
                    const int next = NVX_ZOOM_PLANE(s + 1);
                    uint16_t *const l2 = lines + z * zoom_entries + NVX_ZOOM_STAGE_AT(s + 1) + NVX_ZOOM_LINE_AT + i0 / 2;
                    *(uint32_t *)&l2[0 * next] = pack16(vi[0], vi[2]);
                    *(uint32_t *)&l2[1 * next] = pack16(vi[1], vi[3]);
                    *(uint32_t *)&l2[2 * next] = pack16(vq[0], vq[2]);
                    *(uint32_t *)&l2[3 * next] = pack16(vq[1], vq[3]);
                } else {
                    const int m0 = tile * outs + i0;                // of the call
                    uint32_t *const dst = out + (size_t)z * a.pitch_out + m0;
                    const uint32_t word[4] = { pack16(vi[0], vq[0]), pack16(vi[1], vq[1]), pack16(vi[2], vq[2]), pack16(vi[3], vq[3]) };
                    if (a.out_vec && m0 + 4 <= n_out) {
                        const u32x4 v = { word[0], word[1], word[2], word[3] };
                        __builtin_nontemporal_store(v, (u32x4 *)dst);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            if (m0 + r < n_out) dst[r] = word[r];
                    }
                }
            }
            if (!last) __syncthreads();
        }

        // ---- every plane's last 28 entries go to its front
        uint32_t c[NVX_REAL_HISTORY / 2];
        if (carries) {
#pragma unroll
            for (int t = 0; t < NVX_REAL_HISTORY / 2; t++) c[t] = carry_from[t];
        }
        __syncthreads();
        if (carries) {
#pragma unroll
            for (int t = 0; t < NVX_REAL_HISTORY / 2; t++) carry_to[t] = c[t];
        }
        // the next block's first barrier stands between these writes and the stages' reads
    }

    // the input's state for the next call: by the workgroup of its last sample, into the row this launch does not read
    if (blockIdx.x == gridDim.x - 1) {
        uint32_t *const next = a.state_out + (size_t)input * H;
        for (int j = tid; j < H; j += NVX_ZOOM_THREADS) {
            const int at = n_in - H + j;                            // the sample, counted from the call's first
            next[j] = at >= 0 ? load_sample<FMT>(row, at) : st[n_in + j];
        }
    }
}

static const size_t LDS_DYNAMIC_MAX = NVX_ZOOM_LDS_DYNAMIC(NVX_ZOOM_MAX_LOG2, NVX_ZOOM_MAX_ZOOMS);

void nvx_zoom_prepare(void)
{
    const void *fns[] = { (const void *)nvx_zoom_bank<NVX_RS_CS16>, (const void *)nvx_zoom_bank<NVX_RS_CU8>, (const void *)nvx_zoom_bank<NVX_RS_CS8>,
                          (const void *)nvx_zoom_bank<NVX_RS_CF32> };
    // a runtime that does not know the attribute launches with whatever LDS the launch names; one that enforces it has it set
    for (const void *f : fns)
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_DYNAMIC_MAX) != hipSuccess) (void)hipGetLastError();
}

template <int FMT>
static hipError_t launch_one(const nvx_zoom_args *a, dim3 grid, size_t lds, hipStream_t s)
{
    hipLaunchKernelGGL((nvx_zoom_bank<FMT>), grid, dim3(NVX_ZOOM_THREADS), lds, s, *a);
    return hipGetLastError();
}

hipError_t nvx_zoom_launch(const nvx_zoom_args *a, int format, int n_inputs, int chunks, hipStream_t s)
{
    if (a->log2_decim < NVX_ZOOM_MIN_LOG2 || a->log2_decim > NVX_ZOOM_MAX_LOG2 || a->n_zooms < 1 || a->n_zooms > NVX_ZOOM_MAX_ZOOMS) return hipErrorInvalidValue;
    const dim3 grid((unsigned)chunks, (unsigned)n_inputs);
    const size_t lds = NVX_ZOOM_LDS_DYNAMIC(a->log2_decim, a->n_zooms);
    return nvx_for_format(format, [&](auto fmt) { return launch_one<decltype(fmt)::value>(a, grid, lds, s); });
}
