// nvx_notch.hip -- the tone notch's kernels (include/navtex_amd_notch.h states the arithmetic; this file arranges it).
//
// The sums and the apply kernels have the grid (chunks, rows) and 256 threads, and walk consecutive tiles of 4096 samples of
// one row, counted from the call's first sample (rows are 16-byte aligned there; the blocks of the contract, counted from the
// row's reset, are not).  Wave w owns samples [1024 w, 1024 w + 1024) of the tile; a lane takes four (8-bit formats: eight)
// consecutive samples from one 16-byte load, so a wave's step is 256 samples: one block where the call starts on a block's
// first sample, parts of two otherwise (8-bit formats: 512 samples, two blocks or parts of three).  Both hold the NCO table in
// the LDS as 4096 packed (c, s) words, 16 KB, filled from the copy the host made of nvx_ddc_table.h's numbers.
//
//   nvx_notch_sums<FMT>    B of every block the call touches, for every notch of the row.  Per sample and notch: the phase is
//       step * (position + i) in 32 bits, the table word comes from the LDS, and u is two v_dot2_i32_i16 of the packed sample,
//       against (c, s) and against (-s, c) (no table entry is -32768, so the negation fits).  A lane adds its samples of a
//       block in 64 bits, the wave reduces the lanes in three limbs, and the last lane writes the record of (row, block, notch): with
//       a plain 16-byte store where the call starts on a block's first sample (every block then lies in one step of one wave),
//       with two 64-bit atomic adds otherwise (exact in any order; the host zeroes the records in front of such a call).
//       Plain loads: the lines stay for the second pass.
//   nvx_notch_update       one lane per (row, notch): the offset readout X over the blocks that ended inside the call, and the
//       notch's carried sums for the next call -- the last 2R + 2 complete blocks and the open block's partial --, into the
//       state row this launch does not read.  It stops at 4096 pairs, so in a steady stream it only moves the sums.
//   nvx_notch_apply<FMT>   per tile, 18 K threads form the 18 values of M the tile's words touch, each from the 2R - 1 block
//       sums around it (the carried ones in front of the call, the call's records behind), into the LDS.  Then per word i of
//       the call, which is y[position + i - D]: x from the delay line (i < D) or from the call's input (i - D is a multiple of
//       the lane's group where i is, so the 16-byte loads stay aligned), the two values of M interpolated in 64 bits, the
//       amplitude, the table word at the phase of that sample, e in 64 bits (a c reaches 2^35 at the rails), the rounding
//       shift, the sum over the enabled notches, v_med3 clamps and a pack; 16-byte non-temporal stores where the output rows
//       are 16-byte aligned.  The workgroup of a row's last sample writes the new delay line into the other state row.
// The formats' sizes, load_words, load_sample and the CF32 rule are the resampler's (nvx_rs_device.h).  The step's shape,
// the wave sums in the last lane, in_vector_registers and the dispatch on the format are the same-rate companions'
// (nvx_stream_device.h); the group load stays here, for its clamped-index tail.
#include "nvx_notch_plan.h"
#include "nvx_stream_device.h"

static_assert(NVX_NOTCH_CS16 == NVX_RS_CS16 && NVX_NOTCH_CU8 == NVX_RS_CU8 && NVX_NOTCH_CS8 == NVX_RS_CS8 && NVX_NOTCH_CF32 == NVX_RS_CF32, "formats");

typedef i64 i64x2 __attribute__((ext_vector_type(2)));

// samples per lane and step, samples of a wave's step, steps per region, and the blocks a step can reach behind its first
template <int FMT> struct Shape : StreamShape<FMT, NVX_NOTCH_REGION> { static constexpr int REACH = Shape::STEP / NVX_NOTCH_BLOCK; };

// the table, from the host's copy to the LDS: four 16-byte words per thread
__device__ __forceinline__ void fill_table(uint32_t *tab, const uint32_t *src, int tid)
{
    for (int t = tid; t < NVX_NOTCH_TABLE / 4; t += NVX_NOTCH_THREADS) ((u32x4 *)tab)[t] = ((const u32x4 *)src)[t];
    __syncthreads();
}

// the SPT words of a lane's group at call index `base` of `row_src`, whose sample 0 is call index `first`; those behind the
// call's end are zero
template <int FMT, bool NONTEMPORAL>
__device__ __forceinline__ void load_group_words(const char *row_src, int first, int base, int n_in, uint32_t *w)
{
    constexpr int SPT = Shape<FMT>::SPT;
    if (base + SPT <= n_in) load_words<FMT, NONTEMPORAL>(row_src, base - first, w);
    else {
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            // no branch per sample: the call's last sample is read in place of one behind it, or the row's first where the
            // call ends in front of `first` (a step of 512 samples can reach over the delay while the call does not)
            const int at = (base + k < n_in ? base + k : n_in - 1) - first;
            const uint32_t v = load_sample<FMT>(row_src, at > 0 ? at : 0);
            w[k] = base + k < n_in ? v : 0u;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ sums
template <int FMT>
__global__ __launch_bounds__(NVX_NOTCH_THREADS) void nvx_notch_sums(const nvx_notch_args a)
{
    constexpr int SPT = Shape<FMT>::SPT, STEP = Shape<FMT>::STEP, STEPS = Shape<FMT>::STEPS, REACH = Shape<FMT>::REACH;
    __shared__ __attribute__((aligned(16))) uint32_t tab[NVX_NOTCH_TABLE];
    const int tid = threadIdx.x, lane = tid & 63, row = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    fill_table(tab, a.table, tid);
    const char *const src = (const char *)a.in + (size_t)row * a.pitch_in * Fmt<FMT>::BPS;
    const uint32_t *const cfg = a.cfg + (size_t)row * a.cfg_words;
    u64 *const records = a.records + (size_t)row * a.blocks * a.n_notches * 2;
    const int n_in = a.n_in, K = a.n_notches;
    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;

    for (int tile = tile0; tile < tile1; tile++) {
#pragma unroll 1
        for (int j = 0; j < STEPS; j++) {
            const int s0 = tile * NVX_NOTCH_TILE + wave * NVX_NOTCH_REGION + j * STEP;        // the step's first sample: uniform
            if (s0 >= n_in) break;
            const int base = s0 + lane * SPT;
            uint32_t w[SPT];
            load_group_words<FMT, false>(src, 0, base, n_in, w);
            // the blocks the step's samples lie in, counted from the call's first: r0 .. r_last <= r0 + REACH, all below a.blocks
            const int s1 = s0 + STEP < n_in ? s0 + STEP : n_in;
            const int r0 = (a.off0 + s0) >> 8, r_last = (a.off0 + s1 - 1) >> 8;
            const int q0 = ((a.off0 + base) >> 8) - r0;             // of this lane's first sample
            const int to_next = NVX_NOTCH_BLOCK - ((a.off0 + base) & (NVX_NOTCH_BLOCK - 1));      // its samples in front of the next block
#pragma unroll 1
            for (int k = 0; k < K; k++) {
                const uint32_t step = cfg[2 + 2 * k];
                uint32_t ph = step * (a.in_lo + (uint32_t)base);
                i64 re[REACH + 1] = {}, im[REACH + 1] = {};
                // formed again for every notch: kept, the comparisons below hold two scalar registers per sample and block
                int q_first = q0;
                asm volatile("" : "+v"(q_first));
#pragma unroll
                for (int t = 0; t < SPT; t++) {
                    const uint32_t cs = tab[ph >> 20];
                    const uint32_t sc = ((0u - (cs >> 16)) & 0xffffu) | (cs << 16);               // (-s, c)
                    const int ur = dot2(w[t], cs, 0), ui = dot2(w[t], sc, 0);
                    const int q = q_first + (t >= to_next ? 1 : 0);      // a lane's group reaches one block end at most
#pragma unroll
                    for (int b = 0; b <= REACH; b++) { re[b] += q == b ? ur : 0; im[b] += q == b ? ui : 0; }
                    ph += step;
                }
#pragma unroll
                for (int b = 0; b <= REACH; b++) {
                    if (r0 + b > r_last) break;                     // uniform
                    const i64 tr = wave_sum64_in_last_lane(re[b]), ti = wave_sum64_in_last_lane(im[b]);
                    if (lane == 63) {
                        // the address through vector registers: a uniform one has the compiler sum the (one) active lane's
                        // values in a scalar loop in front of each atomic
                        u64 *const rec = records + in_vector_registers((i64)((size_t)(r0 + b) * K + k) * 2);
                        if (a.off0 == 0) *(i64x2 *)rec = i64x2{ tr, ti };
                        else { atomicAdd(&rec[0], (u64)tr); atomicAdd(&rec[1], (u64)ti); }
                    }
                }
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------- block sums and M
// The sums of one notch as a call sees them: block j, counted from the call's first, is a carried one in front of the call
// (hist[H + j]; zero where the notch starts anew with this call) and the call's record behind, the first with the open block's
// carried partial.  Blocks the call does not reach are zero: only words behind the call's end would interpolate from them.
struct NotchSums {
    const i64 *st;            // the notch's carried words
    const u64 *rec;           // the row's records, at this notch: K * 2 words from block to block
    int H, K, blocks;
    bool fresh;

    __device__ __forceinline__ i64x2 block(int j) const
    {
        if (j < 0) return fresh || j < -H ? i64x2{ 0, 0 } : *(const i64x2 *)(st + 2 * (H + j));
        if (j >= blocks) return i64x2{ 0, 0 };
        i64x2 v = *(const i64x2 *)(rec + (size_t)j * K * 2);
        if (j == 0 && !fresh) v += *(const i64x2 *)(st + 2 * H + NVX_NOTCH_ST_PARTIAL);
        return v;
    }
    // M[b]: components within 2^(39 + 2r)
    __device__ __forceinline__ i64x2 smooth(int b, int R) const
    {
        i64x2 m = block(b) * (i64)R;
#pragma unroll 1
        for (int k = 1; k < R; k++) m += (block(b - k) + block(b + k)) * (i64)(R - k);
        return m;
    }
};

__device__ __forceinline__ NotchSums notch_sums(const nvx_notch_args &a, int row, int k, const i64 *row_state, const uint32_t *row_cfg)
{
    NotchSums s;
    s.st = row_state + NVX_NOTCH_ROW_SCALARS + (size_t)k * a.notch_words;
    s.rec = a.records + ((size_t)row * a.blocks * a.n_notches + k) * 2;
    s.H = a.hist; s.K = a.n_notches; s.blocks = a.blocks;
    s.fresh = (row_cfg[0] & NVX_NOTCH_ROW_RESET) || (row_cfg[3 + 2 * k] & NVX_NOTCH_RESTART);
    return s;
}

// ---------------------------------------------------------------------------------------------------------------- update
__global__ __launch_bounds__(64) void nvx_notch_update(const nvx_notch_args a)
{
    const int id = (int)(blockIdx.x * 64 + threadIdx.x);
    if (id >= a.n_rows * a.n_notches) return;
    const int row = id / a.n_notches, k = id - row * a.n_notches;
    const i64 *const st = a.state_in + (size_t)row * a.state_words;
    i64 *const so = a.state_out + (size_t)row * a.state_words;
    const uint32_t *const cfg = a.cfg + (size_t)row * a.cfg_words;
    const NotchSums s = notch_sums(a, row, k, st, cfg);
    const int H = a.hist, R = 1 << a.width_log2, r = a.width_log2;
    const bool reset = cfg[0] & NVX_NOTCH_ROW_RESET;
    if (k == 0) { so[0] = reset ? a.position : st[0]; so[1] = 0; }

    const bool anew = s.fresh || (cfg[3 + 2 * k] & NVX_NOTCH_MEASURE);
    const i64 b0 = a.position >> 8;                                 // the call's first block
    i64 x_re = anew ? 0 : s.st[2 * H + NVX_NOTCH_ST_X], x_im = anew ? 0 : s.st[2 * H + NVX_NOTCH_ST_X + 1];
    i64 pairs = anew ? 0 : s.st[2 * H + NVX_NOTCH_ST_PAIRS];
    const i64 from = anew ? (a.position + NVX_NOTCH_BLOCK - 1) >> 8 : s.st[2 * H + NVX_NOTCH_ST_FROM];
    // block c (counted from the call's first) has ended: the pair (b, b - 1) with b = c - (R - 1), whose oldest block is
    // b - R = c - 2R + 1; that one lies behind the restart from c = from - b0 + 2R - 1 on
    i64 c_first = from - b0 + 2 * R - 1;
    if (c_first < 0) c_first = 0;
    i64x2 prev = {};
    bool have = false;
    for (i64 c = c_first; c < a.done && pairs < NVX_NOTCH_MAX_PAIRS; c++) {
        const int b = (int)c - (R - 1);
        if (!have) prev = s.smooth(b - 1, R) >> (i64)(2 * r + 15);
        const i64x2 cur = s.smooth(b, R) >> (i64)(2 * r + 15);
        x_re += cur.x * prev.x + cur.y * prev.y;
        x_im += cur.y * prev.x - cur.x * prev.y;
        pairs++;
        prev = cur; have = true;
    }
    i64 *const no = so + NVX_NOTCH_ROW_SCALARS + (size_t)k * a.notch_words;
    for (int j = 0; j < H; j++) *(i64x2 *)(no + 2 * j) = s.block(a.done - H + j);
    const bool open = ((a.off0 + a.n_in) & (NVX_NOTCH_BLOCK - 1)) != 0;
    *(i64x2 *)(no + 2 * H + NVX_NOTCH_ST_PARTIAL) = open ? s.block(a.done) : i64x2{ 0, 0 };
    no[2 * H + NVX_NOTCH_ST_X] = x_re; no[2 * H + NVX_NOTCH_ST_X + 1] = x_im;
    no[2 * H + NVX_NOTCH_ST_PAIRS] = pairs; no[2 * H + NVX_NOTCH_ST_FROM] = from;
}

// ----------------------------------------------------------------------------------------------------------------- apply
template <int FMT>
__global__ __launch_bounds__(NVX_NOTCH_THREADS) void nvx_notch_apply(const nvx_notch_args a)
{
    constexpr int SPT = Shape<FMT>::SPT, STEP = Shape<FMT>::STEP, STEPS = Shape<FMT>::STEPS;
    __shared__ __attribute__((aligned(16))) uint32_t tab[NVX_NOTCH_TABLE];
    __shared__ i64x2 mt[NVX_NOTCH_MAX_NOTCHES][NVX_NOTCH_TILE_M];
    const int tid = threadIdx.x, lane = tid & 63, row = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    fill_table(tab, a.table, tid);
    const char *const src = (const char *)a.in + (size_t)row * a.pitch_in * Fmt<FMT>::BPS;
    uint32_t *const out = a.out + (size_t)row * a.pitch_out + a.out_first;
    const i64 *const st = a.state_in + (size_t)row * a.state_words;
    const uint32_t *const cfg = a.cfg + (size_t)row * a.cfg_words;
    const uint32_t *const line = (const uint32_t *)(st + NVX_NOTCH_DELAY_AT(a.width_log2, a.n_notches));
    const int n_in = a.n_in, K = a.n_notches, D = a.delay, R = 1 << a.width_log2;
    const int sh = 27 + 2 * a.width_log2;
    const i64 half = (i64)1 << (sh - 1);
    // words in front of the row's reset position are zero: word i of the call where position + i - D < start
    const i64 start = (cfg[0] & NVX_NOTCH_ROW_RESET) ? a.position : st[0];
    const i64 z = start - a.position + D;
    const int zero_to = z <= 0 ? 0 : (z > n_in ? n_in : (int)z);
    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;

    for (int tile = tile0; tile < tile1; tile++) {
        const int tbase = tile * NVX_NOTCH_TILE;
        const int lo0 = (a.g0 + tbase) >> 8;                        // the tile's first value of M, in blocks from the call's first
        __syncthreads();                                            // the tile before has read its values
        if (tid < K * NVX_NOTCH_TILE_M) {
            const int k = tid / NVX_NOTCH_TILE_M, v = tid - k * NVX_NOTCH_TILE_M;
            mt[k][v] = notch_sums(a, row, k, st, cfg).smooth(lo0 + v, R);
        }
        __syncthreads();
#pragma unroll 1
        for (int j = 0; j < STEPS; j++) {
            const int s0 = tbase + wave * NVX_NOTCH_REGION + j * STEP;
            if (s0 >= n_in) break;
            const int base = s0 + lane * SPT;
            uint32_t w[SPT];
            // D is a multiple of a lane's group: the group lies in the delay line or in the call's input, and stays aligned
            if (base < D) {
#pragma unroll
                for (int t = 0; t < SPT; t += 4) {
                    const u32x4 v = *(const u32x4 *)&line[base + t];
                    w[t] = v.x; w[t + 1] = v.y; w[t + 2] = v.z; w[t + 3] = v.w;
                }
            } else load_group_words<FMT, true>(src, D, base, n_in, w);
            int ei[SPT] = {}, eq[SPT] = {};
#pragma unroll 1
            for (int k = 0; k < K; k++) {
                if (!(cfg[3 + 2 * k] & NVX_NOTCH_ENABLED)) continue;        // uniform
                const uint32_t step = cfg[2 + 2 * k];
                uint32_t ph = step * (a.out_lo + (uint32_t)base);
#pragma unroll
                for (int t = 0; t < SPT; t++) {
                    const int g = a.g0 + base + t, lo = (g >> 8) - lo0, f = g & 255;
                    const i64x2 m = mt[k][lo] * (i64)(256 - f) + mt[k][lo + 1] * (i64)f;
                    const i64 a_re = (m.x + half) >> sh, a_im = (m.y + half) >> sh;           // within 2^20
                    const uint32_t cs = tab[ph >> 20];
                    const i64 c = (int)(cs << 16) >> 16, s = (int)cs >> 16;
                    ei[t] += (int)((a_re * c - a_im * s + (1 << 18)) >> 19);
                    eq[t] += (int)((a_re * s + a_im * c + (1 << 18)) >> 19);
                    ph += step;
                }
            }
#pragma unroll
            for (int t = 0; t < SPT; t++) {
                const int yi = clamp16(((int)(w[t] << 16) >> 16) - ei[t]), yq = clamp16(((int)w[t] >> 16) - eq[t]);
                w[t] = base + t < zero_to ? 0u : ((uint32_t)yi & 0xffffu) | ((uint32_t)yq << 16);
            }
            uint32_t *const dst = out + base;
            if (a.out_vec && base + SPT <= n_in) {
#pragma unroll
                for (int t = 0; t < SPT; t += 4) {
                    const u32x4 v = { w[t], w[t + 1], w[t + 2], w[t + 3] };
                    __builtin_nontemporal_store(v, (u32x4 *)&dst[t]);
                }
            } else {
#pragma unroll
                for (int t = 0; t < SPT; t++)
                    if (base + t < n_in) dst[t] = w[t];
            }
        }
    }

    // the row's delay line for the next call: the last D converted words, by the workgroup of the row's last sample, into the
    // row this launch does not read
    if (blockIdx.x == gridDim.x - 1) {
        uint32_t *const next = (uint32_t *)(a.state_out + (size_t)row * a.state_words + NVX_NOTCH_DELAY_AT(a.width_log2, a.n_notches));
        for (int j = tid; j < D; j += NVX_NOTCH_THREADS) {
            const int i = n_in - D + j;                             // the call's sample that lands in word j
            next[j] = i >= 0 ? load_sample<FMT>(src, i) : line[n_in + j];
        }
    }
}

template <int FMT>
static hipError_t launch_all(const nvx_notch_args *a, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((nvx_notch_sums<FMT>), grid, dim3(NVX_NOTCH_THREADS), 0, s, *a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nvx_notch_update, dim3((unsigned)((a->n_rows * a->n_notches + 63) / 64)), dim3(64), 0, s, *a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((nvx_notch_apply<FMT>), grid, dim3(NVX_NOTCH_THREADS), 0, s, *a);
    return hipGetLastError();
}

hipError_t nvx_notch_launch(const nvx_notch_args *a, int format, int n_rows, int chunks, hipStream_t s)
{
    const dim3 grid((unsigned)chunks, (unsigned)n_rows);
    return nvx_for_format(format, [&](auto fmt) { return launch_all<decltype(fmt)::value>(a, grid, s); });
}
