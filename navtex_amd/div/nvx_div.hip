// nvx_div.hip -- the diversity combiner's three kernels (include/navtex_amd_div.h states the arithmetic; this file arranges it).
//
// The sums and the apply kernels have the grid (chunks, pairs) and 256 threads, and walk consecutive tiles of 4096 samples of
// one pair, counted from the call's first sample (rows are 16-byte aligned there; the blocks and cells of the contract,
// counted from the pair's reset, are not).  Wave w owns samples [1024 w, 1024 w + 1024) of the tile; a lane takes four (8-bit
// formats: eight) consecutive samples of each row from one 16-byte load, so a wave's step is 256 samples: one block where the
// call starts on a block's first sample, parts of two otherwise (8-bit formats: 512 samples, two blocks or parts of three).
//
//   nvx_div_sums<FMT>    A and B of every block the call touches, for every target, from one read of the two rows.  The NCO
//       table lies in the LDS as 4096 packed (c, s) words, 16 KB, filled from the copy the host made of nvx_ddc_table.h's
//       numbers.  Per sample and target: the phase is step * (position + i) in 32 bits, the table word comes from the LDS, and
//       u is two v_dot2_i32_i16 of each row's packed sample, against (c, s) and against (-s, c) (no table entry is -32768, so
//       the negation fits).  A lane adds its samples of a block in 64 bits, the wave reduces the lanes in three limbs, and the
//       last lane writes the record of (pair, block, target): with plain 16-byte stores where the call starts on a block's
//       first sample (every block then lies in one step of one wave), with 64-bit atomic adds otherwise (exact in any order;
//       the host zeroes the records in front of such a call).  Plain loads: the lines stay for the second pass.  This is the
//       tone notch's sums kernel (navtex_amd/notch/nvx_notch.hip) with two rows in place of one.
//   nvx_div_fold         one wave per (pair, target).  It walks the cells the call touches in order: at a cell's first sample
//       it solves where the contract says so (the ring of the last W cell sums lies in the LDS; nvx_div_solve.h is the solve),
//       writes the cell's (lead, weight) to the call's list, then folds the cell's blocks that ended inside the call -- a lane
//       takes every 64th, shifts A and B down and forms the four products, the wave reduces -- and, where the cell ends inside
//       the call, puts its sums into the ring.  Then it writes the other state row and adds to the counters.
//   nvx_div_apply<FMT>   both rows again, with non-temporal loads.  A tile is shorter than a cell, so at most one cell ends
//       inside it; a wave's step lies in one cell, or -- one step of one wave of one tile in sixteen -- a cell's end cuts it.
//       Per target (lead, weight) of the cell come from the list, and per sample two v_dot2_i32_i16 of the weak row's word
//       against the packed pairs (w_re, -w_im) and (w_im, w_re) with 4096 as the accumulator, a shift, an addition, two
//       v_med3_i32 and a pack; 16-byte non-temporal stores where the output rows are 16-byte aligned.
// The formats' sizes, load_words, load_sample and the CF32 rule are the resampler's (nvx_rs_device.h).  The step's shape, load
// and store, the wave sums, in_vector_registers and the dispatch on the format are the same-rate companions'
// (nvx_stream_device.h); the group load with its clamped-index tail is the notch's.
#include "nvx_div_plan.h"
#include "nvx_div_solve.h"
#include "nvx_stream_device.h"

static_assert(NVX_DIV_CS16 == NVX_RS_CS16 && NVX_DIV_CU8 == NVX_RS_CU8 && NVX_DIV_CS8 == NVX_RS_CS8 && NVX_DIV_CF32 == NVX_RS_CF32, "formats");
static_assert(NVX_DIV_TILE < NVX_DIV_CELL && NVX_DIV_CELL % NVX_DIV_TILE == 0 && NVX_DIV_CELL % NVX_DIV_BLOCK == 0, "a tile holds at most one cell end");

typedef i64 i64x2 __attribute__((ext_vector_type(2)));

// samples per lane and step, samples of a wave's step, steps per region, and the blocks a step can reach behind its first
template <int FMT> struct Shape : StreamShape<FMT, NVX_DIV_REGION> { static constexpr int REACH = Shape::STEP / NVX_DIV_BLOCK; };

// the SPT words of a lane's group at call index `base` of `row_src`; those behind the call's end are zero
template <int FMT, bool NONTEMPORAL>
__device__ __forceinline__ void load_group_words(const char *row_src, int base, int n_in, uint32_t *w)
{
    constexpr int SPT = Shape<FMT>::SPT;
    if (base + SPT <= n_in) load_words<FMT, NONTEMPORAL>(row_src, base, w);
    else {
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            // no branch per sample: the call's last sample is read in place of one behind it
            const uint32_t v = load_sample<FMT>(row_src, base + k < n_in ? base + k : n_in - 1);
            w[k] = base + k < n_in ? v : 0u;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ sums
template <int FMT>
__global__ __launch_bounds__(NVX_DIV_THREADS) void nvx_div_sums(const nvx_div_args a)
{
    constexpr int SPT = Shape<FMT>::SPT, STEP = Shape<FMT>::STEP, STEPS = Shape<FMT>::STEPS, REACH = Shape<FMT>::REACH;
    __shared__ __attribute__((aligned(16))) uint32_t tab[NVX_DIV_TABLE];
    const int tid = threadIdx.x, lane = tid & 63, pair = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the table, from the host's copy: four 16-byte words per thread
    for (int t = tid; t < NVX_DIV_TABLE / 4; t += NVX_DIV_THREADS) ((u32x4 *)tab)[t] = ((const u32x4 *)a.table)[t];
    __syncthreads();
    const char *const src_a = (const char *)a.in_main + (size_t)pair * a.pitch_main * Fmt<FMT>::BPS;
    const char *const src_b = (const char *)a.in_second + (size_t)pair * a.pitch_second * Fmt<FMT>::BPS;
    const uint32_t *const cfg = a.cfg + (size_t)pair * a.cfg_words;
    const int n_in = a.n_in, K = a.n_targets;
    u64 *const records = a.records + (size_t)pair * a.blocks * K * NVX_DIV_SUMS;
    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;

    for (int tile = tile0; tile < tile1; tile++) {
#pragma unroll 1
        for (int j = 0; j < STEPS; j++) {
            const int s0 = tile * NVX_DIV_TILE + wave * NVX_DIV_REGION + j * STEP;            // the step's first sample: uniform
            if (s0 >= n_in) break;
            const int base = s0 + lane * SPT;
            uint32_t wa[SPT], wb[SPT];
            load_group_words<FMT, false>(src_a, base, n_in, wa);
            load_group_words<FMT, false>(src_b, base, n_in, wb);
            // the blocks the step's samples lie in, counted from the call's first: r0 .. r_last <= r0 + REACH, all below a.blocks
            const int s1 = s0 + STEP < n_in ? s0 + STEP : n_in;
            const int r0 = (a.off0 + s0) >> 8, r_last = (a.off0 + s1 - 1) >> 8;
            const int q0 = ((a.off0 + base) >> 8) - r0;             // of this lane's first sample
            const int to_next = NVX_DIV_BLOCK - ((a.off0 + base) & (NVX_DIV_BLOCK - 1));          // its samples in front of the next block
#pragma unroll 1
            for (int k = 0; k < K; k++) {
                const uint32_t step = cfg[2 + NVX_DIV_CFG_TARGET * k + NVX_DIV_CFG_STEP];
                uint32_t ph = step * (a.in_lo + (uint32_t)base);
                // a lane's group reaches one block end at most: its samples in front of it (block q0) and behind it (block q0 + 1)
                i64 front[NVX_DIV_SUMS] = {}, back[NVX_DIV_SUMS] = {};
#pragma unroll
                for (int t = 0; t < SPT; t++) {
                    const uint32_t cs = tab[ph >> 20];
                    const uint32_t sc = ((0u - (cs >> 16)) & 0xffffu) | (cs << 16);               // (-s, c)
                    const int u[NVX_DIV_SUMS] = { dot2(wa[t], cs, 0), dot2(wa[t], sc, 0), dot2(wb[t], cs, 0), dot2(wb[t], sc, 0) };
                    const bool behind = t >= to_next;
#pragma unroll
                    for (int i = 0; i < NVX_DIV_SUMS; i++) { front[i] += behind ? 0 : u[i]; back[i] += behind ? u[i] : 0; }
                    ph += step;
                }
#pragma unroll
                for (int b = 0; b <= REACH; b++) {
                    if (r0 + b > r_last) break;                     // uniform
                    i64 v[NVX_DIV_SUMS];
#pragma unroll
                    for (int i = 0; i < NVX_DIV_SUMS; i++) v[i] = wave_sum64_in_last_lane((q0 == b ? front[i] : 0) + (q0 + 1 == b ? back[i] : 0));
                    const i64 s_ar = v[0], s_ai = v[1], s_br = v[2], s_bi = v[3];
                    if (lane == 63) {
                        // the address through vector registers: a uniform one has the compiler sum the (one) active lane's
                        // values in a scalar loop in front of each atomic
                        u64 *const rec = records + in_vector_registers((i64)((size_t)(r0 + b) * K + k) * NVX_DIV_SUMS);
                        if (a.off0 == 0) { *(i64x2 *)rec = i64x2{ s_ar, s_ai }; *(i64x2 *)(rec + 2) = i64x2{ s_br, s_bi }; }
                        else {
                            atomicAdd(&rec[0], (u64)s_ar); atomicAdd(&rec[1], (u64)s_ai);
                            atomicAdd(&rec[2], (u64)s_br); atomicAdd(&rec[3], (u64)s_bi);
                        }
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ fold
__global__ __launch_bounds__(64) void nvx_div_fold(const nvx_div_args a)
{
    __shared__ i64 ring[NVX_DIV_SUMS * 16];
    const int lane = threadIdx.x, K = a.n_targets;
    const int pair = (int)blockIdx.x / K, t = (int)blockIdx.x - pair * K;
    const int W = 1 << a.window_log2;
    const i64 *const st = a.state_in + ((size_t)pair * K + t) * a.state_words;
    i64 *const so = a.state_out + ((size_t)pair * K + t) * a.state_words;
    const i64 *const cell_in = st + NVX_DIV_SUMS * W, *const block_in = cell_in + NVX_DIV_SUMS, *const sc = block_in + NVX_DIV_SUMS;
    const uint32_t *const cfg = a.cfg + (size_t)pair * a.cfg_words, *const tc = cfg + 2 + NVX_DIV_CFG_TARGET * t;
    const uint32_t flags = tc[NVX_DIV_CFG_FLAGS];
    const bool fresh = (cfg[0] & NVX_DIV_PAIR_RESET) || (flags & NVX_DIV_RESTART);
    const int mode = (flags & NVX_DIV_HELD) ? NVX_DIV_HOLD : NVX_DIV_TRACK;
    const i64 F = fresh ? (a.position + NVX_DIV_CELL - 1) >> 16 : sc[NVX_DIV_ST_FIRST];
    int32_t lead = fresh ? 0 : (int32_t)sc[NVX_DIV_ST_LEAD], w_re = fresh ? 0 : (int32_t)sc[NVX_DIV_ST_WRE], w_im = fresh ? 0 : (int32_t)sc[NVX_DIV_ST_WIM];
    int32_t coherence = fresh ? 0 : (int32_t)sc[NVX_DIV_ST_COHERENCE], reason = fresh ? 0 : (int32_t)sc[NVX_DIV_ST_REASON];
    if (flags & NVX_DIV_SET) { lead = (int32_t)tc[NVX_DIV_CFG_LEAD]; w_re = (int32_t)tc[NVX_DIV_CFG_WRE]; w_im = (int32_t)tc[NVX_DIV_CFG_WIM]; }
    if (lane < NVX_DIV_SUMS * W) ring[lane] = fresh ? 0 : st[lane];
    __syncthreads();

    const i64 b0 = a.position >> 8, c0 = a.position >> 16;
    const u64 *const rec = a.records + ((size_t)pair * a.blocks * K + t) * NVX_DIV_SUMS;          // K * NVX_DIV_SUMS words from block to block
    nvx_div_weight *const list = a.weights + (size_t)pair * a.cells * K + t;                       // K entries from cell to cell
    // A and B of block j, counted from the call's first: the call's record, the first with the open block's carried partial
    auto block = [&](int j, int k) -> i64 {
        const i64 v = (i64)rec[(size_t)j * K * NVX_DIV_SUMS + k];
        return j == 0 && !fresh ? v + block_in[k] : v;
    };
    u64 solved = 0, rejected = 0;
    i64 open[NVX_DIV_SUMS] = {};                                    // the sums of the cell the call ends in
#pragma unroll 1
    for (int jc = 0; jc < a.cells; jc++) {
        const i64 c = c0 + jc;
        // the cell's first sample lies in this call
        if ((jc > 0 || a.cell_off == 0) && mode == NVX_DIV_TRACK && c >= F + W) {
            i64 tt[NVX_DIV_SUMS];
#pragma unroll
            for (int k = 0; k < NVX_DIV_SUMS; k++) {
                // the sums are uniform: through vector registers, or the whole solve is scalar code
                tt[k] = in_vector_registers(wave_sum64(lane < W ? ring[lane * NVX_DIV_SUMS + k] : 0));
            }
            reason = nvx_div_solve(tt[0], tt[1], tt[2], tt[3], &lead, &w_re, &w_im, &coherence);
            if (reason) rejected++; else solved++;
        }
        if (lane == 0) list[(size_t)jc * K] = nvx_div_weight{ lead, w_re, w_im, 0 };
        // the cell's blocks that ended inside the call; those in front of the first counted cell are not summed
        i64 jlo = c * 256 - b0, jhi = (c + 1) * 256 - b0;
        if (jlo < 0) jlo = 0;
        if (jhi > a.done) jhi = a.done;
        i64 acc[NVX_DIV_SUMS] = {};
        if (c >= F) {
#pragma unroll 1
            for (int j = (int)jlo + lane; j < (int)jhi; j += 64) {
                const i64 ar = block(j, 0) >> 16, ai = block(j, 1) >> 16, br = block(j, 2) >> 16, bi = block(j, 3) >> 16;
                acc[0] += ar * ar + ai * ai; acc[1] += br * br + bi * bi;
                acc[2] += ar * br + ai * bi; acc[3] += ai * br - ar * bi;
            }
        }
        i64 s[NVX_DIV_SUMS];
#pragma unroll
        for (int k = 0; k < NVX_DIV_SUMS; k++) s[k] = wave_sum64(acc[k]) + (jc == 0 && !fresh ? cell_in[k] : 0);
        __syncthreads();                                            // the solve has read the ring
        if (jc < a.cells_done) {
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < NVX_DIV_SUMS; k++) ring[(int)(c & (W - 1)) * NVX_DIV_SUMS + k] = s[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < NVX_DIV_SUMS; k++) open[k] = s[k];
        }
        __syncthreads();
    }

    // the target's state for the next call, into the row this launch does not read
    if (lane < NVX_DIV_SUMS * W) so[lane] = ring[lane];
    if (lane == 0) {
        i64 *const cell_out = so + NVX_DIV_SUMS * W, *const block_out = cell_out + NVX_DIV_SUMS, *const out = block_out + NVX_DIV_SUMS;
        const bool block_open = ((a.off0 + a.n_in) & (NVX_DIV_BLOCK - 1)) != 0;
#pragma unroll
        for (int k = 0; k < NVX_DIV_SUMS; k++) { cell_out[k] = open[k]; block_out[k] = block_open ? block(a.done, k) : 0; }
        i64 complete = c0 + a.cells_done - F;
        complete = complete < 0 ? 0 : (complete > W ? W : complete);
        out[NVX_DIV_ST_FIRST] = F; out[NVX_DIV_ST_COMPLETE] = complete;
        out[NVX_DIV_ST_LEAD] = lead; out[NVX_DIV_ST_WRE] = w_re; out[NVX_DIV_ST_WIM] = w_im;
        out[NVX_DIV_ST_COHERENCE] = coherence; out[NVX_DIV_ST_MODE] = mode; out[NVX_DIV_ST_REASON] = reason;
        u64 *const counters = a.counters + ((size_t)pair * K + t) * 2;
        counters[0] += solved; counters[1] += rejected;
    }
}

// ----------------------------------------------------------------------------------------------------------------- apply
// the weight as the two words the dot products take: (w_re, -w_im) and (w_im, w_re), low half first
struct Weight { uint32_t k_p, k_r; int lead; };
__device__ __forceinline__ Weight weight(const nvx_div_weight &w)
{
    Weight c = { ((uint32_t)w.w_re & 0xffffu) | ((uint32_t)(-w.w_im) << 16), ((uint32_t)w.w_im & 0xffffu) | ((uint32_t)w.w_re << 16), w.lead };
    // uniform, and through vector registers all the same: the unrolled steps' weights would not fit the scalar ones
    asm volatile("" : "+v"(c.k_p), "+v"(c.k_r), "+v"(c.lead));
    return c;
}

__device__ __forceinline__ uint32_t combine(uint32_t wa, uint32_t wb, const Weight &c)
{
    const uint32_t strong = c.lead ? wb : wa, weak = c.lead ? wa : wb;
    const int p = dot2(weak, c.k_p, 4096), r = dot2(weak, c.k_r, 4096);
    const int oi = clamp16(((int)(strong << 16) >> 16) + (p >> 13)), oq = clamp16(((int)strong >> 16) + (r >> 13));
    return ((uint32_t)oi & 0xffffu) | ((uint32_t)oq << 16);
}

template <int FMT>
__global__ __launch_bounds__(NVX_DIV_THREADS) void nvx_div_apply(const nvx_div_args a)
{
    constexpr int SPT = Shape<FMT>::SPT, STEP = Shape<FMT>::STEP, STEPS = Shape<FMT>::STEPS;
    const int tid = threadIdx.x, lane = tid & 63, pair = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const char *const row_a = (const char *)a.in_main + (size_t)pair * a.pitch_main * Fmt<FMT>::BPS;
    const char *const row_b = (const char *)a.in_second + (size_t)pair * a.pitch_second * Fmt<FMT>::BPS;
    const int n_in = a.n_in, K = a.n_targets;
    uint32_t *const out = a.out + (size_t)pair * K * a.pitch_out + a.out_first;                   // target t: a.pitch_out words further each
    const nvx_div_weight *const list = a.weights + (size_t)pair * a.cells * K;
    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
    const int first = wave * NVX_DIV_REGION + lane * SPT;           // this thread's first sample of a tile

    auto walk = [&](int tbase, int jc, int n_a, bool split, auto full) {
        constexpr bool FULL = decltype(full)::value;
        const int base = tbase + first;
        const char *const src_a = row_a + (size_t)base * Fmt<FMT>::BPS;
        const char *const src_b = row_b + (size_t)base * Fmt<FMT>::BPS;
        const nvx_div_weight *const in_front = list + (size_t)jc * K, *const behind = list + (size_t)(jc + (split ? 1 : 0)) * K;
#pragma unroll
        for (int j = 0; j < STEPS; j++) {
            uint32_t wa[SPT], wb[SPT];
            load_step<FMT, FULL, true>(src_a, base, j, n_in, wa);
            load_step<FMT, FULL, true>(src_b, base, j, n_in, wb);
            // a wave's samples of a step are consecutive: they lie in one cell, or a cell's end cuts them
            const int lo = wave * NVX_DIV_REGION + j * STEP;
            const bool cut = lo < n_a && lo + STEP > n_a;
#pragma unroll 1
            for (int t = 0; t < K; t++) {
                uint32_t o[SPT];
                if (cut) {
                    const Weight ca = weight(in_front[t]), cb = weight(behind[t]);
#pragma unroll
                    for (int k = 0; k < SPT; k++) {
                        const uint32_t x = combine(wa[k], wb[k], ca), y = combine(wa[k], wb[k], cb);
                        o[k] = j * STEP + k < n_a - first ? x : y;
                    }
                } else {
                    const Weight c = weight(lo >= n_a ? behind[t] : in_front[t]);
#pragma unroll
                    for (int k = 0; k < SPT; k++) o[k] = combine(wa[k], wb[k], c);
                }
                store_step<FMT, FULL>(out + (size_t)t * a.pitch_out + base, a.out_vec, base, j, n_in, o);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    for (int tile = tile0; tile < tile1; tile++) {
        const int tbase = tile * NVX_DIV_TILE, coff = a.cell_off + tbase;
        const int jc = coff >> 16, in_cell = coff & (NVX_DIV_CELL - 1);
        int n_a = NVX_DIV_CELL - in_cell;                           // the tile's samples in front of the cell's end
        const bool split = n_a < NVX_DIV_TILE && tbase + n_a < n_in;       // it lies inside the tile, and inside the call
        if (!split) n_a = NVX_DIV_TILE;
        if (tbase + NVX_DIV_TILE <= n_in) walk(tbase, jc, n_a, split, std::true_type{}); else walk(tbase, jc, n_a, split, std::false_type{});
    }
}

template <int FMT>
static hipError_t launch_all(const nvx_div_args *a, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((nvx_div_sums<FMT>), grid, dim3(NVX_DIV_THREADS), 0, s, *a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nvx_div_fold, dim3((unsigned)(a->n_pairs * a->n_targets)), dim3(64), 0, s, *a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((nvx_div_apply<FMT>), grid, dim3(NVX_DIV_THREADS), 0, s, *a);
    return hipGetLastError();
}

hipError_t nvx_div_launch(const nvx_div_args *a, int format, int n_pairs, int chunks, hipStream_t s)
{
    const dim3 grid((unsigned)chunks, (unsigned)n_pairs);
    return nvx_for_format(format, [&](auto fmt) { return launch_all<decltype(fmt)::value>(a, grid, s); });
}
