// nvx_align.hip -- the row aligner's two kernels (include/navtex_amd_align.h states the arithmetic; this file arranges it).
//
//   nvx_align_measure<FMT>   the lag-domain correlator, bound by compute: 2 n_lags N dot products per pair.  Grid (n_lags / 64,
//       chunks, pairs), 256 threads.  Output-stationary: a workgroup owns 64 lags, lane l of every wave the lag lag0 + l, and
//       walks tiles of 1024 main samples, of which each wave takes 256.  A tile is staged in the LDS, converted and reduced
//       to 12 bits: the main row as (I, Q) and (Q, -I) per sample (8 KB; -2048 negates safely, -32768 would not), the sense
//       span of 1024 + 63 samples four times over, copy v moved by v samples (17 KB), so that lane 4 u + v reads the four
//       samples behind its lag with one aligned 16-byte read of copy v at word 4 (p + u) -- the copies lie 16 banks apart and
//       the sixteen lanes of a pass touch 64 different banks.  The main row's words are the same for every lane: two 16-byte
//       reads of one address per four samples.  So three LDS reads feed eight v_dot2_i32_i16.  A term is at most 2^23: 128
//       samples are added in 32 bits (2^30) and folded into 64, twice per wave and tile, and at the chunk's end every lane adds
//       its two sums to the table with 64-bit atomics: exact in any order.  The workgroups of the first 64 lags add SAA and
//       SBB up while they stage.
//   nvx_align_apply<FMT>     grid (chunks, pairs), 256 threads, tiles of 4096 outputs in the same-rate companions' layout
//       (nvx_stream_device.h: wave w owns outputs [1024 w, 1024 w + 1024) of the tile, a lane four of them per step).  The main
//       row is the conversion moved: four loads of a sample each (the move is G + Dm samples, never a multiple of four
//       words for long) and one 16-byte non-temporal store.  The sense row's span of a tile, 4096 + 16 converted words from
//       the carried samples and the call's, is staged in the LDS; a lane reads the twenty words behind its four outputs with
//       five aligned 16-byte reads, forms the I pairs and the Q pairs with v_perm_b32, and takes eight v_dot2_i32_i16 per
//       output and component against the phase's eight tap words, which come from the LDS as well.  8192 is the
//       accumulator's start; a shift, v_med3_i32 and a pack finish.  Every workgroup writes its share of the carried samples
//       for the next call into the state row this launch does not read.
// The formats' sizes, load_sample and the CF32 rule are the resampler's (nvx_rs_device.h).  The step's shape and store, the
// wave sums and the dispatch on the format are the same-rate companions' (nvx_stream_device.h).
#include "nvx_align_plan.h"
#include "nvx_stream_device.h"

static_assert(NVX_ALIGN_CS16 == NVX_RS_CS16 && NVX_ALIGN_CU8 == NVX_RS_CU8 && NVX_ALIGN_CS8 == NVX_RS_CS8 && NVX_ALIGN_CF32 == NVX_RS_CF32, "formats");
static_assert(NVX_ALIGN_TAPS == 16 && NVX_ALIGN_REGION == 4 * StreamLane<NVX_RS_CS16>::STEP, "the apply kernel's shape");

// --------------------------------------------------------------------------------------------------------------- measure
#define SENSE_COPY (NVX_ALIGN_M_TILE + 64 + 16)        // words of a copy: 16 banks beyond a multiple of 64

// both halves >> 4, floor
__device__ __forceinline__ uint32_t reduce12(uint32_t w)
{
    return (((uint32_t)((int)(w << 16) >> 20)) & 0xffffu) | ((uint32_t)((int)w >> 20) << 16);
}

template <int FMT>
__global__ __launch_bounds__(NVX_ALIGN_THREADS) void nvx_align_measure(const nvx_align_measure_args a)
{
    __shared__ u32x4 mainw[NVX_ALIGN_M_TILE / 2];               // two samples: (I, Q), (Q, -I), (I, Q), (Q, -I)
    __shared__ __attribute__((aligned(16))) uint32_t sense[4 * SENSE_COPY];
    const int tid = threadIdx.x, lane = tid & 63, pair = blockIdx.z;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const char *const row_a = (const char *)a.in_main + (size_t)pair * a.pitch_main * Fmt<FMT>::BPS;
    const char *const row_b = (const char *)a.in_sense + (size_t)pair * a.pitch_sense * Fmt<FMT>::BPS;
    const int lag0 = a.lag_first + (int)blockIdx.x * NVX_ALIGN_M_LAGS;
    const bool powers = blockIdx.x == 0;
    const int tile0 = (int)blockIdx.y * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
    const int u = lane >> 2, v = lane & 3;
    uint32_t *const main_words = (uint32_t *)mainw;
    i64 acc_re = 0, acc_im = 0;
    u64 saa = 0, sbb = 0;

    for (int tile = tile0; tile < tile1; tile++) {
        const int left = a.window - tile * NVX_ALIGN_M_TILE;    // main samples from the tile's first on: a multiple of 256
        const int have = left < NVX_ALIGN_M_TILE ? left : NVX_ALIGN_M_TILE;
        const int first = a.n0 + tile * NVX_ALIGN_M_TILE;       // the tile's first main sample
        __syncthreads();
        for (int i = tid; i < NVX_ALIGN_M_TILE; i += NVX_ALIGN_THREADS) {
            const uint32_t w = i < have ? reduce12(load_sample<FMT>(row_a, first + i)) : 0u;
            main_words[2 * i] = w;
            main_words[2 * i + 1] = (w >> 16) | ((uint32_t)(-((int)(w << 16) >> 16)) << 16);
            if (powers) saa += (uint32_t)dot2(w, w, 0);
        }
        // sample j of the span goes to word j - c of copy c
        for (int j = tid; j < NVX_ALIGN_M_TILE + 64 + 3; j += NVX_ALIGN_THREADS) {
            const int idx = first + lag0 + j;
            const uint32_t w = idx >= 0 && idx < a.n_in ? reduce12(load_sample<FMT>(row_b, idx)) : 0u;
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (j - c >= 0 && j - c < NVX_ALIGN_M_TILE + 64) sense[c * SENSE_COPY + j - c] = w;
            if (powers && j < have) sbb += (uint32_t)dot2(w, w, 0);
        }
        __syncthreads();
        if (wave * 256 < have) {
            const u32x4 *const mine = (const u32x4 *)&sense[v * SENSE_COPY + 4 * u];
#pragma unroll 1
            for (int fold = 0; fold < 256 / NVX_ALIGN_M_FOLD; fold++) {
                int re = 0, im = 0;
                const int p0 = wave * 64 + fold * (NVX_ALIGN_M_FOLD / 4);
#pragma unroll 8
                for (int g = 0; g < NVX_ALIGN_M_FOLD / 4; g++) {
                    const int p = p0 + g;
                    const u32x4 m0 = mainw[2 * p], m1 = mainw[2 * p + 1], b = mine[p];
                    re = dot2(m0.x, b.x, re); im = dot2(m0.y, b.x, im);
                    re = dot2(m0.z, b.y, re); im = dot2(m0.w, b.y, im);
                    re = dot2(m1.x, b.z, re); im = dot2(m1.y, b.z, im);
                    re = dot2(m1.z, b.w, re); im = dot2(m1.w, b.w, im);
                }
                acc_re += re; acc_im += im;
            }
        }
    }
    u64 *const cell = a.table + ((size_t)pair * a.n_lags + (size_t)blockIdx.x * NVX_ALIGN_M_LAGS + lane) * 2;
    if (acc_re) atomicAdd(&cell[0], (u64)acc_re);
    if (acc_im) atomicAdd(&cell[1], (u64)acc_im);
    if (powers) {
        const i64 ta = wave_sum64((i64)saa), tb = wave_sum64((i64)sbb);
        if (lane == 0) { atomicAdd(&a.power[2 * (size_t)pair], (u64)ta); atomicAdd(&a.power[2 * (size_t)pair + 1], (u64)tb); }
    }
}

// ----------------------------------------------------------------------------------------------------------------- apply
template <int FMT>
__global__ __launch_bounds__(NVX_ALIGN_THREADS) void nvx_align_apply(const nvx_align_args a)
{
    constexpr int G = NVX_ALIGN_GROUP_DELAY, T = NVX_ALIGN_TAPS;
    __shared__ __attribute__((aligned(16))) uint32_t win[NVX_ALIGN_TILE + T];      // word j: sense sample tbase - Ds - T + j
    __shared__ uint32_t tap_words[T / 2];
    const int tid = threadIdx.x, lane = tid & 63, pair = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const char *const row_a = (const char *)a.in_main + (size_t)pair * a.pitch_main * Fmt<FMT>::BPS;
    const char *const row_b = (const char *)a.in_sense + (size_t)pair * a.pitch_sense * Fmt<FMT>::BPS;
    uint32_t *const out_a = a.out_main + (size_t)pair * a.pitch_out_main + a.out_first;
    uint32_t *const out_b = a.out_sense + (size_t)pair * a.pitch_out_sense + a.out_first;
    const int H = a.history, n_in = a.n_in;
    const uint32_t *const hist_a = a.state_in + (size_t)pair * a.state_words, *const hist_b = hist_a + H;
    int dm, ds, f;
    nvx_align_split_delay(__builtin_amdgcn_readfirstlane(a.delays[pair]), &dm, &ds, &f);

    if (tid < T / 2) tap_words[tid] = a.taps[f * (T / 2) + tid];
    __syncthreads();
    uint32_t tw[T / 2];
#pragma unroll
    for (int q = 0; q < T / 2; q++) tw[q] = tap_words[q];

    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
    const int first = wave * NVX_ALIGN_REGION + lane * 4;          // this thread's first output of a tile

    auto walk = [&](int tbase, auto full) {
        constexpr bool FULL = decltype(full)::value;
        __syncthreads();
        for (int j = tid; j < NVX_ALIGN_TILE + T; j += NVX_ALIGN_THREADS) {
            const int s = tbase - ds - T + j;
            uint32_t w = 0;
            if (s < 0) w = hist_b[H + s];                           // s >= -max_delay - T = -H
            else if (s < n_in) w = load_sample<FMT>(row_b, s);
            win[j] = w;
        }
        __syncthreads();
        const int base = tbase + first;
#pragma unroll 1
        for (int j = 0; j < NVX_ALIGN_REGION / 256; j++) {
            const int o = first + j * 256, n = tbase + o;
            if (!FULL && n >= n_in) continue;
            // the main row: sample n + k - G - Dm, from the carried samples in front of the call
            uint32_t wm[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int m = n + k - G - dm;
                wm[k] = 0;
                if (FULL || n + k < n_in) wm[k] = m < 0 ? hist_a[H + m] : load_sample<FMT>(row_a, m);      // H + m >= T - G
            }
            store_step<NVX_RS_CS16, FULL>(out_a + base, a.vec_main, base, j, n_in, wm);
            // the sense row: words o .. o + 19 of the window hold samples n - Ds - 16 .. n - Ds + 3
            uint32_t w[20];
#pragma unroll
            for (int i = 0; i < 5; i++) {
                const u32x4 q = *(const u32x4 *)&win[o + 4 * i];
                w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
            }
            uint32_t pi[19], pq[19];
#pragma unroll
            for (int i = 1; i < 19; i++) { pi[i] = lo_pair(w[i], w[i + 1]); pq[i] = hi_pair(w[i], w[i + 1]); }
            uint32_t ws[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                int si = 8192, sq = 8192;
#pragma unroll
                for (int q = 0; q < T / 2; q++) { si = dot2(pi[k + 1 + 2 * q], tw[q], si); sq = dot2(pq[k + 1 + 2 * q], tw[q], sq); }
                ws[k] = ((uint32_t)clamp16(si >> 14) & 0xffffu) | ((uint32_t)clamp16(sq >> 14) << 16);
            }
            store_step<NVX_RS_CS16, FULL>(out_b + base, a.vec_sense, base, j, n_in, ws);
        }
    };
    for (int tile = tile0; tile < tile1; tile++) {
        const int tbase = tile * NVX_ALIGN_TILE;
        if (tbase + NVX_ALIGN_TILE <= n_in) walk(tbase, std::true_type{}); else walk(tbase, std::false_type{});
    }

    // the carried samples of the next call: sample n_in - H + j in word j, this workgroup's share
    uint32_t *const so = a.state_out + (size_t)pair * a.state_words;
    const int j0 = (int)blockIdx.x * a.history_per_chunk;
    const int j1 = j0 + a.history_per_chunk < H ? j0 + a.history_per_chunk : H;
    for (int j = j0 + tid; j < j1; j += NVX_ALIGN_THREADS) {
        const int s = n_in - H + j;
        so[j] = s < 0 ? hist_a[n_in + j] : load_sample<FMT>(row_a, s);
        so[H + j] = s < 0 ? hist_b[n_in + j] : load_sample<FMT>(row_b, s);
    }
}

template <int FMT>
static hipError_t launch_apply(const nvx_align_args *a, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((nvx_align_apply<FMT>), grid, dim3(NVX_ALIGN_THREADS), 0, s, *a);
    return hipGetLastError();
}

template <int FMT>
static hipError_t launch_measure(const nvx_align_measure_args *a, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((nvx_align_measure<FMT>), grid, dim3(NVX_ALIGN_THREADS), 0, s, *a);
    return hipGetLastError();
}

hipError_t nvx_align_launch(const nvx_align_args *a, int format, int n_pairs, int chunks, hipStream_t s)
{
    const dim3 grid((unsigned)chunks, (unsigned)n_pairs);
    return nvx_for_format(format, [&](auto fmt) { return launch_apply<decltype(fmt)::value>(a, grid, s); });
}

hipError_t nvx_align_measure_launch(const nvx_align_measure_args *a, int format, int n_pairs, int chunks, hipStream_t s)
{
    const dim3 grid((unsigned)a->n_lags / NVX_ALIGN_M_LAGS, (unsigned)chunks, (unsigned)n_pairs);
    return nvx_for_format(format, [&](auto fmt) { return launch_measure<decltype(fmt)::value>(a, grid, s); });
}
