// nvx_real.hip -- the real-input converter's kernel (include/navtex_amd_real.h states the arithmetic; this file arranges it).
//
//   nvx_real<FMT>   grid (chunks, streams), 256 threads.  A workgroup walks consecutive tiles of T = 4096 outputs of one
//   stream, counted from the call's first (rows are 16-byte aligned there).  An output is a pair of samples (e, o), and a pair
//   has the bytes of one IQ sample of the resampler's format of the same component type: the loads and conversions are
//   nvx_rs_device.h's, and a converted pair is one packed word, e in the low half.
//
// Per tile:
//   load     16 pairs per thread: 16-byte non-temporal loads, a wave's instruction reading 1 KB (S16, F32: 4 pairs per lane
//            and step, 4 steps; U8, S8: 8 pairs, 2 steps; F32 takes two loads per step and issues them step by step).  In
//            the tile in which the call ends the group that straddles the end is read pair by pair; behind the end: zeros.
//   stage    e and o go to the LDS as two int16 rows, the tile's 4096 entries behind a halo of 28: 8 or 16 bytes per lane and
//            store, consecutive lanes side by side.  Threads 0 .. 27 fetch the halo: the stream's state row in front of the
//            call's first tile, the input itself in front of every other (a pure FIR: no chunk waits for another).
//                                                                                                          -- barrier 1
//   filter   a thread takes four consecutive outputs i0 .. i0 + 3 (i0 a multiple of 4), four times; consecutive lanes take
//            consecutive groups.  The 31 odd samples they reach over lie in 16 words from an 8-byte aligned entry: eight
//            ds_read_b64 at a lane stride of 8 bytes, which is free of bank conflicts (32 lanes x 8 bytes = the 64 banks).
//            Outputs 1 and 3 start on a word; for outputs 0 and 2 fifteen funnel shifts (v_perm_b32 here) make the words
//            displaced by one sample.  The antisymmetric 28-tap row is fourteen packed immediates, the Q sum fourteen
//            v_dot2_i32_i16 / v_dot2c_i32_i16 per output through the compiler's builtin, exact in int32.  The even samples:
//            three words.
//            s alternates from output to output and i0 is a multiple of 4: the sign of a thread's first output is uniform.
//   store    16 bytes, non-temporal, where the output rows are 16-byte aligned; word by word otherwise, and for the group
//            the call's end cuts.                                                                          -- barrier 2
// The workgroup of a stream's last sample writes the other state row: the last 28 pairs of the stream, from the input, or
// from the state row read where the call is shorter than that.
// Integers only, except F32's conversion.  The step's shape and load, the look-ahead rule and the dispatch on the format are
// the same-rate companions' (nvx_stream_device.h), which brings nvx_rs_device.h along.
#include "nvx_real_plan.h"
#include "nvx_stream_device.h"

static_assert(NVX_REAL_S16 == NVX_RS_CS16 && NVX_REAL_U8 == NVX_RS_CU8 && NVX_REAL_S8 == NVX_RS_CS8 && NVX_REAL_F32 == NVX_RS_CF32, "formats");
static_assert(NVX_REAL_HISTORY == 28 && NVX_REAL_HISTORY <= NVX_REAL_HALO_AT && NVX_REAL_HALO_AT % 8 == 0, "the halo");

// pairs per lane and step, steps per region: a pair is what a sample is to the other companions
template <int FMT> using Shape = StreamShape<FMT, NVX_REAL_REGION>;

// element t of the row over o[m - 27 + t]: A[13] .. A[0], -A[0] .. -A[13]
constexpr int tap_row(int t) { return t < NVX_REAL_NTAPS ? NVX_REAL_TAPS[NVX_REAL_K - t] : -NVX_REAL_TAPS[t - NVX_REAL_NTAPS]; }
constexpr uint32_t tap_pair(int u) { return ((uint32_t)tap_row(2 * u) & 0xffffu) | ((uint32_t)tap_row(2 * u + 1) << 16); }

// the Q sum over fourteen words of odd samples
__device__ __forceinline__ int q_sum(const uint32_t *x)
{
    constexpr uint32_t H[NVX_REAL_NTAPS] = { tap_pair(0), tap_pair(1), tap_pair(2), tap_pair(3), tap_pair(4), tap_pair(5), tap_pair(6),
                                             tap_pair(7), tap_pair(8), tap_pair(9), tap_pair(10), tap_pair(11), tap_pair(12), tap_pair(13) };
    int acc = 1 << (NVX_REAL_S - 1);
#pragma unroll
    for (int u = 0; u < NVX_REAL_NTAPS; u++) acc = dot2(x[u], H[u], acc);
    return acc >> NVX_REAL_S;
}

template <int FMT>
__global__ __launch_bounds__(NVX_REAL_THREADS) void nvx_real(const nvx_real_args a)
{
    constexpr int SPT = Shape<FMT>::SPT, STEPS = Shape<FMT>::STEPS;
    typedef typename std::conditional<SPT == 8, u32x4, u32x2>::type stage_t;
    __shared__ __attribute__((aligned(16))) uint16_t lds_e[NVX_REAL_LDS_ENTRIES], lds_o[NVX_REAL_LDS_ENTRIES];

    const int tid = threadIdx.x, lane = tid & 63, stream = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const char *const row = (const char *)a.in + (size_t)stream * a.pitch_in * (Fmt<FMT>::BPS / 2);
    uint32_t *const out = a.out + (size_t)stream * a.pitch_out + a.out_first;
    const uint32_t *const st = a.state_in + (size_t)stream * NVX_REAL_STATE_WORDS;
    const int n = a.n;
    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
    const int first = wave * NVX_REAL_REGION + lane * SPT;          // this thread's first pair of a tile
    // the signs of a thread's outputs 0 and 2 (1 and 3 have the others): I, and Q with the plan's `invert`
    const int s_i = a.par ? -1 : 1, s_q = a.invert ? -s_i : s_i;

    auto walk = [&](int tbase, auto full) {
        constexpr bool FULL = decltype(full)::value;
        // ---- load, convert and stage
        const int base = tbase + first;
        const char *const src = row + (size_t)base * Fmt<FMT>::BPS;
        uint32_t w[16];
        if constexpr (Ahead<FMT>::value) {
#pragma unroll
            for (int j = 0; j < STEPS; j++) load_step<FMT, FULL, true>(src, base, j, n, &w[j * SPT]);
        }
        if (tid < NVX_REAL_HISTORY) {
            const uint32_t h = tbase == 0 ? st[tid] : load_sample<FMT>(row, tbase - NVX_REAL_HISTORY + tid);
            lds_e[NVX_REAL_HALO_AT - NVX_REAL_HISTORY + tid] = (uint16_t)h;
            lds_o[NVX_REAL_HALO_AT - NVX_REAL_HISTORY + tid] = (uint16_t)(h >> 16);
        }
#pragma unroll
        for (int j = 0; j < STEPS; j++) {
            if constexpr (!Ahead<FMT>::value) load_step<FMT, FULL, true>(src, base, j, n, &w[j * SPT]);
            const int at = NVX_REAL_HALO_AT + first + j * 64 * SPT;
            stage_t e, o;
            const uint32_t *const p = &w[j * SPT];
            if constexpr (SPT == 8) {
                e = stage_t{ lo_pair(p[0], p[1]), lo_pair(p[2], p[3]), lo_pair(p[4], p[5]), lo_pair(p[6], p[7]) };
                o = stage_t{ hi_pair(p[0], p[1]), hi_pair(p[2], p[3]), hi_pair(p[4], p[5]), hi_pair(p[6], p[7]) };
            } else {
                e = stage_t{ lo_pair(p[0], p[1]), lo_pair(p[2], p[3]) };
                o = stage_t{ hi_pair(p[0], p[1]), hi_pair(p[2], p[3]) };
            }
            *(stage_t *)&lds_e[at] = e;
            *(stage_t *)&lds_o[at] = o;
        }
        __syncthreads();

        // ---- filter and store
#pragma unroll
        for (int g = 0; g < NVX_REAL_TILE / (4 * NVX_REAL_THREADS); g++) {
            const int i0 = (g * NVX_REAL_THREADS + tid) * 4;       // of the tile
            // the odd samples of pairs i0 - 28 .. i0 + 3: x[d] holds those of pairs i0 - 28 + 2 d and the next
            uint32_t x[16], y[15];
            const lds_vu2 *const po = (const lds_vu2 *)&lds_o[NVX_REAL_HALO_AT - NVX_REAL_HISTORY + i0];
#pragma unroll
            for (int d = 0; d < 8; d++) { const u32x2 v = po[d]; x[2 * d] = v.x; x[2 * d + 1] = v.y; }
            // the even samples of pairs i0 - 14 .. i0 - 9
            const uint32_t *const pe = (const uint32_t *)&lds_e[NVX_REAL_HALO_AT - NVX_REAL_K - 1 + i0];
            const uint32_t e0 = pe[0], e1 = pe[1], e2 = pe[2];
#pragma unroll
            for (int d = 0; d < 15; d++) y[d] = __builtin_amdgcn_alignbit(x[d + 1], x[d], 16);
            // output r reaches over pairs i0 + r - 27 .. i0 + r
            const int q[4] = { q_sum(&y[0]), q_sum(&x[1]), q_sum(&y[1]), q_sum(&x[2]) };
            const int e[4] = { (int)e0 >> 16, (int)(e1 << 16) >> 16, (int)e1 >> 16, (int)(e2 << 16) >> 16 };
            uint32_t word[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int vi = clamp16(r & 1 ? -s_i * e[r] : s_i * e[r]), vq = clamp16(r & 1 ? -s_q * q[r] : s_q * q[r]);
                word[r] = ((uint32_t)vi & 0xffffu) | ((uint32_t)vq << 16);
            }
            uint32_t *const dst = out + tbase + i0;
            if (a.out_vec && (FULL || tbase + i0 + 4 <= n)) {
                const u32x4 v = { word[0], word[1], word[2], word[3] };
                __builtin_nontemporal_store(v, (u32x4 *)dst);
            } else {
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (FULL || tbase + i0 + r < n) dst[r] = word[r];
            }
        }
        __syncthreads();
    };

    for (int tile = tile0; tile < tile1; tile++) {
        const int tbase = tile * NVX_REAL_TILE;
        if (tbase + NVX_REAL_TILE <= n) walk(tbase, std::true_type{}); else walk(tbase, std::false_type{});
    }

    // the stream's state for the next call: by the workgroup of its last sample, into the row this launch does not read
    if (blockIdx.x == gridDim.x - 1 && tid < NVX_REAL_HISTORY) {
        const int at = n - NVX_REAL_HISTORY + tid;                  // the pair, counted from the call's first
        a.state_out[(size_t)stream * NVX_REAL_STATE_WORDS + tid] = at >= 0 ? load_sample<FMT>(row, at) : st[NVX_REAL_HISTORY + at];
    }
}

template <int FMT>
static hipError_t launch_one(const nvx_real_args *a, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((nvx_real<FMT>), grid, dim3(NVX_REAL_THREADS), 0, s, *a);
    return hipGetLastError();
}

hipError_t nvx_real_launch(const nvx_real_args *a, int format, int n_streams, int chunks, hipStream_t s)
{
    const dim3 grid((unsigned)chunks, (unsigned)n_streams);
    return nvx_for_format(format, [&](auto fmt) { return launch_one<decltype(fmt)::value>(a, grid, s); });
}
