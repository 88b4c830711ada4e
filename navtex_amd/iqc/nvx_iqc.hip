// nvx_iqc.hip -- the IQ corrector's two kernels (include/navtex_amd_iqc.h states the arithmetic; this file arranges it).
//
// Both have the grid (chunks, streams) and 256 threads, and walk consecutive tiles of 4096 samples of one stream, counted
// from the call's first sample (rows are 16-byte aligned there; the blocks of the contract, counted from the stream's reset,
// are not).  Wave w owns samples [1024 w, 1024 w + 1024) of the tile, a thread 16 of them: 16-byte loads, a wave's instruction
// reading 1 KB.  A tile is shorter than a block, so at most one block ends inside it: the samples in front of that end are
// the tile's A part, the rest its B part.  In the tile in which the call ends the group that straddles the end is read
// sample by sample.
//
//   nvx_iqc_sums<FMT>    the five sums of every block the call touches.  Per packed word x: v_dot2_i32_i16(x, x) is
//       I^2 + Q^2 (up to 2^31: unsigned bits), v_dot2_i32_i16(x, x with its halves swapped) is 2 I Q (it wraps only for
//       I = Q = -32768, to a value no other sample gives), I^2 is a 24-bit multiply; the sum of Q^2 is the difference, and
//       the sum of I Q half the sum of 2 I Q.  Over a tile a thread adds the products' halves in 32 bits, over tiles in
//       64.  Where the block changes, and behind its last tile, a wave reduces its lanes and adds its five sums to the
//       call's record of (stream, block) with 64-bit atomics: exact in any order.  The host zeroes the records in front.
//       Plain loads: the lines stay for the second pass.
//   nvx_iqc_apply<FMT>   the coefficients of a block are the carried ones, or -- in TRACK mode, once W blocks are complete
//       in front of it -- solved from the W records in front of it: the carried ring's for the blocks in front of the
//       call, the call's own behind.  They depend on nothing else, so every workgroup forms those of the blocks it touches:
//       wave 0 adds the W records up, lane 0 solves (shifts, a 64-step division, a 32-step square root: integers only),
//       and the LDS hands the five numbers round.  The workgroup in which a block starts counts it.  Per sample two
//       v_mad_i32_i24, a shift, two v_med3_i32 and a pack; 16-byte non-temporal stores where the output rows are 16-byte
//       aligned.  The workgroup of a stream's last sample writes the other state row: the ring of the last W complete
//       blocks, the open block's sums, the coefficients of the last sample.
// The formats' sizes, load_words, load_sample and the CF32 rule are the resampler's (nvx_rs_device.h).  The step's shape, load
// and store, the look-ahead rule, the wave sums, the 64-bit division and the dispatch on the format are the same-rate
// companions' (nvx_stream_device.h).
#include "nvx_iqc_plan.h"
#include "nvx_stream_device.h"

static_assert(NVX_IQC_CS16 == NVX_RS_CS16 && NVX_IQC_CU8 == NVX_RS_CU8 && NVX_IQC_CS8 == NVX_RS_CS8 && NVX_IQC_CF32 == NVX_RS_CF32, "formats");

// samples per lane and step, steps per region
template <int FMT> using Shape = StreamShape<FMT, NVX_IQC_REGION>;

// ------------------------------------------------------------------------------------------------------------------ sums
struct Sums { i64 si, sq, s2iq; u64 sii, spp; };
// A thread's sums over its samples of one tile, in 32-bit registers: the products in two halves, so that nothing carries
// (sixteen low halves stay below 2^20, sixteen high halves below 2^20 as well).
struct TileSums { int si, sq, x_hi; uint32_t ii_lo, ii_hi, pp_lo, pp_hi, x_lo; };

__device__ __forceinline__ void add_word(TileSums &s, uint32_t w)
{
    const int i = (int)(w << 16) >> 16, q = (int)w >> 16;
    const uint32_t ii = (uint32_t)__mul24(i, i);                    // up to 2^30
    const uint32_t pp = (uint32_t)dot2(w, w, 0);                    // I^2 + Q^2, up to 2^31: unsigned bits
    const int twice = dot2(w, __builtin_amdgcn_alignbit(w, w, 16), 0);      // 2 I Q, in -2 * 32768 * 32767 .. 2^31
    s.si += i; s.sq += q;
    s.ii_lo += ii & 0xffffu; s.ii_hi += ii >> 16;
    s.pp_lo += pp & 0xffffu; s.pp_hi += pp >> 16;
    // the bits of -2^31 are those of 2^31, which I = Q = -32768 gives and nothing else
    s.x_lo += (uint32_t)twice & 0xffffu; s.x_hi += (twice >> 16) + (twice == (int)0x80000000 ? 65536 : 0);
    // one sample after the other: left to itself the compiler forms the sixteen samples' products side by side, in a hundred registers
    asm volatile("" : "+v"(s.si), "+v"(s.sq), "+v"(s.x_hi), "+v"(s.ii_lo), "+v"(s.ii_hi), "+v"(s.pp_lo), "+v"(s.pp_hi), "+v"(s.x_lo));
}

__device__ __forceinline__ void fold(Sums &acc, const TileSums &s)
{
    acc.si += s.si; acc.sq += s.sq;
    acc.sii += ((u64)s.ii_hi << 16) + s.ii_lo; acc.spp += ((u64)s.pp_hi << 16) + s.pp_lo;
    acc.s2iq += (i64)s.x_hi * 65536 + s.x_lo;
}

// the wave's sums to the record: SI, SQ, SII, SQQ, SIQ
__device__ __forceinline__ void flush(const Sums &s, u64 *rec, int lane)
{
    const i64 v[NVX_IQC_SUMS] = { s.si, s.sq, (i64)s.sii, (i64)(s.spp - s.sii), s.s2iq >> 1 };      // a thread's 2 I Q sum is even
#pragma unroll
    for (int k = 0; k < NVX_IQC_SUMS; k++) {
        const i64 t = wave_sum64(v[k]);
        if (lane == 0 && t) atomicAdd(&rec[k], (u64)t);
    }
}

template <int FMT>
__global__ __launch_bounds__(NVX_IQC_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void nvx_iqc_sums(const nvx_iqc_args a)
{
    constexpr int SPT = Shape<FMT>::SPT, STEPS = Shape<FMT>::STEPS;
    const int tid = threadIdx.x, lane = tid & 63, stream = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const char *const row = (const char *)a.in + (size_t)stream * a.pitch_in * Fmt<FMT>::BPS;
    u64 *const records = a.records + (size_t)stream * a.blocks * NVX_IQC_SUMS;
    const int n_in = a.n_in;
    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
    const int first = wave * NVX_IQC_REGION + lane * SPT;           // this thread's first sample of a tile

    // acc belongs to block cur (counted from the call's first), per wave: a wave whose region lies in front of a block's end
    // goes on adding where the wave behind it has flushed
    Sums acc = {};
    int cur = (a.off0 + tile0 * NVX_IQC_TILE) >> 16;
    auto enter = [&](int block) {
        if (block != cur) { flush(acc, records + (size_t)cur * NVX_IQC_SUMS, lane); acc = Sums{}; cur = block; }
    };
    auto walk = [&](int tbase, auto full) {
        constexpr bool FULL = decltype(full)::value;
        const int boff = a.off0 + tbase, r = boff >> 16;
        int n_a = NVX_IQC_BLOCK - (boff & (NVX_IQC_BLOCK - 1));    // the tile's samples in front of the block's end
        if (n_a >= NVX_IQC_TILE || tbase + n_a >= n_in) n_a = NVX_IQC_TILE;      // it ends behind the tile, or behind the call
        const char *const src = row + (size_t)(tbase + first) * Fmt<FMT>::BPS;
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < STEPS; j++) {
            load_step<FMT, FULL, false>(src, tbase + first, j, n_in, &w[j * SPT]);
            // float32: the step's four words are formed before the next step's loads go out
            if constexpr (!Ahead<FMT>::value) asm volatile("" : "+v"(w[j * SPT]), "+v"(w[j * SPT + 1]), "+v"(w[j * SPT + 2]), "+v"(w[j * SPT + 3]) : : "memory");
        }
        enter(r);
        TileSums s = {};
        if ((wave + 1) * NVX_IQC_REGION <= n_a) {                   // the wave's region lies in front of the end: the usual case
#pragma unroll
            for (int j = 0; j < 16; j++) add_word(s, w[j]);
        } else {                                                    // one tile in sixteen: what lies in front of it, then the rest
            const int lim = n_a - first;                            // sample (j, k) of this thread lies in front where j * 64 * SPT + k < lim
#pragma unroll
            for (int j = 0; j < STEPS; j++)
#pragma unroll
                for (int k = 0; k < SPT; k++) add_word(s, j * 64 * SPT + k < lim ? w[j * SPT + k] : 0u);
            fold(acc, s);
            enter(r + 1);
            s = TileSums{};
#pragma unroll
            for (int j = 0; j < STEPS; j++)
#pragma unroll
                for (int k = 0; k < SPT; k++) add_word(s, j * 64 * SPT + k < lim ? 0u : w[j * SPT + k]);
        }
        fold(acc, s);
    };
    int tile = tile0;
    for (; tile < tile1 && (tile + 1) * NVX_IQC_TILE <= n_in; tile++) walk(tile * NVX_IQC_TILE, std::true_type{});
    if (tile < tile1) walk(tile * NVX_IQC_TILE, std::false_type{});        // the call's last tile, where it is not a whole one
    flush(acc, records + (size_t)cur * NVX_IQC_SUMS, lane);
}

// ----------------------------------------------------------------------------------------------------------------- solve
__device__ __forceinline__ u64 isqrt64(u64 x)
{
    u64 r = 0, bit = (u64)1 << 62;
#pragma unroll 1
    for (; bit; bit >>= 2) {
        if (x >= r + bit) { x -= r + bit; r = (r >> 1) + bit; }
        else r >>= 1;
    }
    return r;
}

// steps 1 .. 10 of the contract on the window's sums; returns the reason
__device__ int solve(const i64 (&t)[NVX_IQC_SUMS], int window_log2, int &d_i, int &d_q, int &c_i, int &c_q)
{
    const int ln = 16 + window_log2;
    const i64 N = (i64)1 << ln;
    const i64 TI = t[0], TQ = t[1], TII = t[2], TQQ = t[3], TIQ = t[4];
    const i64 dI = (TI + N / 2) >> ln, dQ = (TQ + N / 2) >> ln;
    const i64 CII = TII - 2 * dI * TI + N * dI * dI, CQQ = TQQ - 2 * dQ * TQ + N * dQ * dQ, CIQ = TIQ - dI * TQ - dQ * TI + N * dI * dQ;
    d_i = (int)dI; d_q = (int)dQ; c_i = 0; c_q = NVX_IQC_CQ_IDENTITY;
    if (CII < 16 * N || CQQ < 16 * N) return 1;
    const i64 m = CII > CQQ ? CII : CQQ;
    const int bits = 64 - __builtin_clzll((u64)m), s = bits > 30 ? bits - 30 : 0;
    const i64 cii = CII >> s, cqq = CQQ >> s, ciq = CIQ >> s;
    const i64 al = floor_div(-ciq * 32768 + cii, 2 * cii);
    if (al > 4096 || al < -4096) return 2;
    const i64 v = cqq + ((2 * al * ciq) >> 14) + ((al * al * cii) >> 28);
    if (v <= 0) return 3;
    const i64 g = (i64)isqrt64(udiv64((u64)cii << 28, (u64)v));
    if (g < NVX_IQC_CQ_MIN || g > NVX_IQC_CQ_MAX) return 4;
    c_q = (int)g; c_i = (int)((al * g + 8192) >> 14);
    return 0;
}

// ----------------------------------------------------------------------------------------------------------------- apply
struct Coef { int d_i, d_q, c_i, c_q; };

// a * b + c of 24-bit a and b: written out, or the compiler makes a multiply and a three-operand add of the two
__device__ __forceinline__ int mad24(int a, int b, int c)
{
    int d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

__device__ __forceinline__ uint32_t correct(uint32_t w, const Coef &c)
{
    const int i = ((int)(w << 16) >> 16) - c.d_i, q = ((int)w >> 16) - c.d_q;
    const int oq = clamp16(mad24(c.c_i, i, mad24(c.c_q, q, 8192)) >> 14);
    return ((uint32_t)clamp16(i) & 0xffffu) | ((uint32_t)oq << 16);
}

template <int FMT>
__global__ __launch_bounds__(NVX_IQC_THREADS) void nvx_iqc_apply(const nvx_iqc_args a)
{
    constexpr int SPT = Shape<FMT>::SPT, STEPS = Shape<FMT>::STEPS;
    __shared__ int xch[5];
    const int tid = threadIdx.x, lane = tid & 63, stream = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const char *const row = (const char *)a.in + (size_t)stream * a.pitch_in * Fmt<FMT>::BPS;
    uint32_t *const out = a.out + (size_t)stream * a.pitch_out + a.out_first;
    const u64 *const records = a.records + (size_t)stream * a.blocks * NVX_IQC_SUMS;
    const i64 *const st = a.state_in + (size_t)stream * a.state_words;
    const int n_in = a.n_in, W = 1 << a.window_log2;
    const i64 *const partial = st + NVX_IQC_SUMS * W, *const scalars = partial + NVX_IQC_SUMS;
    const int complete_in = (int)scalars[NVX_IQC_ST_COMPLETE], mode = (int)scalars[NVX_IQC_ST_MODE];
    // the carried coefficients: read where they are wanted, not held
    auto carried = [&]() -> Coef { return { (int)scalars[NVX_IQC_ST_DI], (int)scalars[NVX_IQC_ST_DQ], (int)scalars[NVX_IQC_ST_CI], (int)scalars[NVX_IQC_ST_CQ] }; };
    int reason = (int)scalars[NVX_IQC_ST_REASON];

    // sum k of block j, counted from the call's first block: the carried ring's in front of the call, the call's record behind
    auto record = [&](int j, int k) -> i64 {
        if (j < 0) return st[(size_t)((a.slot0 + j) & (W - 1)) * NVX_IQC_SUMS + k];
        const i64 v = (i64)records[(size_t)j * NVX_IQC_SUMS + k];
        return j == 0 ? v + partial[k] : v;
    };
    // the coefficients of block r; `starts`: its first sample lies in this workgroup's tiles, which then counts the block.
    // Uniform: every thread of the workgroup calls it with the same r.
    auto coefficients = [&](int r, bool starts) -> Coef {
        if (mode != NVX_IQC_TRACK || (r == 0 && a.off0 != 0) || complete_in + r < W) return carried();
        if (wave == 0) {
            i64 t[NVX_IQC_SUMS];
#pragma unroll
            for (int k = 0; k < NVX_IQC_SUMS; k++) {
                // the sums are uniform: through vector registers, or the whole solve is scalar code and its sixty-odd registers
                // are spilled around every tile
                t[k] = in_vector_registers(wave_sum64(lane < W ? record(r - W + lane, k) : 0));
            }
            if (lane == 0) {
                int d_i, d_q, c_i, c_q;
                const int why = solve(t, a.window_log2, d_i, d_q, c_i, c_q);
                xch[0] = d_i; xch[1] = d_q; xch[2] = c_i; xch[3] = c_q; xch[4] = why;
                if (starts) atomicAdd(&a.counters[2 * (size_t)stream + (why ? 1 : 0)], 1ull);
            }
        }
        __syncthreads();
        const Coef c = { xch[0], xch[1], xch[2], xch[3] };
        reason = xch[4];
        __syncthreads();
        return c;
    };

    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
    const int first = wave * NVX_IQC_REGION + lane * SPT;           // this thread's first sample of a tile
    Coef ca = {}, cb = {};                                          // of the tile's A part, and of its B part
    int cur = -1;                                                   // the block ca belongs to
    int n_a = 0;

    auto walk = [&](int tbase, auto full) {
        constexpr bool FULL = decltype(full)::value;
        const int base = tbase + first;
        const char *const src = row + (size_t)base * Fmt<FMT>::BPS;
        uint32_t *const dst = out + base;
        uint32_t w[16];
        if constexpr (Ahead<FMT>::value) {
#pragma unroll
            for (int j = 0; j < STEPS; j++) load_step<FMT, FULL, true>(src, base, j, n_in, &w[j * SPT]);
        }
#pragma unroll
        for (int j = 0; j < STEPS; j++) {
            if constexpr (!Ahead<FMT>::value) load_step<FMT, FULL, true>(src, base, j, n_in, &w[j * SPT]);
            // a wave's samples of a step are consecutive: they lie in one block, or -- one step of one wave of one tile in
            // sixteen -- a block's end cuts them
            const int lo = wave * NVX_IQC_REGION + j * 64 * SPT;
            if (lo < n_a && lo + 64 * SPT > n_a) {
#pragma unroll
                for (int k = 0; k < SPT; k++) {
                    const uint32_t in_front = correct(w[j * SPT + k], ca), behind = correct(w[j * SPT + k], cb);
                    w[j * SPT + k] = j * 64 * SPT + k < n_a - first ? in_front : behind;
                }
            } else {
                const bool b = lo >= n_a;
                const Coef c = { b ? cb.d_i : ca.d_i, b ? cb.d_q : ca.d_q, b ? cb.c_i : ca.c_i, b ? cb.c_q : ca.c_q };
#pragma unroll
                for (int k = 0; k < SPT; k++) w[j * SPT + k] = correct(w[j * SPT + k], c);
            }
            store_step<FMT, FULL>(dst, a.out_vec, base, j, n_in, &w[j * SPT]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    for (int tile = tile0; tile < tile1; tile++) {
        const int tbase = tile * NVX_IQC_TILE, boff = a.off0 + tbase;
        const int r = boff >> 16, in_block = boff & (NVX_IQC_BLOCK - 1);
        if (r != cur) { ca = coefficients(r, in_block == 0); cur = r; }
        n_a = NVX_IQC_BLOCK - in_block;                             // the tile's samples in front of the block's end
        const bool split = n_a < NVX_IQC_TILE && tbase + n_a < n_in;       // it lies inside the tile, and inside the call
        if (split) cb = coefficients(r + 1, true);
        else n_a = NVX_IQC_TILE;
        if (tbase + NVX_IQC_TILE <= n_in) walk(tbase, std::true_type{}); else walk(tbase, std::false_type{});
        if (split) { ca = cb; cur = r + 1; }
    }

    // the stream's state for the next call: by the workgroup of its last sample, into the row this launch does not read
    if (blockIdx.x == gridDim.x - 1) {
        i64 *const so = a.state_out + (size_t)stream * a.state_words;
        const int done = (a.off0 + n_in) >> 16;                     // blocks that ended inside the call
        if (tid < W) {                                              // the last W complete blocks, each to its slot
            const int j = done - 1 - tid;
#pragma unroll
            for (int k = 0; k < NVX_IQC_SUMS; k++) so[(size_t)((a.slot0 + j) & (W - 1)) * NVX_IQC_SUMS + k] = record(j, k);
        }
        if (tid == 64) {
            const bool open = ((a.off0 + n_in) & (NVX_IQC_BLOCK - 1)) != 0;
#pragma unroll
            for (int k = 0; k < NVX_IQC_SUMS; k++) so[NVX_IQC_SUMS * W + k] = open ? record(done, k) : 0;
        }
        if (tid == 65) {
            i64 *const sc = so + NVX_IQC_SUMS * W + NVX_IQC_SUMS;
            sc[NVX_IQC_ST_COMPLETE] = complete_in + done < W ? complete_in + done : W;
            sc[NVX_IQC_ST_DI] = ca.d_i; sc[NVX_IQC_ST_DQ] = ca.d_q; sc[NVX_IQC_ST_CI] = ca.c_i; sc[NVX_IQC_ST_CQ] = ca.c_q;
            sc[NVX_IQC_ST_MODE] = mode; sc[NVX_IQC_ST_REASON] = reason; sc[NVX_IQC_ST_REASON + 1] = 0;
        }
    }
}

template <int FMT>
static hipError_t launch_both(const nvx_iqc_args *a, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((nvx_iqc_sums<FMT>), grid, dim3(NVX_IQC_THREADS), 0, s, *a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((nvx_iqc_apply<FMT>), grid, dim3(NVX_IQC_THREADS), 0, s, *a);
    return hipGetLastError();
}

hipError_t nvx_iqc_launch(const nvx_iqc_args *a, int format, int n_streams, int chunks, hipStream_t s)
{
    const dim3 grid((unsigned)chunks, (unsigned)n_streams);
    return nvx_for_format(format, [&](auto fmt) { return launch_both<decltype(fmt)::value>(a, grid, s); });
}
