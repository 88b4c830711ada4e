// nvx_anc.hip -- the noise canceller's two kernels (include/navtex_amd_anc.h states the arithmetic; this file arranges it).
//
// Both have the grid (chunks, pairs) and 256 threads, and walk consecutive tiles of 4096 samples of one pair, counted from
// the call's first sample (rows are 16-byte aligned there; the blocks of the contract, counted from the pair's reset, are
// not).  Wave w owns samples [1024 w, 1024 w + 1024) of the tile, a thread 16 of them in each row: 16-byte loads, a wave's
// instruction reading 1 KB.  A tile is shorter than a block, so at most one block ends inside it: the samples in front of
// that end are the tile's A part, the rest its B part.  In the tile in which the call ends the group that straddles the end
// is read sample by sample.  This is the IQ corrector's layout (navtex_amd/iqc/nvx_iqc.hip) with two rows in place of one.
//
//   nvx_anc_sums<FMT>    the four sums of every block the call touches.  Per pair of packed words a (main) and b (sense):
//       v_dot2_i32_i16(a, a) and (b, b) are I^2 + Q^2 (up to 2^31: unsigned bits), v_dot2_i32_i16(a, b) is I1 I2 + Q1 Q2 (it
//       wraps only where all four halves are -32768, to a value nothing else gives), and Q1 I2 - I1 Q2 is two 24-bit
//       multiplies and a subtraction (within -2^31 + 32768 .. 2^31 - 32768: negating a half for a third dot product would
//       not fit int16 at -32768).  Over a tile a thread adds the products' halves in 32 bits, over tiles in 64.  Where the
//       block changes, and behind its last tile, a wave reduces its lanes and adds its four sums to the call's record of
//       (pair, block) with 64-bit atomics: exact in any order.  The host zeroes the records in front.  Plain loads: the lines
//       stay for the second pass.
//   nvx_anc_apply<FMT>   the weight of a block is the carried one, or -- in TRACK mode, once W blocks are complete in front
//       of it -- solved from the W records in front of it: the carried ring's for the blocks in front of the call, the
//       call's own behind.  It depends on nothing else, so every workgroup forms that of the blocks it touches: wave 0 adds
//       the W records up, lane 0 solves (shifts and 64-step divisions: integers only), and the LDS hands the numbers round.
//       The workgroup in which a block starts counts it.  Per sample two v_dot2_i32_i16 of (I2, Q2) against the packed pairs
//       (c_re, -c_im) and (c_im, c_re) with 4096 as the accumulator (|c_im| <= 32767 makes the negation safe), a shift, a
//       subtraction, two v_med3_i32 and a pack; 16-byte non-temporal stores where the output rows are 16-byte aligned.  The
//       workgroup of a pair's last sample writes the other state row: the ring of the last W complete blocks, the open
//       block's sums, the weight of the last sample, the coherence and reason of the last solve.
// The formats' sizes, load_words, load_sample and the CF32 rule are the resampler's (nvx_rs_device.h).  The step's shape, load
// and store, the look-ahead rule, the wave sums, the 64-bit division and the dispatch on the format are the same-rate
// companions' (nvx_stream_device.h).
#include "nvx_anc_plan.h"
#include "nvx_stream_device.h"

static_assert(NVX_ANC_CS16 == NVX_RS_CS16 && NVX_ANC_CU8 == NVX_RS_CU8 && NVX_ANC_CS8 == NVX_RS_CS8 && NVX_ANC_CF32 == NVX_RS_CF32, "formats");

// samples per lane and step, steps per region
template <int FMT> using Shape = StreamShape<FMT, NVX_ANC_REGION>;

// ------------------------------------------------------------------------------------------------------------------ sums
struct Sums { u64 saa, sbb; i64 sre, sim; };
// A thread's sums over its samples of one tile, in 32-bit registers: the products in two halves, so that nothing carries
// (sixteen low halves stay below 2^20, sixteen high halves within 2^20 as well).
struct TileSums { uint32_t aa_lo, aa_hi, bb_lo, bb_hi, re_lo, im_lo; int re_hi, im_hi; };

__device__ __forceinline__ void add_pair(TileSums &s, uint32_t a, uint32_t b)
{
    const int i1 = (int)(a << 16) >> 16, q1 = (int)a >> 16, i2 = (int)(b << 16) >> 16, q2 = (int)b >> 16;
    const uint32_t aa = (uint32_t)dot2(a, a, 0), bb = (uint32_t)dot2(b, b, 0);     // I^2 + Q^2, up to 2^31: unsigned bits
    const int re = dot2(a, b, 0);                                   // I1 I2 + Q1 Q2, in -2 * 32768 * 32767 .. 2^31
    const int im = __mul24(q1, i2) - __mul24(i1, q2);               // Q1 I2 - I1 Q2: fits
    s.aa_lo += aa & 0xffffu; s.aa_hi += aa >> 16;
    s.bb_lo += bb & 0xffffu; s.bb_hi += bb >> 16;
    // the bits of -2^31 are those of 2^31, which four halves of -32768 give and nothing else
    s.re_lo += (uint32_t)re & 0xffffu; s.re_hi += (re >> 16) + (re == (int)0x80000000 ? 65536 : 0);
    s.im_lo += (uint32_t)im & 0xffffu; s.im_hi += im >> 16;
    // one sample after the other: left to itself the compiler forms the sixteen samples' products side by side, in a hundred registers
    asm volatile("" : "+v"(s.aa_lo), "+v"(s.aa_hi), "+v"(s.bb_lo), "+v"(s.bb_hi), "+v"(s.re_lo), "+v"(s.im_lo), "+v"(s.re_hi), "+v"(s.im_hi));
}

__device__ __forceinline__ void fold(Sums &acc, const TileSums &s)
{
    acc.saa += ((u64)s.aa_hi << 16) + s.aa_lo; acc.sbb += ((u64)s.bb_hi << 16) + s.bb_lo;
    acc.sre += (i64)s.re_hi * 65536 + s.re_lo; acc.sim += (i64)s.im_hi * 65536 + s.im_lo;
}

// the wave's sums to the record: SAA, SBB, SRE, SIM
__device__ __forceinline__ void flush(const Sums &s, u64 *rec, int lane)
{
    const i64 v[NVX_ANC_SUMS] = { (i64)s.saa, (i64)s.sbb, s.sre, s.sim };
#pragma unroll
    for (int k = 0; k < NVX_ANC_SUMS; k++) {
        const i64 t = wave_sum64(v[k]);
        if (lane == 0 && t) atomicAdd(&rec[k], (u64)t);
    }
}

template <int FMT>
__global__ __launch_bounds__(NVX_ANC_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void nvx_anc_sums(const nvx_anc_args a)
{
    constexpr int SPT = Shape<FMT>::SPT, STEPS = Shape<FMT>::STEPS;
    const int tid = threadIdx.x, lane = tid & 63, pair = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const char *const row_a = (const char *)a.in_main + (size_t)pair * a.pitch_main * Fmt<FMT>::BPS;
    const char *const row_b = (const char *)a.in_sense + (size_t)pair * a.pitch_sense * Fmt<FMT>::BPS;
    u64 *const records = a.records + (size_t)pair * a.blocks * NVX_ANC_SUMS;
    const int n_in = a.n_in;
    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
    const int first = wave * NVX_ANC_REGION + lane * SPT;           // this thread's first sample of a tile

    // acc belongs to block cur (counted from the call's first), per wave: a wave whose region lies in front of a block's end
    // goes on adding where the wave behind it has flushed
    Sums acc = {};
    int cur = (a.off0 + tile0 * NVX_ANC_TILE) >> 16;
    auto enter = [&](int block) {
        if (block != cur) { flush(acc, records + (size_t)cur * NVX_ANC_SUMS, lane); acc = Sums{}; cur = block; }
    };
    auto walk = [&](int tbase, auto full) {
        constexpr bool FULL = decltype(full)::value;
        const int boff = a.off0 + tbase, r = boff >> 16;
        int n_a = NVX_ANC_BLOCK - (boff & (NVX_ANC_BLOCK - 1));    // the tile's samples in front of the block's end
        if (n_a >= NVX_ANC_TILE || tbase + n_a >= n_in) n_a = NVX_ANC_TILE;      // it ends behind the tile, or behind the call
        const char *const src_a = row_a + (size_t)(tbase + first) * Fmt<FMT>::BPS;
        const char *const src_b = row_b + (size_t)(tbase + first) * Fmt<FMT>::BPS;
        enter(r);
        // the usual case: the wave's region lies in front of the end.  One tile in sixteen, from one wave on: what lies in
        // front of it to s, the rest to s_b, each sample added twice, once as zeros
        const bool cut = (wave + 1) * NVX_ANC_REGION > n_a;
        const int lim = n_a - first;                                // sample (j, k) of this thread lies in front where j * 64 * SPT + k < lim
        // half a tile's loads in flight at once: the other half's thirty-two words would not fit beside the sums
        auto halves = [&](TileSums &s, TileSums &s_b, auto is_cut) {
            constexpr bool CUT = decltype(is_cut)::value;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                constexpr int HALF = STEPS / 2;
                uint32_t wa[8], wb[8];
#pragma unroll
                for (int i = 0; i < HALF; i++) {
                    const int j = h * HALF + i;
                    load_step<FMT, FULL, false>(src_a, tbase + first, j, n_in, &wa[i * SPT]);
                    load_step<FMT, FULL, false>(src_b, tbase + first, j, n_in, &wb[i * SPT]);
                    // float32: the step's eight words are formed before the next step's loads go out
                    if constexpr (!Ahead<FMT>::value)
                        asm volatile("" : "+v"(wa[i * SPT]), "+v"(wa[i * SPT + 1]), "+v"(wa[i * SPT + 2]), "+v"(wa[i * SPT + 3]), "+v"(wb[i * SPT]),
                                     "+v"(wb[i * SPT + 1]), "+v"(wb[i * SPT + 2]), "+v"(wb[i * SPT + 3]) : : "memory");
                }
                if constexpr (!CUT) {
#pragma unroll
                    for (int i = 0; i < 8; i++) add_pair(s, wa[i], wb[i]);
                } else {
#pragma unroll
                    for (int i = 0; i < HALF; i++)
#pragma unroll
                        for (int k = 0; k < SPT; k++) {
                            const bool in_front = (h * HALF + i) * 64 * SPT + k < lim;
                            add_pair(s, in_front ? wa[i * SPT + k] : 0u, in_front ? wb[i * SPT + k] : 0u);
                            add_pair(s_b, in_front ? 0u : wa[i * SPT + k], in_front ? 0u : wb[i * SPT + k]);
                        }
                }
                __builtin_amdgcn_sched_barrier(0);                  // the second half's loads stay behind the first half's sums
            }
        };
        TileSums s = {};
        if (!cut) { halves(s, s, std::false_type{}); fold(acc, s); }
        else {
            TileSums s_b = {};
            halves(s, s_b, std::true_type{});
            fold(acc, s); enter(r + 1); fold(acc, s_b);
        }
    };
    int tile = tile0;
    for (; tile < tile1 && (tile + 1) * NVX_ANC_TILE <= n_in; tile++) walk(tile * NVX_ANC_TILE, std::true_type{});
    if (tile < tile1) walk(tile * NVX_ANC_TILE, std::false_type{});        // the call's last tile, where it is not a whole one
    flush(acc, records + (size_t)cur * NVX_ANC_SUMS, lane);
}

// ----------------------------------------------------------------------------------------------------------------- solve
// steps 1 .. 6 of the contract on the window's sums; returns the reason
__device__ int solve(const i64 (&t)[NVX_ANC_SUMS], int window_log2, int &c_re, int &c_im, int &coherence)
{
    const i64 N = (i64)1 << (16 + window_log2);
    const i64 TAA = t[0], TBB = t[1], TRE = t[2], TIM = t[3];
    c_re = 0; c_im = 0; coherence = 0;
    if (TBB < 16 * N) return 1;
    const i64 m = TAA > TBB ? TAA : TBB;
    const int bits = 64 - __builtin_clzll((u64)m), s = bits > 30 ? bits - 30 : 0;
    const i64 taa = TAA >> s, tbb = TBB >> s, tre = TRE >> s, tim = TIM >> s;
    if (tbb < 1024) return 2;
    const i64 cr = floor_div(tre * 16384 + tbb, 2 * tbb), ci = floor_div(tim * 16384 + tbb, 2 * tbb);
    const i64 den = (taa * tbb) >> 14;
    if (den > 0) {
        const u64 q = udiv64((u64)(tre * tre + tim * tim), (u64)den);
        coherence = q > NVX_ANC_COHERENCE_ONE ? NVX_ANC_COHERENCE_ONE : (int)q;
    }
    if (cr > NVX_ANC_C_MAX || cr < -NVX_ANC_C_MAX || ci > NVX_ANC_C_MAX || ci < -NVX_ANC_C_MAX) return 3;
    c_re = (int)cr; c_im = (int)ci;
    return 0;
}

// ----------------------------------------------------------------------------------------------------------------- apply
// the weight as the two words the dot products take: (c_re, -c_im) and (c_im, c_re), low half first
struct Weight { uint32_t k_p, k_r; };
__device__ __forceinline__ Weight weight(int c_re, int c_im)
{
    return { ((uint32_t)c_re & 0xffffu) | ((uint32_t)(-c_im) << 16), ((uint32_t)c_im & 0xffffu) | ((uint32_t)c_re << 16) };
}

__device__ __forceinline__ uint32_t cancel(uint32_t wa, uint32_t wb, const Weight &c)
{
    const int p = dot2(wb, c.k_p, 4096), r = dot2(wb, c.k_r, 4096);
    const int oi = clamp16(((int)(wa << 16) >> 16) - (p >> 13)), oq = clamp16(((int)wa >> 16) - (r >> 13));
    return ((uint32_t)oi & 0xffffu) | ((uint32_t)oq << 16);
}

template <int FMT>
__global__ __launch_bounds__(NVX_ANC_THREADS) void nvx_anc_apply(const nvx_anc_args a)
{
    constexpr int SPT = Shape<FMT>::SPT, STEPS = Shape<FMT>::STEPS;
    __shared__ int xch[4];
    const int tid = threadIdx.x, lane = tid & 63, pair = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const char *const row_a = (const char *)a.in_main + (size_t)pair * a.pitch_main * Fmt<FMT>::BPS;
    const char *const row_b = (const char *)a.in_sense + (size_t)pair * a.pitch_sense * Fmt<FMT>::BPS;
    uint32_t *const out = a.out + (size_t)pair * a.pitch_out + a.out_first;
    const u64 *const records = a.records + (size_t)pair * a.blocks * NVX_ANC_SUMS;
    const i64 *const st = a.state_in + (size_t)pair * a.state_words;
    const int n_in = a.n_in, W = 1 << a.window_log2;
    const i64 *const partial = st + NVX_ANC_SUMS * W, *const scalars = partial + NVX_ANC_SUMS;
    const int complete_in = (int)scalars[NVX_ANC_ST_COMPLETE], mode = (int)scalars[NVX_ANC_ST_MODE];
    // the carried weight: read where it is wanted, not held
    auto carried = [&]() -> Weight { return weight((int)scalars[NVX_ANC_ST_CRE], (int)scalars[NVX_ANC_ST_CIM]); };
    int reason = (int)scalars[NVX_ANC_ST_REASON], coherence = (int)scalars[NVX_ANC_ST_COHERENCE];

    // sum k of block j, counted from the call's first block: the carried ring's in front of the call, the call's record behind
    auto record = [&](int j, int k) -> i64 {
        if (j < 0) return st[(size_t)((a.slot0 + j) & (W - 1)) * NVX_ANC_SUMS + k];
        const i64 v = (i64)records[(size_t)j * NVX_ANC_SUMS + k];
        return j == 0 ? v + partial[k] : v;
    };
    // the weight of block r; `starts`: its first sample lies in this workgroup's tiles, which then counts the block.
    // Uniform: every thread of the workgroup calls it with the same r.
    auto weight_of = [&](int r, bool starts) -> Weight {
        if (mode != NVX_ANC_TRACK || (r == 0 && a.off0 != 0) || complete_in + r < W) return carried();
        if (wave == 0) {
            i64 t[NVX_ANC_SUMS];
#pragma unroll
            for (int k = 0; k < NVX_ANC_SUMS; k++) {
                // the sums are uniform: through vector registers, or the whole solve is scalar code and its registers are
                // spilled around every tile
                t[k] = in_vector_registers(wave_sum64(lane < W ? record(r - W + lane, k) : 0));
            }
            if (lane == 0) {
                int c_re, c_im, coh;
                const int why = solve(t, a.window_log2, c_re, c_im, coh);
                xch[0] = c_re; xch[1] = c_im; xch[2] = coh; xch[3] = why;
                if (starts) atomicAdd(&a.counters[2 * (size_t)pair + (why ? 1 : 0)], 1ull);
            }
        }
        __syncthreads();
        const Weight c = weight(xch[0], xch[1]);
        coherence = xch[2]; reason = xch[3];
        __syncthreads();
        return c;
    };

    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
    const int first = wave * NVX_ANC_REGION + lane * SPT;           // this thread's first sample of a tile
    Weight ca = {}, cb = {};                                        // of the tile's A part, and of its B part
    int cur = -1;                                                   // the block ca belongs to
    int n_a = 0;

    auto walk = [&](int tbase, auto full) {
        constexpr bool FULL = decltype(full)::value;
        const int base = tbase + first;
        const char *const src_a = row_a + (size_t)base * Fmt<FMT>::BPS;
        const char *const src_b = row_b + (size_t)base * Fmt<FMT>::BPS;
        uint32_t *const dst = out + base;
        uint32_t wa[16], wb[16];
        if constexpr (Ahead<FMT>::value) {
#pragma unroll
            for (int j = 0; j < STEPS; j++) {
                load_step<FMT, FULL, true>(src_a, base, j, n_in, &wa[j * SPT]);
                load_step<FMT, FULL, true>(src_b, base, j, n_in, &wb[j * SPT]);
            }
        }
#pragma unroll
        for (int j = 0; j < STEPS; j++) {
            if constexpr (!Ahead<FMT>::value) {
                load_step<FMT, FULL, true>(src_a, base, j, n_in, &wa[j * SPT]);
                load_step<FMT, FULL, true>(src_b, base, j, n_in, &wb[j * SPT]);
            }
            // a wave's samples of a step are consecutive: they lie in one block, or -- one step of one wave of one tile in
            // sixteen -- a block's end cuts them
            const int lo = wave * NVX_ANC_REGION + j * 64 * SPT;
            if (lo < n_a && lo + 64 * SPT > n_a) {
#pragma unroll
                for (int k = 0; k < SPT; k++) {
                    const uint32_t in_front = cancel(wa[j * SPT + k], wb[j * SPT + k], ca), behind = cancel(wa[j * SPT + k], wb[j * SPT + k], cb);
                    wa[j * SPT + k] = j * 64 * SPT + k < n_a - first ? in_front : behind;
                }
            } else {
                const bool b = lo >= n_a;
                const Weight c = { b ? cb.k_p : ca.k_p, b ? cb.k_r : ca.k_r };
#pragma unroll
                for (int k = 0; k < SPT; k++) wa[j * SPT + k] = cancel(wa[j * SPT + k], wb[j * SPT + k], c);
            }
            store_step<FMT, FULL>(dst, a.out_vec, base, j, n_in, &wa[j * SPT]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    for (int tile = tile0; tile < tile1; tile++) {
        const int tbase = tile * NVX_ANC_TILE, boff = a.off0 + tbase;
        const int r = boff >> 16, in_block = boff & (NVX_ANC_BLOCK - 1);
        if (r != cur) { ca = weight_of(r, in_block == 0); cur = r; }
        n_a = NVX_ANC_BLOCK - in_block;                             // the tile's samples in front of the block's end
        const bool split = n_a < NVX_ANC_TILE && tbase + n_a < n_in;       // it lies inside the tile, and inside the call
        if (split) cb = weight_of(r + 1, true);
        else n_a = NVX_ANC_TILE;
        if (tbase + NVX_ANC_TILE <= n_in) walk(tbase, std::true_type{}); else walk(tbase, std::false_type{});
        if (split) { ca = cb; cur = r + 1; }
    }

    // the pair's state for the next call: by the workgroup of its last sample, into the row this launch does not read
    if (blockIdx.x == gridDim.x - 1) {
        i64 *const so = a.state_out + (size_t)pair * a.state_words;
        const int done = (a.off0 + n_in) >> 16;                     // blocks that ended inside the call
        if (tid < W) {                                              // the last W complete blocks, each to its slot
            const int j = done - 1 - tid;
#pragma unroll
            for (int k = 0; k < NVX_ANC_SUMS; k++) so[(size_t)((a.slot0 + j) & (W - 1)) * NVX_ANC_SUMS + k] = record(j, k);
        }
        if (tid == 64) {
            const bool open = ((a.off0 + n_in) & (NVX_ANC_BLOCK - 1)) != 0;
#pragma unroll
            for (int k = 0; k < NVX_ANC_SUMS; k++) so[NVX_ANC_SUMS * W + k] = open ? record(done, k) : 0;
        }
        if (tid == 65) {
            i64 *const sc = so + NVX_ANC_SUMS * W + NVX_ANC_SUMS;
            sc[NVX_ANC_ST_COMPLETE] = complete_in + done < W ? complete_in + done : W;
            sc[NVX_ANC_ST_CRE] = (int)ca.k_r >> 16; sc[NVX_ANC_ST_CIM] = (int)(ca.k_r << 16) >> 16;
            sc[NVX_ANC_ST_COHERENCE] = coherence; sc[NVX_ANC_ST_MODE] = mode; sc[NVX_ANC_ST_REASON] = reason;
            sc[NVX_ANC_ST_REASON + 1] = 0; sc[NVX_ANC_ST_REASON + 2] = 0;
        }
    }
}

template <int FMT>
static hipError_t launch_both(const nvx_anc_args *a, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((nvx_anc_sums<FMT>), grid, dim3(NVX_ANC_THREADS), 0, s, *a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((nvx_anc_apply<FMT>), grid, dim3(NVX_ANC_THREADS), 0, s, *a);
    return hipGetLastError();
}

hipError_t nvx_anc_launch(const nvx_anc_args *a, int format, int n_pairs, int chunks, hipStream_t s)
{
    const dim3 grid((unsigned)chunks, (unsigned)n_pairs);
    return nvx_for_format(format, [&](auto fmt) { return launch_both<decltype(fmt)::value>(a, grid, s); });
}
