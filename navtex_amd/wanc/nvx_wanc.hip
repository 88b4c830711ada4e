// nvx_wanc.hip -- the multi-tap canceller's three kernels (include/navtex_amd_wanc.h states the arithmetic; this file arranges
// it).  Every kernel is an instance per tap count K = 4, 8, 16, the first and the last per format as well.
//
// nvx_wanc_sums and nvx_wanc_apply have the grid (chunks, pairs) and 256 threads, and walk consecutive tiles of 4096 samples of
// one pair, counted from the call's first sample (rows are 16-byte aligned there; the blocks of the contract, counted from
// the pair's reset, are not): the noise canceller's tiles (navtex_amd/anc/nvx_anc.hip).  A tile of both rows is loaded 16
// bytes at a time as there (wave w loads samples [1024 w, 1024 w + 1024)), converted, and staged in the LDS as packed words:
// the sense row behind a halo of 16 words, of which the last K - 1 are the samples in front of the tile, and the main row moved
// by G = K / 2 words, so that word j is a[tile + j - G].  The halo comes from the carried words at a call's start and from the
// row inside it.  A lane then takes four consecutive samples a step: one aligned 16-byte LDS read of the main words and
// K / 4 + 1 (K = 4: 2) of the sense words behind them.  A tile is shorter than a block, so at most one block ends inside it;
// such a tile (one in sixteen) is walked twice, once for the samples in front of the end and once for those behind it.
//
//   nvx_wanc_sums<FMT, K>   the 4 K + 1 sums of every block the call touches.  Per sample, against each of the K sense words
//       b[n - k]: v_dot2_i32_i16 for the real part of b[n] conj(b[n - k]) and of a[n - G] conj(b[n - k]) (it wraps only where
//       all four halves are -32768, to the bits of 2^31 that nothing else gives), two 24-bit multiplies and a subtraction for
//       each imaginary part (within +-(2^31 - 32768)).  A lane adds its terms in 64 bits.  Where the block changes, and behind
//       its last tile, a wave reduces its lanes and adds its sums to the call's record of (pair, block) with 64-bit atomics:
//       exact in any order.  The host zeroes the records in front.  Plain loads: the lines stay for the second pass.
//   nvx_wanc_solve<K>       one lane per (pair, block the call touches), sixteen lanes a workgroup.  A block whose start lies in
//       the call, in TRACK mode, with W blocks complete in front of it is solved: the lane adds up the W records in front of it
//       (the carried ring's for the blocks in front of the call, the call's own behind), runs the fp64 steps of
//       nvx_wanc_solve.h in its column of the LDS and counts the block; any other block gets the carried weights.  The
//       weights, the coherence and the reason go to the block's weight record.  No fused multiply-add, and so no fp64 division
//       instruction sequence either: nvx_wanc_solve.h has the quotients.
//   nvx_wanc_apply<FMT, K>  the block's weights are read from its weight record as the two words per
//       tap the dot products take, (w_re, -w_im) and (w_im, w_re) (|w_im| <= 32767 makes the negation safe), the same in every lane.  Per sample and
//       tap two v_dot2_i32_i16 of the packed sense word, with 4096 as the accumulators' start; a shift, a subtraction, two
//       v_med3_i32 and a pack; 16-byte non-temporal stores where the output rows are 16-byte aligned.  The workgroup of a
//       pair's last sample writes the other state row: the ring of the last W complete blocks, the open block's sums, the
//       last block's weights, coherence and reason, the last K - 1 sense words and the last G main words.
// The formats' sizes, load_words, load_sample and the CF32 rule are the resampler's (nvx_rs_device.h).  The step's shape and
// load, the wave sums and the dispatch on the format are the same-rate companions' (nvx_stream_device.h).
#include "nvx_wanc_plan.h"
#include "nvx_wanc_solve.h"
#include "nvx_stream_device.h"

static_assert(NVX_WANC_CS16 == NVX_RS_CS16 && NVX_WANC_CU8 == NVX_RS_CU8 && NVX_WANC_CS8 == NVX_RS_CS8 && NVX_WANC_CF32 == NVX_RS_CF32, "formats");
static_assert(NVX_WANC_PAD >= NVX_WANC_TAPS_MAX - 1 && NVX_WANC_PAD % 4 == 0 && NVX_WANC_PAD + NVX_WANC_TAPS_MAX / 2 <= NVX_WANC_THREADS, "the halo");

template <int FMT> using Shape = StreamShape<FMT, NVX_WANC_REGION>;

// where a pair's state row keeps what (nvx_wanc_plan.h)
struct StateAt {
    int ns, W, scalars, weights, sense, main;
    __device__ StateAt(int K, int window_log2) : ns(NVX_WANC_SUMS(K)), W(1 << window_log2), scalars(ns * (W + 1)), weights(scalars + NVX_WANC_STATE_SCALARS),
                                                 sense(weights + 2 * K), main(sense + K - 1) {}
};

// ---------------------------------------------------------------------------------------------------------------- staging
// the tile from sample tbase on: sense[NVX_WANC_PAD + j] = b[tbase + j], mainw[j] = a[tbase + j - G]; samples behind the call's
// end are zero, samples in front of the call are the carried ones
template <int FMT, int K, bool FULL, bool NONTEMPORAL>
__device__ __forceinline__ void stage(uint32_t *sense, uint32_t *mainw, const char *row_a, const char *row_b, const i64 *hist_b, const i64 *hist_a, int tbase,
                                      int n_in, int tid, int first)
{
    constexpr int SPT = Shape<FMT>::SPT, STEPS = Shape<FMT>::STEPS, G = K / 2;
    const int base = tbase + first;
    const char *const src_a = row_a + (size_t)base * Fmt<FMT>::BPS;
    const char *const src_b = row_b + (size_t)base * Fmt<FMT>::BPS;
#pragma unroll
    for (int j = 0; j < STEPS; j++) {
        uint32_t wa[SPT], wb[SPT];
        load_step<FMT, FULL, NONTEMPORAL>(src_a, base, j, n_in, wa);
        load_step<FMT, FULL, NONTEMPORAL>(src_b, base, j, n_in, wb);
        const int o = first + j * 64 * SPT;
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            sense[NVX_WANC_PAD + o + k] = wb[k];
            if (o + k + G < NVX_WANC_TILE) mainw[o + k + G] = wa[k];
        }
    }
    if (tid < NVX_WANC_PAD) {
        const int s = tbase - NVX_WANC_PAD + tid;          // s < tbase <= n_in
        uint32_t v = 0;
        if (s >= 0) v = load_sample<FMT>(row_b, s);
        else if (s >= -(K - 1)) v = (uint32_t)hist_b[K - 1 + s];
        sense[tid] = v;
    } else if (tid < NVX_WANC_PAD + G) {
        const int i = tid - NVX_WANC_PAD, s = tbase - G + i;
        mainw[i] = s >= 0 ? load_sample<FMT>(row_a, s) : (uint32_t)hist_a[G + s];
    }
}

// the words a lane's four samples from sample o of the tile need: w[KP + s - k] = b[o + s - k], ma[s] = a[o + s - G]
template <int K> struct Reach { static constexpr int KP = (K - 1 + 3) / 4 * 4, WORDS = KP + 4; };

template <int K>
__device__ __forceinline__ void read_group(const uint32_t *sense, const uint32_t *mainw, int o, uint32_t (&w)[Reach<K>::WORDS], uint32_t (&ma)[4])
{
    const u32x4 *const p = (const u32x4 *)&sense[NVX_WANC_PAD + o - Reach<K>::KP];
#pragma unroll
    for (int i = 0; i < Reach<K>::WORDS / 4; i++) {
        const u32x4 q = p[i];
        w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
    }
    const u32x4 m = *(const u32x4 *)&mainw[o];
    ma[0] = m.x; ma[1] = m.y; ma[2] = m.z; ma[3] = m.w;
}

// ------------------------------------------------------------------------------------------------------------------ sums
__device__ __forceinline__ int lo16s(uint32_t w) { return (int)(w << 16) >> 16; }
__device__ __forceinline__ int hi16s(uint32_t w) { return (int)w >> 16; }

// x conj(y) added to (re, im)
__device__ __forceinline__ void add_conj(i64 &re, i64 &im, uint32_t x, int ix, int qx, uint32_t y, int iy, int qy)
{
    const int r = dot2(x, y, 0);                                    // Ix Iy + Qx Qy, in -2 * 32768 * 32767 .. 2^31
    re += r == (int)0x80000000 ? (i64)2147483648ll : (i64)r;        // the bits of -2^31 are those of 2^31, which four halves of -32768 give and nothing else
    im += (i64)(__mul24(qx, iy) - __mul24(ix, qy));                 // Qx Iy - Ix Qy: fits
}

template <int K>
__device__ __forceinline__ void flush(i64 (&acc)[NVX_WANC_SUMS(K)], u64 *rec, int lane)
{
#pragma unroll
    for (int k = 0; k < NVX_WANC_SUMS(K); k++) {
        const i64 t = wave_sum64(acc[k]);
        if (lane == 0 && t) atomicAdd(&rec[k], (u64)t);
        acc[k] = 0;
    }
}

template <int FMT, int K>
__global__ __launch_bounds__(NVX_WANC_THREADS) void nvx_wanc_sums(const nvx_wanc_args a)
{
    constexpr int NS = NVX_WANC_SUMS(K), KP = Reach<K>::KP;
    __shared__ __attribute__((aligned(16))) uint32_t sense[NVX_WANC_PAD + NVX_WANC_TILE];
    __shared__ __attribute__((aligned(16))) uint32_t mainw[NVX_WANC_TILE];
    const int tid = threadIdx.x, lane = tid & 63, pair = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const char *const row_a = (const char *)a.in_main + (size_t)pair * a.pitch_main * Fmt<FMT>::BPS;
    const char *const row_b = (const char *)a.in_sense + (size_t)pair * a.pitch_sense * Fmt<FMT>::BPS;
    u64 *const records = a.records + (size_t)pair * a.blocks * NS;
    const StateAt at(K, a.window_log2);
    const i64 *const st = a.state_in + (size_t)pair * a.state_words;
    const int n_in = a.n_in;
    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
    const int first = wave * NVX_WANC_REGION + lane * Shape<FMT>::SPT;     // the first sample of a tile this thread loads
    const int mine = wave * NVX_WANC_REGION + lane * 4;                     // ... and the first it adds up

    i64 acc[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) acc[k] = 0;
    int cur = (a.off0 + tile0 * NVX_WANC_TILE) >> 16;                       // the block acc belongs to, counted from the call's first

    // the tile's samples [lo, hi)
    auto pass = [&](int lo, int hi) {
#pragma unroll 1
        for (int j = 0; j < NVX_WANC_REGION / 256; j++) {
            const int o = mine + j * 256;
            if (o + 4 <= lo || o >= hi) continue;
            uint32_t w[Reach<K>::WORDS], ma[4];
            read_group<K>(sense, mainw, o, w, ma);
            int wi[Reach<K>::WORDS], wq[Reach<K>::WORDS];
#pragma unroll
            for (int i = 0; i < Reach<K>::WORDS; i++) { wi[i] = lo16s(w[i]); wq[i] = hi16s(w[i]); }
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const bool valid = o + s >= lo && o + s < hi;
                const uint32_t b = valid ? w[KP + s] : 0u, m = valid ? ma[s] : 0u;
                const int bi = lo16s(b), bq = hi16s(b), mi = lo16s(m), mq = hi16s(m);
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const int h = KP + s - k;
                    add_conj(acc[k], acc[K + k], b, bi, bq, w[h], wi[h], wq[h]);
                    add_conj(acc[2 * K + k], acc[3 * K + k], m, mi, mq, w[h], wi[h], wq[h]);
                }
                acc[4 * K] += (i64)(u64)(uint32_t)dot2(m, m, 0);    // I^2 + Q^2, up to 2^31: unsigned bits
            }
        }
    };

    for (int tile = tile0; tile < tile1; tile++) {
        const int tbase = tile * NVX_WANC_TILE, boff = a.off0 + tbase;
        const int r = boff >> 16, n_a = NVX_WANC_BLOCK - (boff & (NVX_WANC_BLOCK - 1));     // the tile's samples in front of the block's end
        const int hi = n_in - tbase < NVX_WANC_TILE ? n_in - tbase : NVX_WANC_TILE;
        const bool split = n_a < hi;                                // the end lies inside the tile, and inside the call
        __syncthreads();
        if (tbase + NVX_WANC_TILE <= n_in) stage<FMT, K, true, false>(sense, mainw, row_a, row_b, st + at.sense, st + at.main, tbase, n_in, tid, first);
        else stage<FMT, K, false, false>(sense, mainw, row_a, row_b, st + at.sense, st + at.main, tbase, n_in, tid, first);
        __syncthreads();
        // one walk, or two where the block ends inside: [0, n_a) for block r, [n_a, hi) for the next
#pragma unroll 1
        for (int part = 0; part <= (int)split; part++) {
            if (r + part != cur) { flush<K>(acc, records + (size_t)cur * NS, lane); cur = r + part; }
            pass(part ? n_a : 0, split && !part ? n_a : hi);
        }
    }
    flush<K>(acc, records + (size_t)cur * NS, lane);
}

// ----------------------------------------------------------------------------------------------------------------- solve
// sum k of block j of the pair, counted from the call's first block: the carried ring's in front of the call, the call's
// record behind
struct Blocks {
    const i64 *st; const u64 *records; int ns, W, slot0;
    __device__ i64 operator()(int j, int k) const
    {
        if (j < 0) return st[(size_t)((slot0 + j) & (W - 1)) * ns + k];
        const i64 v = (i64)records[(size_t)j * ns + k];
        return j == 0 ? v + st[(size_t)W * ns + k] : v;            // the open block's partial sums
    }
};

template <int K>
__global__ __launch_bounds__(NVX_WANC_SOLVE_LANES) void nvx_wanc_solve_blocks(const nvx_wanc_args a)
{
    constexpr int NS = NVX_WANC_SUMS(K), WREC = NVX_WANC_WREC(K);
    __shared__ double ws[NVX_WANC_WS_DOUBLES(K) * NVX_WANC_SOLVE_LANES];
    const int idx = (int)blockIdx.x * NVX_WANC_SOLVE_LANES + (int)threadIdx.x;
    if (idx >= a.n_pairs * a.blocks) return;
    const int pair = idx / a.blocks, r = idx - pair * a.blocks;
    const StateAt at(K, a.window_log2);
    const i64 *const st = a.state_in + (size_t)pair * a.state_words;
    const Blocks record = { st, a.records + (size_t)pair * a.blocks * NS, NS, at.W, a.slot0 };
    int32_t *const wrec = a.weights + (size_t)idx * WREC;
    const int complete_in = (int)st[at.scalars + NVX_WANC_SC_COMPLETE], mode = (int)st[at.scalars + NVX_WANC_SC_MODE];
    if (mode != NVX_WANC_TRACK || (r == 0 && a.off0 != 0) || complete_in + r < at.W) {      // the carried weights
        for (int k = 0; k < 2 * K; k++) wrec[k] = (int32_t)st[at.weights + k];
        wrec[2 * K] = (int32_t)st[at.scalars + NVX_WANC_SC_COHERENCE]; wrec[2 * K + 1] = (int32_t)st[at.scalars + NVX_WANC_SC_REASON];
        wrec[2 * K + 2] = 0; wrec[2 * K + 3] = 0;
        return;
    }
    double *const my = ws + threadIdx.x;
    i64 R0 = 0, TAA = 0;
    for (int k = 0; k < NS; k++) {
        i64 t = 0;
        for (int j = r - at.W; j < r; j++) t += record(j, k);
        if (k == 0) R0 = t;
        if (k < 4 * K) my[(size_t)k * NVX_WANC_SOLVE_LANES] = (double)t;
        else TAA = t;
    }
    int32_t coherence;
    // the tap count as a number the compiler does not know: the loops of the solve stay loops
    const int reason = nvx_wanc_solve(a.n_taps, a.window_log2, a.load_log2, R0, TAA, my, NVX_WANC_SOLVE_LANES, wrec, 1, &coherence);
    wrec[2 * K] = coherence; wrec[2 * K + 1] = reason; wrec[2 * K + 2] = 1; wrec[2 * K + 3] = 0;
    atomicAdd(&a.counters[2 * (size_t)pair + (reason ? 1 : 0)], 1ull);
}

// ----------------------------------------------------------------------------------------------------------------- apply
template <int FMT, int K>
__global__ __launch_bounds__(NVX_WANC_THREADS) void nvx_wanc_apply(const nvx_wanc_args a)
{
    constexpr int NS = NVX_WANC_SUMS(K), KP = Reach<K>::KP, G = K / 2, WREC = NVX_WANC_WREC(K);
    __shared__ __attribute__((aligned(16))) uint32_t sense[NVX_WANC_PAD + NVX_WANC_TILE];
    __shared__ __attribute__((aligned(16))) uint32_t mainw[NVX_WANC_TILE];
    const int tid = threadIdx.x, lane = tid & 63, pair = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const char *const row_a = (const char *)a.in_main + (size_t)pair * a.pitch_main * Fmt<FMT>::BPS;
    const char *const row_b = (const char *)a.in_sense + (size_t)pair * a.pitch_sense * Fmt<FMT>::BPS;
    uint32_t *const out = a.out + (size_t)pair * a.pitch_out + a.out_first;
    const int32_t *const wrecs = a.weights + (size_t)pair * a.blocks * WREC;
    const StateAt at(K, a.window_log2);
    const i64 *const st = a.state_in + (size_t)pair * a.state_words;
    const int n_in = a.n_in;
    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
    const int first = wave * NVX_WANC_REGION + lane * Shape<FMT>::SPT;     // the first sample of a tile this thread loads
    const int mine = wave * NVX_WANC_REGION + lane * 4;                     // ... and the first it writes

    // the weights of block r as the words the dot products take, (w_re, -w_im) and (w_im, w_re), low half first: the same
    // in every lane, and in vector registers, of which the kernel has plenty (the scalar ones are taken by its arguments)
    uint32_t kp[K], kr[K];
    auto weights_of = [&](int r) {
        const int32_t *const wr = wrecs + (size_t)r * WREC;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int re = wr[k], im = wr[K + k];
            kp[k] = ((uint32_t)re & 0xffffu) | ((uint32_t)(-im) << 16);
            kr[k] = ((uint32_t)im & 0xffffu) | ((uint32_t)re << 16);
        }
    };
    int cur = -1;                                                           // the block kp and kr belong to

    // the tile's samples [lo, hi)
    auto pass = [&](int tbase, int lo, int hi) {
#pragma unroll 1
        for (int j = 0; j < NVX_WANC_REGION / 256; j++) {
            const int o = mine + j * 256;
            if (o + 4 <= lo || o >= hi) continue;
            uint32_t w[Reach<K>::WORDS], ma[4], y[4];
            read_group<K>(sense, mainw, o, w, ma);
#pragma unroll
            for (int s = 0; s < 4; s++) {
                int p = 4096, r = 4096;
#pragma unroll
                for (int k = 0; k < K; k++) { p = dot2(w[KP + s - k], kp[k], p); r = dot2(w[KP + s - k], kr[k], r); }
                const int oi = clamp16(lo16s(ma[s]) - (p >> 13)), oq = clamp16(hi16s(ma[s]) - (r >> 13));
                y[s] = ((uint32_t)oi & 0xffffu) | ((uint32_t)oq << 16);
            }
            uint32_t *const dst = out + tbase + o;
            if (a.out_vec && o >= lo && o + 4 <= hi) {
                const u32x4 v = { y[0], y[1], y[2], y[3] };
                __builtin_nontemporal_store(v, (u32x4 *)dst);
            } else {
#pragma unroll
                for (int s = 0; s < 4; s++)
                    if (o + s >= lo && o + s < hi) dst[s] = y[s];
            }
        }
    };

    for (int tile = tile0; tile < tile1; tile++) {
        const int tbase = tile * NVX_WANC_TILE, boff = a.off0 + tbase;
        const int r = boff >> 16, n_a = NVX_WANC_BLOCK - (boff & (NVX_WANC_BLOCK - 1));     // the tile's samples in front of the block's end
        const int hi = n_in - tbase < NVX_WANC_TILE ? n_in - tbase : NVX_WANC_TILE;
        const bool split = n_a < hi;                                // the end lies inside the tile, and inside the call
        __syncthreads();
        if (tbase + NVX_WANC_TILE <= n_in) stage<FMT, K, true, true>(sense, mainw, row_a, row_b, st + at.sense, st + at.main, tbase, n_in, tid, first);
        else stage<FMT, K, false, true>(sense, mainw, row_a, row_b, st + at.sense, st + at.main, tbase, n_in, tid, first);
        __syncthreads();
        // one walk, or two where the block ends inside: [0, n_a) with block r's weights, [n_a, hi) with the next one's
#pragma unroll 1
        for (int part = 0; part <= (int)split; part++) {
            if (r + part != cur) { weights_of(r + part); cur = r + part; }
            pass(tbase, part ? n_a : 0, split && !part ? n_a : hi);
        }
    }

    // the pair's state for the next call: by the workgroup of its last sample, into the row this launch does not read
    if (blockIdx.x == gridDim.x - 1) {
        i64 *const so = a.state_out + (size_t)pair * a.state_words;
        const Blocks record = { st, a.records + (size_t)pair * a.blocks * NS, NS, at.W, a.slot0 };
        const int done = (a.off0 + n_in) >> 16;                     // blocks that ended inside the call
        const int32_t *const last = wrecs + (size_t)(a.blocks - 1) * WREC;
        if (tid < at.W) {                                           // the last W complete blocks, each to its slot
            const int j = done - 1 - tid;
            for (int k = 0; k < NS; k++) so[(size_t)((a.slot0 + j) & (at.W - 1)) * NS + k] = record(j, k);
        } else if (tid == 64) {
            const bool open = ((a.off0 + n_in) & (NVX_WANC_BLOCK - 1)) != 0;
            for (int k = 0; k < NS; k++) so[(size_t)at.W * NS + k] = open ? record(done, k) : 0;
        } else if (tid == 65) {
            const int complete_in = (int)st[at.scalars + NVX_WANC_SC_COMPLETE];
            i64 *const sc = so + at.scalars;
            sc[NVX_WANC_SC_COMPLETE] = complete_in + done < at.W ? complete_in + done : at.W;
            sc[NVX_WANC_SC_COHERENCE] = last[2 * K]; sc[NVX_WANC_SC_MODE] = st[at.scalars + NVX_WANC_SC_MODE]; sc[NVX_WANC_SC_REASON] = last[2 * K + 1];
            for (int k = NVX_WANC_SC_REASON + 1; k < NVX_WANC_STATE_SCALARS; k++) sc[k] = 0;
        } else if (tid >= 128 && tid < 128 + 2 * K) {
            so[at.weights + tid - 128] = last[tid - 128];
        } else if (tid >= 192 && tid < 192 + K - 1) {               // b[n_in - (K - 1)] ..
            const int i = tid - 192, s = n_in - (K - 1) + i;
            so[at.sense + i] = s >= 0 ? (i64)load_sample<FMT>(row_b, s) : st[at.sense + K - 1 + s];
        } else if (tid >= 224 && tid < 224 + G) {                   // a[n_in - G] ..
            const int i = tid - 224, s = n_in - G + i;
            so[at.main + i] = s >= 0 ? (i64)load_sample<FMT>(row_a, s) : st[at.main + G + s];
        }
    }
}

template <int FMT, int K>
static hipError_t launch_three(const nvx_wanc_args *a, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((nvx_wanc_sums<FMT, K>), grid, dim3(NVX_WANC_THREADS), 0, s, *a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned solves = (unsigned)a->n_pairs * (unsigned)a->blocks;
    hipLaunchKernelGGL((nvx_wanc_solve_blocks<K>), dim3((solves + NVX_WANC_SOLVE_LANES - 1) / NVX_WANC_SOLVE_LANES), dim3(NVX_WANC_SOLVE_LANES), 0, s, *a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((nvx_wanc_apply<FMT, K>), grid, dim3(NVX_WANC_THREADS), 0, s, *a);
    return hipGetLastError();
}

hipError_t nvx_wanc_launch(const nvx_wanc_args *a, int format, int n_pairs, int chunks, hipStream_t s)
{
    const dim3 grid((unsigned)chunks, (unsigned)n_pairs);
    return nvx_for_format(format, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        switch (a->n_taps) {
        case 4: return launch_three<FMT, 4>(a, grid, s);
        case 8: return launch_three<FMT, 8>(a, grid, s);
        case 16: return launch_three<FMT, 16>(a, grid, s);
        }
        return hipErrorInvalidValue;
    });
}
