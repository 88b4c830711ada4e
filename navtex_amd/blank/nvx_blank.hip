// nvx_blank.hip -- the blanker's kernel (include/navtex_amd_blank.h states the arithmetic; this file arranges it).
//
//   nvx_blank<FMT>   grid (chunks, streams), 256 threads.  A workgroup walks consecutive tiles of 4096 samples of one stream,
//   counted from the call's first sample (rows are 16-byte aligned there; the blocks of the contract, counted from the
//   stream's reset, are not).  Wave w of the workgroup owns samples [1024 w, 1024 w + 1024) of the tile, its region: as long as
//   a block, so exactly one block ends inside it, behind its sample off - 1 (off = 1024 - position mod 1024, the same in
//   every region of a call).  The region's samples in front of that end are its A part, the rest its B part.
//
// Per tile:
//   load     16 samples per thread, all in flight at once: 16-byte non-temporal loads, a wave's instruction reading 1 KB
//            (CS16, CF32: 4 samples per lane and step, 4 steps; CU8, CS8: 8 samples, 2 steps; CF32 takes two loads per
//            step and issues them step by step).  Converted to packed words; m = |I| + |Q| is recomputed where it is
//            needed.  In the tile in which the call ends the group that straddles the end is read sample by sample.
//   sums     each wave adds m over its A and its B part (DPP inside the wave) and leaves both in the LDS.   -- barrier 1
//   levels   every wave walks the four regions in uniform registers: a region's A sum closes the open block, whose sum
//            enters the ring of the last four, and the level of the block that opens follows from the ring's minimum.  The
//            five levels go to the LDS and a wave reads back its two, by its own number.
//   detect   m against the level of its part, a bit per sample in one register; each thread's latest detection per step; an
//            exclusive max-scan of those over the wave (DPP), and the wave's latest detection to the LDS.  -- barrier 2
//   hold     the latest detection in front of each region: the carried one and those of the waves before it, picked as the
//            levels are.  A sample is blanked when the latest detection at or in front of it is at most `hold` back.
//   store    zero or the word: 16 bytes at a time, non-temporal where the output rows are 16-byte aligned.
// Between tiles one uniform set is carried: the ring, the partial sum, the blocks complete, the latest detection.  Chunk 0
// of a stream takes it from the stream's state row; a later chunk walks NVX_BLANK_PREROLL_TILES tiles in front of its own
// from nothing, storing and counting nothing: eight block ends later the ring, the partial sum and the detections of the
// last block (hold reaches no further) are the stream's own.  The last chunk writes the other state row.
// Integers only, except CF32's conversion.  The formats' sizes, load_sample and the CF32 rule are the resampler's
// (nvx_rs_device.h), and so are the tile's 16-byte loads (load_words).  The step's shape and store, the DPP controls, the wave
// sum and the dispatch on the format are the same-rate companions' (nvx_stream_device.h); the step's load is load_step's
// body written out ("What the same-rate kernels share", says why).  Registers: DESIGN 3.9 says why the A-part bounds pass through an empty asm, why
// the detections are bits, and why a wave's own values come back from the LDS.
#include "nvx_blank_plan.h"
#include "nvx_stream_device.h"

static_assert(NVX_BLANK_CS16 == NVX_RS_CS16 && NVX_BLANK_CU8 == NVX_RS_CU8 && NVX_BLANK_CS8 == NVX_RS_CS8 && NVX_BLANK_CF32 == NVX_RS_CF32, "formats");

#define NVX_BLANK_NONE (-(1 << 29))          // "no detection": further back than any hold, and far from wrapping
#define NVX_BLANK_OFF 0xffffffffu            // a level no magnitude exceeds

__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// the maximum over the lanes in front of this one (NVX_BLANK_NONE for lane 0); total: over the whole wave, uniform
__device__ __forceinline__ int wave_max_before(int v, int &total)
{
    v = imax(v, dpp<ROW_SHR1, 0xf>(NVX_BLANK_NONE, v)); v = imax(v, dpp<ROW_SHR2, 0xf>(NVX_BLANK_NONE, v));
    v = imax(v, dpp<ROW_SHR4, 0xf>(NVX_BLANK_NONE, v)); v = imax(v, dpp<ROW_SHR8, 0xf>(NVX_BLANK_NONE, v));
    v = imax(v, dpp<ROW_BCAST15, 0xa>(NVX_BLANK_NONE, v)); v = imax(v, dpp<ROW_BCAST31, 0xc>(NVX_BLANK_NONE, v));
    total = __builtin_amdgcn_readlane(v, 63);
    return dpp<WAVE_SHR1, 0xf>(NVX_BLANK_NONE, v);
}

__device__ __forceinline__ uint32_t magnitude(uint32_t w)
{
    const int i = (int)(w << 16) >> 16, q = (int)w >> 16;
    return (uint32_t)((i < 0 ? -i : i) + (q < 0 ? -q : q));
}

// the level of the block that opens behind `complete` blocks whose last four sums are s[0 .. 3]
__device__ __forceinline__ uint32_t level_of(const uint32_t (&s)[4], uint32_t complete, uint32_t thr_q8, uint32_t floor)
{
    const uint32_t a = s[0] < s[1] ? s[0] : s[1], b = s[2] < s[3] ? s[2] : s[3], ref = a < b ? a : b;
    const uint32_t lv = (thr_q8 * (ref >> 10)) >> 8;
    return (complete < 4 || thr_q8 == 0) ? NVX_BLANK_OFF : (lv > floor ? lv : floor);
}

// samples per lane and step, steps per region: a wave's region is a block
template <int FMT> using Shape = StreamShape<FMT, NVX_BLANK_BLOCK>;

template <int FMT>
__global__ __launch_bounds__(NVX_BLANK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void nvx_blank(const nvx_blank_args a)
{
    constexpr int SPT = Shape<FMT>::SPT, STEPS = Shape<FMT>::STEPS, PER = SPT * STEPS;      // PER = 16
    // per wave the sums of its two parts and its latest detection; the levels and the latest detections in front of the regions
    enum { X_SUMS = 0, X_LATEST = 8, X_LEVELS = 12, X_FRONTS = 17 };
    __shared__ uint32_t xch[NVX_BLANK_LDS_BYTES / 4];

    const int tid = threadIdx.x, lane = tid & 63, stream = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const char *const row = (const char *)a.in + (size_t)stream * a.pitch_in * Fmt<FMT>::BPS;
    uint32_t *const out = a.out + (size_t)stream * a.pitch_out + a.out_first;
    const int n_in = a.n_in, off = a.off, hold = a.hold;

    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;

    // the carried set, uniform: chunk 0 from the stream's state row, a later chunk from nothing and a pre-roll
    uint32_t ring[4] = { 0, 0, 0, 0 }, partial = 0, complete = 0;
    int latest = -(hold + 1);                               // the latest detection, as a sample of the tile (here: in front of it)
    int tile = tile0 - NVX_BLANK_PREROLL_TILES;
    if (blockIdx.x == 0) {
        const uint32_t *st = a.state_in + (size_t)stream * NVX_BLANK_STATE_WORDS;
        ring[0] = st[0]; ring[1] = st[1]; ring[2] = st[2]; ring[3] = st[3]; partial = st[4]; complete = st[5];
        latest = (int)st[6] - (hold + 1);
        tile = 0;
    }
    uint32_t level = __builtin_amdgcn_readfirstlane(level_of(ring, complete, a.thr_q8, a.floor));       // of the open block
    uint32_t n_det = 0, n_blank = 0;

    const int lim0 = off - lane * SPT;                      // sample (j, k) of this thread lies in the A part where j * 64 * SPT + k < lim0
    // One tile.  FULL: all of it lies inside the call (every tile but a call's last, and every tile of a pre-roll).
    auto walk = [&](auto full) {
        constexpr bool FULL = decltype(full)::value;
        const bool live = !FULL || tile >= tile0;
        const int base = tile * NVX_BLANK_TILE + wave * NVX_BLANK_BLOCK + lane * SPT;       // this thread's first sample, of the call
        const int tile_n = FULL ? NVX_BLANK_TILE : n_in - tile * NVX_BLANK_TILE;
        const char *const src = row + (size_t)base * Fmt<FMT>::BPS;
        uint32_t *const dst = out + base;

        // ---- load and convert: sample (j, k) of this thread is sample j * 64 * SPT + lane * SPT + k of the wave's region
        uint32_t w[PER];
#pragma unroll
        for (int j = 0; j < STEPS; j++) {
            // float32 brings twice the bytes: its loads go out step by step, or thirty-two registers wait for them
            if (FMT == NVX_RS_CF32 && j > 0) __builtin_amdgcn_sched_barrier(0);
            if (FULL || base + j * 64 * SPT + SPT <= n_in) load_words<FMT>(src, j * 64 * SPT, &w[j * SPT]);
            else {
#pragma unroll
                for (int k = 0; k < SPT; k++) w[j * SPT + k] = base + j * 64 * SPT + k < n_in ? load_sample<FMT>(src, j * 64 * SPT + k) : 0u;
            }
        }
        // n_a: how many of this thread's samples of step j lie in the A part (they come first).  The same in every tile, so it
        // goes through an empty asm: otherwise the sixteen comparisons below are made once, in front of the loop, and held as
        // lane masks across it, 32 scalar registers
        uint32_t sum_a = 0, sum_b = 0;
        int n_a = lim0;
#pragma unroll
        for (int j = 0; j < STEPS; j++) {
            asm volatile("" : "+v"(n_a));
#pragma unroll
            for (int k = 0; k < SPT; k++) {
                const uint32_t m = magnitude(w[j * SPT + k]);               // of a word behind the call's end: zero
                sum_a += k < n_a ? m : 0u; sum_b += k < n_a ? 0u : m;
            }
            n_a -= 64 * SPT;
        }
        sum_a = wave_sum(sum_a); sum_b = wave_sum(sum_b);
        if (lane == 0) { xch[X_SUMS + 2 * wave] = sum_a; xch[X_SUMS + 2 * wave + 1] = sum_b; }
        __syncthreads();

        // ---- the four regions in order, the same in every wave: the level in front of each and the set behind the tile.  A
        // wave picks its two levels from the LDS by its own number (selecting by comparisons costs a lane mask each); every
        // wave writes the same five words, and reads them before barrier 2, which the next tile's writers are behind.
        xch[X_LEVELS] = level;
#pragma unroll
        for (int r = 0; r < NVX_BLANK_WAVES; r++) {
            const uint32_t sa = __builtin_amdgcn_readfirstlane(xch[X_SUMS + 2 * r]), sb = __builtin_amdgcn_readfirstlane(xch[X_SUMS + 2 * r + 1]);
            if (FULL || tile_n - r * NVX_BLANK_BLOCK >= off) {      // the block ends inside the call
                ring[0] = ring[1]; ring[1] = ring[2]; ring[2] = ring[3]; ring[3] = partial + sa;
                partial = sb;
                complete = complete < 4 ? complete + 1 : 4;
                level = level_of(ring, complete, a.thr_q8, a.floor);
            } else partial += sa;                           // the call ends first: sb is zero
            xch[X_LEVELS + 1 + r] = level;
        }
        const uint32_t level_a = xch[X_LEVELS + wave], level_b = xch[X_LEVELS + wave + 1];

        // ---- detections: a bit per sample; per step this thread's latest, then the latest of the lanes in front
        uint32_t det = 0;                                   // bit j * SPT + k: sample (j, k) is a detection
#pragma unroll
        for (int j = STEPS - 1; j >= 0; j--) {              // from the last sample down: each bit is shifted in at the bottom
            n_a += 64 * SPT;
            asm volatile("" : "+v"(n_a));
#pragma unroll
            for (int k = SPT - 1; k >= 0; k--)
                det = (det << 1) | (magnitude(w[j * SPT + k]) > (k < n_a ? level_a : level_b) ? 1u : 0u);
        }
        asm volatile("" : "+v"(det));                       // one register of bits from here on, not sixteen lane masks
        if (live) n_det += (uint32_t)__builtin_popcount(det);
        // detections of a step are counted from the step's first sample, so that the lane's own offset is the only number a
        // thread keeps; step j of this wave starts at sample step0 + j * 64 * SPT of the tile (NONE plus that is still none)
        const int step0 = wave * NVX_BLANK_BLOCK;
        int before[STEPS], step_total[STEPS], region_latest = NVX_BLANK_NONE;
#pragma unroll
        for (int j = 0; j < STEPS; j++) {
            const uint32_t bits = (det >> (j * SPT)) & ((1u << SPT) - 1);
            const int mine = bits ? lane * SPT + 31 - __builtin_clz(bits) : NVX_BLANK_NONE;
            before[j] = wave_max_before(mine, step_total[j]);
            region_latest = imax(region_latest, step_total[j] + step0 + j * 64 * SPT);
        }
        if (lane == 0) xch[X_LATEST + wave] = (uint32_t)region_latest;
        __syncthreads();

        // ---- hold: the latest detection in front of each region, picked as the levels are, and behind the tile
#pragma unroll
        for (int r = 0; r < NVX_BLANK_WAVES; r++) {
            xch[X_FRONTS + r] = (uint32_t)latest;
            latest = imax(latest, __builtin_amdgcn_readfirstlane((int)xch[X_LATEST + r]));
        }
        int front = __builtin_amdgcn_readfirstlane((int)xch[X_FRONTS + wave]);
        // ---- ... and the stores.  Sample k of a step is blanked where reach >= k: reach = the latest detection + hold, counted
        // from the thread's first sample of the step
#pragma unroll
        for (int j = 0; j < STEPS; j++) {
            int reach = imax(front - (step0 + j * 64 * SPT), before[j]) - lane * SPT + hold;
            uint32_t gone = 0;
#pragma unroll
            for (int k = 0; k < SPT; k++) {
                if (__builtin_amdgcn_ubfe(det, j * SPT + k, 1)) reach = k + hold;
                if (reach >= k && (FULL || base + j * 64 * SPT + k < n_in)) { w[j * SPT + k] = 0u; gone++; }
            }
            front = imax(front, step_total[j] + step0 + j * 64 * SPT);
            if (live) {
                n_blank += gone;
                store_step<FMT, FULL>(dst, a.out_vec, base, j, n_in, &w[j * SPT]);
            }
        }
        // the next tile counts its samples from its own first; the next call from the end of this one
        latest = imax(latest - tile_n, -(hold + 1));
    };
    for (; tile < tile1 && (tile + 1) * NVX_BLANK_TILE <= n_in; tile++) walk(std::true_type{});
    if (tile < tile1) walk(std::false_type{});              // the call's last tile, where it is not a whole one

    n_det = wave_sum(n_det); n_blank = wave_sum(n_blank);
    if (lane == 0 && (n_det | n_blank)) {
        if (n_det) atomicAdd(&a.counters[2 * (size_t)stream], (unsigned long long)n_det);
        if (n_blank) atomicAdd(&a.counters[2 * (size_t)stream + 1], (unsigned long long)n_blank);
    }
    // the stream's state for the next call: by the last chunk, into the row this launch does not read
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {
        uint32_t *st = a.state_out + (size_t)stream * NVX_BLANK_STATE_WORDS;
        st[0] = ring[0]; st[1] = ring[1]; st[2] = ring[2]; st[3] = ring[3]; st[4] = partial; st[5] = complete;
        st[6] = (uint32_t)(latest + hold + 1); st[7] = 0u;
    }
}

template <int FMT>
static hipError_t launch_one(const nvx_blank_args *a, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((nvx_blank<FMT>), grid, dim3(NVX_BLANK_THREADS), 0, s, *a);
    return hipGetLastError();
}

hipError_t nvx_blank_launch(const nvx_blank_args *a, int format, int n_streams, int chunks, hipStream_t s)
{
    const dim3 grid((unsigned)chunks, (unsigned)n_streams);
    return nvx_for_format(format, [&](auto fmt) { return launch_one<decltype(fmt)::value>(a, grid, s); });
}
