// nvx_narrow.hip -- the narrowband interpolator's kernel (include/navtex_amd_narrow.h states the arithmetic; this file
// arranges it).
//
//   nvx_nb<FMT, KIND, TQ>   grid (chunks, streams), 256 threads; TQ = ceil(T / 8), the 16-byte words of a tap row, is 2, 3 or
//   4: the window's registers are counted at compile time, and one kernel with all three bodies spills scalar registers.
//   Window-stationary: an interpolator's L / M consecutive outputs share one window of T input samples, so a thread keeps
//   the window in registers (Tp = 8 TQ samples: the oldest Tp - T meet zero taps) and reads only taps.  A workgroup walks
//   consecutive tiles of `windows` input samples of one stream (256, or 128 / 64 where a window has more than 32 / 64
//   outputs and two / four threads share it).  The tap table lies in the LDS, copied once per workgroup (nvx_narrow_plan.h
//   has its layout).
//
// Per tile:
//   stage    the tile's input samples and the Tp - 1 in front of them, converted, as packed words in the LDS: from the
//            stream's state row in front of the call's first sample, from the input itself elsewhere (a pure FIR: no chunk
//            waits for another), zeros behind the call's end.  The input is 1 / 21 of the output at 12 kS/s: sample by sample.
//                                                                                                          -- barrier 1
//   window   a thread reads its window's Tp words (ds_read_b32, consecutive lanes side by side) and splits them into Tp / 2
//            words of I pairs and Tp / 2 of Q pairs (one v_perm_b32 each; the REAL kind has no Q).
//   filter   per output one row of the table, tq ds_read_b128 (rows are odd numbers of 16-byte words: the M rows a wave
//            reads at a time lie on different banks, and lanes on one row are one broadcast), and per 16-byte word four
//            v_dot2 for I and four for Q: one LDS read per 8 dot products (REAL: 4).  clamp16((acc + 2^13) >> 14), packed,
//            goes to the tile's output image in the LDS at the output's index.  The phase steps by M, the row by M rows.
//                                                                                                          -- barrier 2
//   store    the image as consecutive words: 16 bytes per lane, aligned, non-temporal, where the row's first output word is
//            16-byte aligned (the image starts at the tile's first output index rounded down to 4); word by word otherwise
//            and at the tile's ragged ends.
// The workgroup of a stream's last sample writes the other state row: the stream's last T - 1 samples, from the input, or
// from the state row read where the call is shorter than that.
// Integers only, except F32's conversion.  nvx_narrow_plan.h's functions give every position; nothing here divides.
#include "nvx_narrow_plan.h"
#include "nvx_rs_device.h"

static_assert(NVX_NB_S16 == NVX_RS_CS16 && NVX_NB_U8 == NVX_RS_CU8 && NVX_NB_S8 == NVX_RS_CS8 && NVX_NB_F32 == NVX_RS_CF32, "formats");
static_assert(NVX_NB_THREADS == NVX_RS_THREADS, "threads");
static_assert(NVX_NB_STAGE_WORDS >= NVX_NB_THREADS + NVX_NB_MAX_T - 1, "the stage");
static_assert(NVX_NB_OUT_WORDS >= NVX_NB_THREADS * NVX_NB_PART_OUTPUTS + 3 && NVX_NB_OUT_WORDS % 4 == 0, "the output image");

typedef __attribute__((address_space(3))) u32x4 lds_u4;

// sample idx of the row as a packed word: (I, Q), or (x, 0) for the REAL kind
template <int FMT, int KIND>
__device__ __forceinline__ uint32_t nb_sample(const char *row, int idx)
{
    if constexpr (KIND == NVX_NB_IQ) return load_sample<FMT>(row, idx);
    else if constexpr (FMT == NVX_RS_CS16) return ((const uint16_t *)row)[idx];
    else if constexpr (FMT == NVX_RS_CU8) return (((uint32_t)((const uint8_t *)row)[idx] << 8) ^ 0x8080u);     // (2 u - 255) * 128 in 16 bits
    else if constexpr (FMT == NVX_RS_CS8) return (uint32_t)((const uint8_t *)row)[idx] << 8;
    else return cf32_to_i16(((const uint32_t *)row)[idx]);
}
template <int FMT, int KIND> struct Bytes { static constexpr int value = KIND == NVX_NB_IQ ? Fmt<FMT>::BPS : Fmt<FMT>::BPS / 2; };

template <int FMT, int KIND, int TQ>
__device__ __forceinline__ void nb_walk(const nvx_nb_args &a, uint32_t *lds)
{
    constexpr int TP = 8 * TQ, NP = 4 * TQ;
    const int tid = threadIdx.x, stream = blockIdx.y;
    uint32_t *const stage = lds + (size_t)a.table_quads * 4, *const image = stage + NVX_NB_STAGE_WORDS;
    const char *const row = (const char *)a.in + (size_t)stream * a.pitch_in * Bytes<FMT, KIND>::value;
    uint32_t *const out = a.out + (size_t)stream * a.pitch_out + a.out_first;
    const uint32_t *const st = a.state_in + (size_t)stream * NVX_NB_STATE_WORDS;
    const int n_in = a.n_in, T = a.T, windows = a.windows;
    const bool vec = ((uintptr_t)out & 15) == 0;

    // the table
    for (int i = tid; i < a.table_quads; i += NVX_NB_THREADS) ((u32x4 *)lds)[i] = ((const u32x4 *)a.table)[i];

    // this thread's window of a tile, and which of its outputs
    const int w = tid >> a.pshift, first_j = (tid & ((1 << a.pshift) - 1)) * a.part;
    uint32_t aw, bw;
    nvx_nb_divmod((uint32_t)w * (uint32_t)a.L, (uint32_t)a.M, 19, &aw, &bw);

    const int tile0 = (int)blockIdx.x * a.tiles_per_chunk;
    const int tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
    uint32_t ti, tr;                                                // the tile's first output and its phase
    nvx_nb_chunk_start(a, blockIdx.x, &ti, &tr);

    for (int tile = tile0; tile < tile1; tile++) {
        const int kb = tile * windows;
        // ---- stage
        for (int t = tid; t < windows + TP - 1; t += NVX_NB_THREADS) {
            const int idx = kb - (TP - 1) + t;
            uint32_t v = 0;
            if (idx >= 0) { if (idx < n_in) v = nb_sample<FMT, KIND>(row, idx); }
            else if (idx >= 1 - T) v = st[T - 1 + idx];
            stage[t] = v;
        }
        __syncthreads();

        uint32_t ni, nr;
        nvx_nb_tile_next(a, ti, tr, &ni, &nr);
        const uint32_t i_end = kb + windows >= n_in ? (uint32_t)a.n_out : ni;     // behind the tile's last output
        const uint32_t image0 = ti & ~3u;

        // ---- window and filter
        if (kb + w < n_in) {
            uint32_t i0, r0;
            int count;
            nvx_nb_window_first(a, ti, tr, aw, bw, &i0, &r0, &count);
            const int last_j = first_j + a.part < count ? first_j + a.part : count;
            uint32_t xi[NP], xq[NP];
#pragma unroll
            for (int u = 0; u < NP; u++) {
                const uint32_t s0 = stage[w + 2 * u], s1 = stage[w + 2 * u + 1];
                xi[u] = lo_pair(s0, s1);
                if constexpr (KIND == NVX_NB_IQ) xq[u] = hi_pair(s0, s1);
            }
            const lds_u4 *taps = (const lds_u4 *)lds + (r0 + (uint32_t)(first_j * a.M)) * (uint32_t)a.row_quads;
            const int row_step = a.M * a.row_quads;
            uint32_t *dst = image + (i0 - image0) + first_j;
            for (int j = first_j; j < last_j; j++) {
                int acc_i = 1 << (NVX_NB_SHIFT - 1), acc_q = 1 << (NVX_NB_SHIFT - 1);
#pragma unroll
                for (int u = 0; u < TQ; u++) {
                    const u32x4 h = taps[u];
                    acc_i = dot2(xi[4 * u], h.x, acc_i); acc_i = dot2(xi[4 * u + 1], h.y, acc_i);
                    acc_i = dot2(xi[4 * u + 2], h.z, acc_i); acc_i = dot2(xi[4 * u + 3], h.w, acc_i);
                    if constexpr (KIND == NVX_NB_IQ) {
                        acc_q = dot2(xq[4 * u], h.x, acc_q); acc_q = dot2(xq[4 * u + 1], h.y, acc_q);
                        acc_q = dot2(xq[4 * u + 2], h.z, acc_q); acc_q = dot2(xq[4 * u + 3], h.w, acc_q);
                    }
                }
                const uint32_t vi = (uint32_t)clamp16(acc_i >> NVX_NB_SHIFT) & 0xffffu;
                if constexpr (KIND == NVX_NB_IQ) *dst = vi | ((uint32_t)clamp16(acc_q >> NVX_NB_SHIFT) << 16);
                else *dst = vi;
                dst++;
                taps += row_step;
            }
        }
        __syncthreads();

        // ---- store: image word s is output image0 + s of the call
        const uint32_t slots = i_end - image0;
        if (vec) {
            for (uint32_t s = 4 * tid; s < slots; s += 4 * NVX_NB_THREADS) {
                const uint32_t i = image0 + s;
                if (i >= ti && i + 4 <= i_end) __builtin_nontemporal_store(*(const u32x4 *)&image[s], (u32x4 *)(out + i));
                else {
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        if (i + c >= ti && i + c < i_end) out[i + c] = image[s + c];
                }
            }
        } else {
            for (uint32_t s = (ti - image0) + tid; s < slots; s += NVX_NB_THREADS) out[image0 + s] = image[s];
        }
        ti = ni; tr = nr;
    }

    // the stream's state for the next call: by the workgroup of its last sample, into the row this launch does not read
    if (blockIdx.x == gridDim.x - 1 && tid < T - 1) {
        const int at = n_in - (T - 1) + tid;
        a.state_out[(size_t)stream * NVX_NB_STATE_WORDS + tid] = at >= 0 ? nb_sample<FMT, KIND>(row, at) : st[T - 1 + at];
    }
}

template <int FMT, int KIND, int TQ>
__global__ __launch_bounds__(NVX_NB_THREADS) void nvx_nb(const nvx_nb_args a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t nb_lds[];
    nb_walk<FMT, KIND, TQ>(a, nb_lds);
}

#define NB_LDS_MAX ((size_t)NVX_NB_MAX_PHASES * 5 * 16 + (NVX_NB_STAGE_WORDS + NVX_NB_OUT_WORDS) * sizeof(uint32_t))

// the family: format, kind, and the 16-byte words of a tap row (2, 3, 4: T up to 16, 24, 32)
typedef void (*nb_kernel)(const nvx_nb_args);
#define NB_ROWS(FMT, KIND) nvx_nb<FMT, KIND, 2>, nvx_nb<FMT, KIND, 3>, nvx_nb<FMT, KIND, 4>
static const nb_kernel NB_FAMILY[4 * 2 * 3] = {
    NB_ROWS(NVX_RS_CS16, NVX_NB_IQ), NB_ROWS(NVX_RS_CS16, NVX_NB_REAL), NB_ROWS(NVX_RS_CU8, NVX_NB_IQ), NB_ROWS(NVX_RS_CU8, NVX_NB_REAL),
    NB_ROWS(NVX_RS_CS8, NVX_NB_IQ), NB_ROWS(NVX_RS_CS8, NVX_NB_REAL), NB_ROWS(NVX_RS_CF32, NVX_NB_IQ), NB_ROWS(NVX_RS_CF32, NVX_NB_REAL),
};

void nvx_nb_prepare(void)
{
    // a runtime that does not know the attribute launches with whatever LDS the launch names; one that enforces it has it set
    for (const nb_kernel k : NB_FAMILY)
        if (hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)NB_LDS_MAX) != hipSuccess) (void)hipGetLastError();
}

hipError_t nvx_nb_launch(const nvx_nb_args *a, int format, int kind, int n_streams, int chunks, hipStream_t s)
{
    const dim3 grid((unsigned)chunks, (unsigned)n_streams);
    if (format < NVX_NB_S16 || format > NVX_NB_F32 || kind < NVX_NB_IQ || kind > NVX_NB_REAL || a->tq < 2 || a->tq > 4 || nvx_nb_lds_bytes(a) > NB_LDS_MAX)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(NB_FAMILY[(format * 2 + kind) * 3 + a->tq - 2], grid, dim3(NVX_NB_THREADS), nvx_nb_lds_bytes(a), s, *a);
    return hipGetLastError();
}
