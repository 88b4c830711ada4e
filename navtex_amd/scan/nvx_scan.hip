// nvx_scan.hip -- the band scan's kernels (include/navtex_amd_scan.h states the arithmetic; this file only arranges it).
//
//   nvx_scan_stream   one workgroup per stream: walks the frames and their slots, both sums in registers, writes the row
//   nvx_scan_frame    one workgroup per (stream, frame): the frame's row into a scratch [stream][frame][2048]
//   nvx_scan_fold     the scan's row from the frame rows, ascending
//
// A workgroup is 256 threads; one slot at a time:
//   stage   the slot's 8256 samples at 252 kS/s -- raw input through stage 0 -- as int16 pairs in the LDS (33 KB; fp64
//           would be 132 KB), converted on read.  Local sample l is sample 4 * (first output - 16) + l of the stream.
//   FIR1    thread t computes outputs n = t + 256 k, k = 0 .. 7, from ten 16-byte LDS reads each (consecutive threads,
//           consecutive quads: conflict-free), in the reference's operand order, and windows them: 8 complex values in
//           registers.  These are the outputs n = t mod 256, i.e. after bit reversal the CONTIGUOUS block of eight
//           positions 8 * rev8(t) + rev3(k): the stages len = 2, 4, 8 run in registers.
//   FFT     the block goes to the LDS (re[] and im[] apart, over the staging area, which is dead by then), and the stages
//           len = 16 .. 2048 run as four passes of two radix-2 levels each (h = 8, 32, 128, 512: a thread holds
//           x[i0 + {0, h, 2h, 3h}]), the arithmetic of every butterfly exactly the header's.  The last pass writes
//           nothing back: its outputs are bins j + 512 m, and the thread adds their powers to its eight sums.
//   LDS index swizzle: position i lives at i ^ rev5((i >> 5) & 31).  Lanes that vary bits 0..2 and 5..6 of i (pass h = 8)
//   and lanes that vary bits 6..10 (the block store) then spread over the banks like lanes that vary bits 0..4.
// The twiddles (cos, -sin)[1024] are a second LDS table, 16 KB, filled once per workgroup: 49 KB in all, three
// workgroups per CU.  No fp64 fused multiply-add (the build's -ffp-contract=off), no atomics: the sums' order is fixed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nvx_scan_kernels.h"
#include "nvx_scan_table.h"
#include "nvx_tables.h"

#define SCAN_THREADS 256
#define SCAN_STAGE 8256                   // samples at 252 kS/s a slot's segment needs, lead-in included: 64 + 4 * 2048
#define SCAN_STAGE_FIRST 28               // FIR1 reaches back to local sample 31: stage 0 starts here (raw: 8 * 28 - 14 >= 0)

// The full table, built from the octant at compile time: tw[j] = (C[j], -S[j]), j = 0 .. 1023
struct ScanTwiddles {
    double v[1024][2];
    constexpr ScanTwiddles() : v{}
    {
        for (int j = 0; j < 1024; j++) { v[j][0] = nvx_scan_cs(j, 0); v[j][1] = -nvx_scan_cs(j, 1); }
    }
};
__device__ const ScanTwiddles nvx_scan_tw = ScanTwiddles();

// stage 0, third order: the 22 weights are three 8-sample boxcars convolved
struct Cic3Weights {
    int w[24];
    constexpr Cic3Weights() : w{}
    {
        int a[8] = {1, 1, 1, 1, 1, 1, 1, 1}, b[15] = {}, c[22] = {};
        for (int i = 0; i < 8; i++) for (int j = 0; j < 8; j++) b[i + j] += a[i] * a[j];
        for (int i = 0; i < 15; i++) for (int j = 0; j < 8; j++) c[i + j] += b[i] * a[j];
        for (int i = 0; i < 22; i++) w[i] = c[i];
    }
};
static constexpr Cic3Weights CIC3 = Cic3Weights();

__device__ __forceinline__ int lo16(uint32_t x) { return (int)(int16_t)(x & 0xffffu); }
__device__ __forceinline__ int hi16(uint32_t x) { return (int)x >> 16; }
__device__ __forceinline__ uint32_t pack16(int i, int q) { return ((uint32_t)i & 0xffffu) | ((uint32_t)q << 16); }
__device__ __forceinline__ int swz(int i) { return i ^ (int)(__builtin_bitreverse32((uint32_t)(i >> 5) & 31u) >> 27); }

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// 16 bytes of input, read once: a streaming load
__device__ __forceinline__ uint4 load_nt(const uint4 *p)
{
    const u32x4 v = __builtin_nontemporal_load((const u32x4 *)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
struct Block8 { uint4 a, b; };            // eight raw samples
__device__ __forceinline__ Block8 load_block(const uint4 *p)
{
    Block8 r;
    r.a = load_nt(p);
    r.b = load_nt(p + 1);
    return r;
}
// sum_i w[off - i] x_i over the block's eight samples, both components
template <int OFF>
__device__ __forceinline__ void cic3_dot(const Block8 &x, int &si, int &sq)
{
    const uint32_t s[8] = { x.a.x, x.a.y, x.a.z, x.a.w, x.b.x, x.b.y, x.b.z, x.b.w };
    si = 0; sq = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { si += CIC3.w[OFF - i] * lo16(s[i]); sq += CIC3.w[OFF - i] * hi16(s[i]); }
}

// The slot's samples at 252 kS/s into xs[SCAN_STAGE].  src: the slot's first sample of the input.
__device__ __forceinline__ void stage_slot(const uint32_t *src, int mode, uint32_t *xs, int t)
{
    // Loads first, a batch of them per thread and none behind a branch (an index past the end is clamped: the same bytes
    // again, inside the slot), then the arithmetic: the loads of a batch are in flight together.
    if (mode == NVX_SCAN_MODE_252K) {
        const uint4 *s4 = (const uint4 *)src;
        uint4 *x4 = (uint4 *)xs;
        constexpr int NQ = SCAN_STAGE / 4, NB = (NQ + SCAN_THREADS - 1) / SCAN_THREADS;      // 2064 quads: 9 per thread
        uint4 v[NB];
#pragma unroll
        for (int u = 0; u < NB; u++) { const int i = t + SCAN_THREADS * u; v[u] = load_nt(s4 + (i < NQ ? i : NQ - 1)); }
#pragma unroll
        for (int u = 0; u < NB; u++) { const int i = t + SCAN_THREADS * u; if (i < NQ) x4[i] = v[u]; }
    } else if (mode == NVX_SCAN_MODE_RAW1) {
        constexpr int NB = 11;                                    // 33 rounds of 256 outputs: three batches
        for (int l0 = t; l0 < SCAN_STAGE; l0 += NB * SCAN_THREADS) {
            Block8 x[NB];
#pragma unroll
            for (int u = 0; u < NB; u++) { const int l = l0 + SCAN_THREADS * u; x[u] = load_block((const uint4 *)src + 2 * (l < SCAN_STAGE ? l : SCAN_STAGE - 1)); }
#pragma unroll
            for (int u = 0; u < NB; u++) {
                const int l = l0 + SCAN_THREADS * u;
                const Block8 &b = x[u];
                const int si = lo16(b.a.x) + lo16(b.a.y) + lo16(b.a.z) + lo16(b.a.w) + lo16(b.b.x) + lo16(b.b.y) + lo16(b.b.z) + lo16(b.b.w) + 4;
                const int sq = hi16(b.a.x) + hi16(b.a.y) + hi16(b.a.z) + hi16(b.a.w) + hi16(b.b.x) + hi16(b.b.y) + hi16(b.b.z) + hi16(b.b.w) + 4;
                if (l < SCAN_STAGE) xs[l] = l < SCAN_STAGE_FIRST ? 0u : pack16(si >> 3, sq >> 3);      // arithmetic shift: floor
            }
        }
    } else {
        // y[l] = A_l + B_(l-1) + C_(l-2): A, B, C the block's sums weighted w[7-i], w[15-i], w[23-i].  A lane takes B and C
        // of the blocks in front from its neighbours in the wave; lanes 0 and 1 load those blocks themselves.
        const int lane = t & 63;
        constexpr int NB = 3;                                     // 33 rounds: eleven batches
        for (int l0 = t; l0 < SCAN_STAGE; l0 += NB * SCAN_THREADS) {
            Block8 x[NB], x1[NB], x2[NB];
            int lc[NB];
#pragma unroll
            for (int u = 0; u < NB; u++) {
                const int l = l0 + SCAN_THREADS * u;
                lc[u] = l < SCAN_STAGE ? l : SCAN_STAGE - 1;      // every lane takes part in the shuffles
                x[u] = load_block((const uint4 *)src + 2 * lc[u]);
                if (lane < 2 && lc[u] >= SCAN_STAGE_FIRST) {
                    x2[u] = load_block((const uint4 *)src + 2 * (lc[u] - 2));
                    if (lane == 0) x1[u] = load_block((const uint4 *)src + 2 * (lc[u] - 1));
                }
            }
#pragma unroll
            for (int u = 0; u < NB; u++) {
                const int l = l0 + SCAN_THREADS * u;
                int ai, aq, bi, bq, ci, cq;
                cic3_dot<7>(x[u], ai, aq); cic3_dot<15>(x[u], bi, bq); cic3_dot<23>(x[u], ci, cq);
                int b1i = __shfl_up(bi, 1), b1q = __shfl_up(bq, 1), c2i = __shfl_up(ci, 2), c2q = __shfl_up(cq, 2);
                if (lane < 2 && lc[u] >= SCAN_STAGE_FIRST) {
                    cic3_dot<23>(x2[u], c2i, c2q);
                    if (lane == 0) cic3_dot<15>(x1[u], b1i, b1q);
                }
                if (l < SCAN_STAGE)
                    xs[l] = l < SCAN_STAGE_FIRST ? 0u : pack16((ai + b1i + c2i + 256) >> 9, (aq + b1q + c2q + 256) >> 9);
            }
        }
    }
}

struct Cx { double re, im; };
// the header's butterfly: t = b * (wr, wi); a, b <- a + t, a - t
__device__ __forceinline__ void bfly(Cx &a, Cx &b, double wr, double wi)
{
    const double tr = b.re * wr - b.im * wi;
    const double ti = b.re * wi + b.im * wr;
    b.re = a.re - tr; b.im = a.im - ti;
    a.re = a.re + tr; a.im = a.im + ti;
}

// One slot: adds the powers of the thread's eight bins -- row indices t + 256 m -- to acc[m].
__device__ __forceinline__ void scan_slot(const uint32_t *src, int mode, uint32_t *xs, const double2 *tw, int t, double (&acc)[8])
{
    double *re = (double *)xs, *im = re + NVX_SCAN_FFT;
    // every address below derives from t: opaque per slot, so that the compiler computes them where they are used -- as
    // invariants of the slot loop they are some eighty registers, which it would hoist and then spill
    asm volatile("" : "+v"(t));
    stage_slot(src, mode, xs, t);
    __syncthreads();

    // FIR1 and the window: v[e] is position 8 * rev8(t) + e of the bit-reversed order, e = rev3(k)
    Cx v[8];
    const uint4 *x4 = (const uint4 *)xs;
    // the taps in scalar registers, set here for every slot: as loop invariants in vector registers they would be spilled
    double h1[NVX_T1];
#pragma unroll
    for (int i = 0; i < NVX_T1; i++) { h1[i] = NVX_H1[i]; asm volatile("" : "+s"(h1[i])); }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int n = t + SCAN_THREADS * k;
        double yi = 0.0, yq = 0.0;
#pragma unroll
        for (int qd = 16; qd >= 7; qd--) {                        // local samples 4 n + 67 (tap 0) down to 4 n + 31 (tap 36)
            uint4 s = x4[n + qd];
            asm("" : "+v"(s.x), "+v"(s.y), "+v"(s.z), "+v"(s.w));  // all four are wanted: one 16-byte read, not the used dwords in pairs
            const uint32_t e4[4] = { s.x, s.y, s.z, s.w };
#pragma unroll
            for (int e = 3; e >= 0; e--) {
                const int i = 67 - 4 * qd - e;
                if (i >= 0 && i < NVX_T1) {
                    yi = yi + h1[i] * (double)lo16(e4[e]);
                    yq = yq + h1[i] * (double)hi16(e4[e]);
                }
            }
        }
        const double c = n < 1024 ? tw[n].x : -tw[n - 1024].x;   // C[n]: half a turn is a sign flip
        const double w = 0.5 - 0.5 * c;
        const int e = ((k & 1) << 2) | (k & 2) | (k >> 2);
        v[e].re = w * yi; v[e].im = w * yq;
        // one output at a time, reads and arithmetic: the eight side by side (360 registers) would spill
        asm volatile("" : "+v"(v[e].re), "+v"(v[e].im));
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();                                              // the staging area is free

    // len = 2, 4, 8 in registers
#pragma unroll
    for (int len = 2; len <= 8; len <<= 1) {
        const int half = len >> 1;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if ((i & half) == 0) {
                const double2 w = tw[(i & (half - 1)) * (NVX_SCAN_FFT / len)];
                bfly(v[i], v[i + half], w.x, w.y);
            }
        }
    }
    const int blk = (int)(__builtin_bitreverse32((uint32_t)t) >> 24) * 8;
#pragma unroll
    for (int e = 0; e < 8; e++) { const int p = swz(blk + e); re[p] = v[e].re; im[p] = v[e].im; }
    __syncthreads();

    // len = 16 .. 2048: two levels per pass
#pragma unroll
    for (int pass = 0; pass < 4; pass++) {
        const int h = 8 << (2 * pass);
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int q = t + SCAN_THREADS * r;
            const int j = q & (h - 1), i0 = (q / h) * (4 * h) + j;
            Cx x[4];
            int p[4];
#pragma unroll
            for (int m = 0; m < 4; m++) { p[m] = swz(i0 + m * h); x[m].re = re[p[m]]; x[m].im = im[p[m]]; }
            const double2 w1 = tw[j * (NVX_SCAN_FFT / (2 * h))];
            bfly(x[0], x[1], w1.x, w1.y);
            bfly(x[2], x[3], w1.x, w1.y);
            const double2 w2a = tw[j * (NVX_SCAN_FFT / (4 * h))], w2b = tw[(j + h) * (NVX_SCAN_FFT / (4 * h))];
            bfly(x[0], x[2], w2a.x, w2a.y);
            bfly(x[1], x[3], w2b.x, w2b.y);
            if (h < 512) {
#pragma unroll
                for (int m = 0; m < 4; m++) { re[p[m]] = x[m].re; im[p[m]] = x[m].im; }
            } else {
                // x[m] is bin j + 512 m, j = t + 256 r: row index (bin + 1024) mod 2048 = t + 256 (r + 2 m + 4) mod 8
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const int o = (r + 2 * m + 4) & 7;
                    acc[o] = acc[o] + (x[m].re * x[m].re + x[m].im * x[m].im);
                }
            }
        }
        __syncthreads();
    }
}

// a frame's row: its nine slots in ascending order, from 0.0
__device__ __forceinline__ void scan_frame(const uint32_t *frame, int mode, uint32_t *xs, const double2 *tw, int t, double (&row)[8])
{
    const size_t slot_len = mode == NVX_SCAN_MODE_252K ? NVX_SCAN_SLOT_IN : NVX_SCAN_SLOT_RAW;
#pragma unroll
    for (int m = 0; m < 8; m++) row[m] = 0.0;
    for (int j = 0; j < 9; j++) scan_slot(frame + (size_t)j * slot_len, mode, xs, tw, t, row);
}

__device__ __forceinline__ void fill_twiddles(double2 *tw, int t)
{
    for (int j = t; j < 1024; j += SCAN_THREADS) tw[j] = make_double2(nvx_scan_tw.v[j][0], nvx_scan_tw.v[j][1]);
    __syncthreads();
}

__global__ __launch_bounds__(SCAN_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void nvx_scan_stream(nvx_scan_args a)
{
    __shared__ __attribute__((aligned(16))) uint32_t xs[SCAN_STAGE];
    __shared__ double2 tw[1024];
    const int t = threadIdx.x;
    fill_twiddles(tw, t);
    const size_t frame_len = a.mode == NVX_SCAN_MODE_252K ? NVX_SCAN_FRAME_IN : NVX_SCAN_FRAME_RAW;
    const uint32_t *in = a.iq + (size_t)blockIdx.x * a.pitch + a.first_frame * frame_len;
    double total[8];
#pragma unroll
    for (int m = 0; m < 8; m++) total[m] = 0.0;
    for (int f = 0; f < a.n_frames; f++) {
        double row[8];
        scan_frame(in + (size_t)f * frame_len, a.mode, xs, tw, t, row);
#pragma unroll
        for (int m = 0; m < 8; m++) total[m] = total[m] + row[m];
    }
    double *out = a.power + (size_t)blockIdx.x * NVX_SCAN_FFT;
#pragma unroll
    for (int m = 0; m < 8; m++) out[t + SCAN_THREADS * m] = total[m];
}

__global__ __launch_bounds__(SCAN_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void nvx_scan_frame(nvx_scan_args a)
{
    __shared__ __attribute__((aligned(16))) uint32_t xs[SCAN_STAGE];
    __shared__ double2 tw[1024];
    const int t = threadIdx.x;
    fill_twiddles(tw, t);
    const size_t frame_len = a.mode == NVX_SCAN_MODE_252K ? NVX_SCAN_FRAME_IN : NVX_SCAN_FRAME_RAW;
    const uint32_t *in = a.iq + (size_t)blockIdx.y * a.pitch + (a.first_frame + blockIdx.x) * frame_len;
    double row[8];
    scan_frame(in, a.mode, xs, tw, t, row);
    double *out = a.rows + ((size_t)blockIdx.y * a.n_frames + blockIdx.x) * NVX_SCAN_FFT;
#pragma unroll
    for (int m = 0; m < 8; m++) out[t + SCAN_THREADS * m] = row[m];
}

__global__ __launch_bounds__(SCAN_THREADS) void nvx_scan_fold(nvx_scan_args a)
{
    const int b = blockIdx.x * SCAN_THREADS + threadIdx.x;        // grid: (2048 / 256, n_streams)
    const double *rows = a.rows + (size_t)blockIdx.y * a.n_frames * NVX_SCAN_FFT + b;
    double total = 0.0;
    for (int f = 0; f < a.n_frames; f++) total = total + rows[(size_t)f * NVX_SCAN_FFT];
    a.power[(size_t)blockIdx.y * NVX_SCAN_FFT + b] = total;
}

hipError_t nvx_scan_launch(const nvx_scan_args *a, int form, hipStream_t s, dim3 *first_grid)
{
    const dim3 grid = form == 1 ? dim3(a->n_streams) : dim3(a->n_frames, a->n_streams);
    *first_grid = grid;
    if (form == 1) {
        hipLaunchKernelGGL(nvx_scan_stream, grid, dim3(SCAN_THREADS), 0, s, *a);
    } else {
        hipLaunchKernelGGL(nvx_scan_frame, grid, dim3(SCAN_THREADS), 0, s, *a);
        hipLaunchKernelGGL(nvx_scan_fold, dim3(NVX_SCAN_FFT / SCAN_THREADS, a->n_streams), dim3(SCAN_THREADS), 0, s, *a);
    }
    return hipGetLastError();
}
