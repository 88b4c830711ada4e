// nvx_spec.hip -- the spectrum monitor's kernels (include/navtex_amd_spec.h states the arithmetic; this file only arranges it).
//
//   nvx_spec_line<FMT, L>   one workgroup of T = N / 4 threads per (line, row), N = 2^L.  Per segment of the line:
//       stage   a thread takes the SPT = 4 (8-bit formats: 8) consecutive samples of one 16-byte load (CF32: two) -- a
//               non-temporal load from the call's input where the group lies in it and is aligned there, sample by sample from
//               the ring and the input otherwise (a call that does not start on a multiple of SPT, or the group that straddles
//               the call's first sample) --, converts them, applies the window and puts them in bit-reversed order into the
//               LDS (re[] and im[] apart).
//       FFT     the stages run as passes of two radix-2 levels each (a thread holds x[i0 + {0, h, 2h, 3h}]; h = 1, 4, 16, ..
//               for even L; for odd L a pass of the one level len = 2 goes in front and h = 2, 8, 32, ..), the arithmetic of
//               every butterfly exactly the header's.  The last pass has h = T: thread t ends with bins t + T m, m = 0 .. 3,
//               in registers, for every segment the same four.  It writes nothing back.
//       sums    the powers and the lag products with the segment before, whose four bins the thread kept, go to the thread's
//               sums: P_line and C_line never leave the registers until the line is done.
//     Then the level words go through the LDS (the transform's area is dead by then) so that they leave in 16-byte
//     non-temporal stores, and P_line, C_line.re and C_line.im go to the line's scratch row, in the order of an output line.
//   LDS index swizzle: position i lives at i ^ rev5((i >> SH) & 31) with SH = max(5, L - 5): the bit-reversed staging stores,
//   whose lanes vary the top bits of i, then spread over the banks like lanes that vary bits 0 .. 4.
//   The twiddles (cos, -sin)[N / 2] are a second LDS table, filled once per workgroup from the 4096-point table at stride
//   4096 / N.  LDS: 24 N bytes -- 96 KB at N = 4096 (one workgroup of 16 waves per CU), 48 KB at 2048 (three), 6 KB at 256.
//   nvx_spec_fold            one thread per (bin, row): the survey's three sums over the launch's scratch rows, ascending,
//       from the survey as it stood (or 0.0 where it starts anew); the line count beside them.
//   nvx_spec_carry<FMT>      the samples behind the call's last complete line, converted, into the row's ring.
// No fp64 fused multiply-add (the build's -ffp-contract=off), no atomics: the sums' order is fixed.
// The formats' sizes, load_words, load_sample and the CF32 rule are the resampler's (nvx_rs_device.h); the lane's group and
// the dispatch on the format are the same-rate companions' (nvx_stream_device.h).
#include "nvx_spec_plan.h"
#include "nvx_spec_table.h"
#include "nvx_stream_device.h"

static_assert(NVX_SPEC_CS16 == NVX_RS_CS16 && NVX_SPEC_CU8 == NVX_RS_CU8 && NVX_SPEC_CS8 == NVX_RS_CS8 && NVX_SPEC_CF32 == NVX_RS_CF32, "formats");

// The full table, built from the octant at compile time: tw[j] = (C[j], -S[j]), j = 0 .. 2047, of the 4096-point turn
struct SpecTwiddles {
    double v[NVX_SPEC_TAB_N / 2][2];
    constexpr SpecTwiddles() : v{}
    {
        for (int j = 0; j < NVX_SPEC_TAB_N / 2; j++) { v[j][0] = nvx_spec_cs(j, 0); v[j][1] = -nvx_spec_cs(j, 1); }
    }
};
__device__ const SpecTwiddles nvx_spec_tw = SpecTwiddles();

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

struct Cx { double re, im; };
// the header's butterfly: t = b * (wr, wi); a, b <- a + t, a - t
__device__ __forceinline__ void bfly(Cx &a, Cx &b, double wr, double wi)
{
    const double tr = b.re * wr - b.im * wi;
    const double ti = b.re * wi + b.im * wr;
    b.re = a.re - tr; b.im = a.im - ti;
    a.re = a.re + tr; a.im = a.im + ti;
}

template <int L> __device__ __forceinline__ int swz(int i)
{
    constexpr int SH = L - 5 > 5 ? L - 5 : 5;
    return i ^ (int)(__builtin_bitreverse32((uint32_t)(i >> SH) & 31u) >> 27);
}

// the level word of a line's power
__device__ __forceinline__ uint32_t level_word(double p)
{
    const long long v = (long long)(__builtin_bit_cast(unsigned long long, p) >> 44) - NVX_SPEC_LEVEL_ZERO;
    return (uint32_t)(v < 0 ? 0 : (v > 65535 ? 65535 : v));
}

template <int FMT, int L>
__global__ __launch_bounds__((1 << L) / 4) void nvx_spec_line(const nvx_spec_args a)
{
    constexpr int N = 1 << L, H = N / 2, T = N / 4, SPT = StreamLane<FMT>::SPT;
    __shared__ __attribute__((aligned(16))) double re[N];
    __shared__ __attribute__((aligned(16))) double im[N];
    __shared__ double2 tw[H];
    int t = threadIdx.x;
    const int row = blockIdx.y, line = a.line0 + (int)blockIdx.x;
    for (int j = t; j < H; j += T) tw[j] = make_double2(nvx_spec_tw.v[j * (NVX_SPEC_TAB_N / N)][0], nvx_spec_tw.v[j * (NVX_SPEC_TAB_N / N)][1]);
    __syncthreads();

    const char *const src = (const char *)a.in + (size_t)row * a.pitch_in * Fmt<FMT>::BPS;
    const uint32_t *const ring = a.ring + (size_t)row * a.ring_words;
    const int A = a.avg;
    const int g_line = line * (A * H) - a.carried;                  // the line's first sample, counted from the call's first

    double P[4], Cr[4], Ci[4];
    Cx prev[4];
#pragma unroll
    for (int m = 0; m < 4; m++) { P[m] = 0.0; Cr[m] = 0.0; Ci[m] = 0.0; prev[m].re = 0.0; prev[m].im = 0.0; }

    for (int s = 0; s < A; s++) {
        // every address below derives from t: opaque per segment, so that the compiler computes them where they are used -- as
        // invariants of the segment loop they are dozens of registers, which it would hoist and, at 1024 threads, spill
        asm volatile("" : "+v"(t));
        // stage: the group of SPT samples from sample n0 of the segment
        if (t < N / SPT) {
            const int n0 = t * SPT, g0 = g_line + s * H + n0;
            uint32_t w[SPT];
            if (g0 >= 0 && (g0 & (SPT - 1)) == 0) load_words<FMT, true>(src, g0, w);
            else {
#pragma unroll
                for (int k = 0; k < SPT; k++) {
                    const int g = g0 + k;
                    if (g >= 0) w[k] = load_sample<FMT>(src, g);
                    else {
                        uint32_t at = a.ring0 + (uint32_t)(a.carried + g);
                        if (at >= (uint32_t)a.span) at -= (uint32_t)a.span;
                        w[k] = ring[at];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < SPT; k++) {
                const int n = n0 + k;
                const double c = n < H ? tw[n].x : -tw[n - H].x;   // C_N[n]: half a turn is a sign flip
                const double wn = 0.5 - 0.5 * c;
                const int p = swz<L>((int)(__builtin_bitreverse32((uint32_t)n) >> (32 - L)));
                re[p] = wn * (double)(int)(int16_t)(w[k] & 0xffffu);
                im[p] = wn * (double)((int)w[k] >> 16);
            }
        }
        __syncthreads();

        if (L & 1) {
            // len = 2 alone: butterflies t and t + T
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const int i0 = 2 * (t + T * r), p0 = swz<L>(i0), p1 = swz<L>(i0 + 1);
                Cx x0 = { re[p0], im[p0] }, x1 = { re[p1], im[p1] };
                const double2 w0 = tw[0];
                bfly(x0, x1, w0.x, w0.y);
                re[p0] = x0.re; im[p0] = x0.im; re[p1] = x1.re; im[p1] = x1.im;
            }
            __syncthreads();
        }
        Cx x[4];
#pragma unroll
        for (int h = (L & 1) ? 2 : 1; h <= T; h <<= 2) {
            const int j = t & (h - 1), i0 = (t / h) * (4 * h) + j;
            int p[4];
#pragma unroll
            for (int m = 0; m < 4; m++) { p[m] = swz<L>(i0 + m * h); x[m].re = re[p[m]]; x[m].im = im[p[m]]; }
            const double2 w1 = tw[j * (N / (2 * h))];
            bfly(x[0], x[1], w1.x, w1.y);
            bfly(x[2], x[3], w1.x, w1.y);
            const double2 w2a = tw[j * (N / (4 * h))], w2b = tw[(j + h) * (N / (4 * h))];
            bfly(x[0], x[2], w2a.x, w2a.y);
            bfly(x[1], x[3], w2b.x, w2b.y);
            if (h < T) {
#pragma unroll
                for (int m = 0; m < 4; m++) { re[p[m]] = x[m].re; im[p[m]] = x[m].im; }
            }
            __syncthreads();                                        // the last one: the area is free for the next segment
        }
        // x[m] is bin t + T m of the segment
#pragma unroll
        for (int m = 0; m < 4; m++) {
            P[m] = P[m] + (x[m].re * x[m].re + x[m].im * x[m].im);
            if (s > 0) {
                Cr[m] = Cr[m] + (x[m].re * prev[m].re + x[m].im * prev[m].im);
                Ci[m] = Ci[m] + (x[m].im * prev[m].re - x[m].re * prev[m].im);
            }
            prev[m] = x[m];
        }
    }

    // bin t + T m is index t + T ((m + 2) mod 4) of the line
    double *const out = a.scratch + ((size_t)row * a.batch_lines + blockIdx.x) * NVX_SPEC_SURVEY_WORDS(N);
    unsigned short *const lv = (unsigned short *)re;
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const int i = t + T * ((m + 2) & 3);
        out[i] = P[m]; out[N + i] = Cr[m]; out[2 * N + i] = Ci[m];
        lv[i] = (unsigned short)level_word(P[m]);
    }
    if (a.levels) {                                                 // uniform
        __syncthreads();
        u16x8 *const dst = (u16x8 *)(a.levels + ((size_t)row * a.line_cap + (size_t)line) * N);
        if (t < N / 8) __builtin_nontemporal_store(((const u16x8 *)lv)[t], dst + t);
    }
}

__global__ __launch_bounds__(NVX_SPEC_FOLD_THREADS) void nvx_spec_fold(const nvx_spec_args a)
{
    const int N = 1 << a.n_log2, row = blockIdx.y;
    const int b = blockIdx.x * NVX_SPEC_FOLD_THREADS + threadIdx.x;           // grid: (3 N / 256, n_rows): SP, SC.re, SC.im in turn
    const uint32_t *const cfg = a.cfg + (size_t)row * NVX_SPEC_CFG_WORDS;
    const bool anew = (cfg[0] & NVX_SPEC_ROW_RESTART) && a.line0 == 0;
    const int skip = (int)cfg[1];                                   // lines of the call that begin in front of the restart
    const int first = skip > a.line0 ? skip - a.line0 : 0;
    double *const sv = a.survey + (size_t)row * NVX_SPEC_SURVEY_WORDS(N) + b;
    const double *const rows = a.scratch + (size_t)row * a.batch_lines * NVX_SPEC_SURVEY_WORDS(N) + b;
    double total = anew ? 0.0 : *sv;
    for (int l = first; l < a.batch_lines; l++) total = total + rows[(size_t)l * NVX_SPEC_SURVEY_WORDS(N)];
    *sv = total;
    if (b == 0) {
        const unsigned long long had = anew ? 0ull : a.count[row];
        a.count[row] = had + (unsigned long long)(first < a.batch_lines ? a.batch_lines - first : 0);
    }
}

template <int FMT>
__global__ __launch_bounds__(NVX_SPEC_CARRY_THREADS) void nvx_spec_carry(const nvx_spec_args a)
{
    const int row = blockIdx.y;
    const char *const src = (const char *)a.in + (size_t)row * a.pitch_in * Fmt<FMT>::BPS;
    uint32_t *const ring = a.ring + (size_t)row * a.ring_words;
    const int n = a.n_in - a.keep_first;                            // below span
    for (int j = (int)(blockIdx.x * NVX_SPEC_CARRY_THREADS + threadIdx.x); j < n; j += (int)(gridDim.x * NVX_SPEC_CARRY_THREADS)) {
        uint32_t at = a.keep_ring + (uint32_t)j;
        if (at >= (uint32_t)a.span) at -= (uint32_t)a.span;
        ring[at] = load_sample<FMT>(src, a.keep_first + j);
    }
}

template <int FMT, int L>
static hipError_t launch_line(const nvx_spec_args *a, hipStream_t s)
{
    hipLaunchKernelGGL((nvx_spec_line<FMT, L>), dim3((unsigned)a->batch_lines, (unsigned)a->n_rows), dim3((1u << L) / 4), 0, s, *a);
    return hipGetLastError();
}

hipError_t nvx_spec_launch_lines(const nvx_spec_args *a, int format, hipStream_t s)
{
    hipError_t e = nvx_for_format(format, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        switch (a->n_log2) {
        case 8:  return launch_line<FMT, 8>(a, s);
        case 9:  return launch_line<FMT, 9>(a, s);
        case 10: return launch_line<FMT, 10>(a, s);
        case 11: return launch_line<FMT, 11>(a, s);
        case 12: return launch_line<FMT, 12>(a, s);
        }
        return hipErrorInvalidValue;
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nvx_spec_fold, dim3((unsigned)(3 << a->n_log2) / NVX_SPEC_FOLD_THREADS, (unsigned)a->n_rows), dim3(NVX_SPEC_FOLD_THREADS), 0, s, *a);
    return hipGetLastError();
}

hipError_t nvx_spec_launch_carry(const nvx_spec_args *a, int format, hipStream_t s)
{
    const int n = a->n_in - a->keep_first;
    if (n <= 0) return hipSuccess;
    const unsigned chunks = (unsigned)((n + 4 * NVX_SPEC_CARRY_THREADS - 1) / (4 * NVX_SPEC_CARRY_THREADS));
    return nvx_for_format(format, [&](auto fmt) {
        hipLaunchKernelGGL((nvx_spec_carry<decltype(fmt)::value>), dim3(chunks, (unsigned)a->n_rows), dim3(NVX_SPEC_CARRY_THREADS), 0, s, *a);
        return hipGetLastError();
    });
}
