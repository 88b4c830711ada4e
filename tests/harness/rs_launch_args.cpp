// rs_launch_args.cpp -- the launch arithmetic of the polyphase plan (navtex_amd/resample/nvx_rs_host.h) without a device:
// for a list of plans, positions, output counts and chunkings, nvx_rs_fill_args' numbers against direct arithmetic in
// 128-bit integers.  The kernels' walk over chunks, tiles and threads is restated here step by step -- the two
// shift-and-subtract divisions as plain divisions with the bounds they rely on asserted -- and every output of the call must
// be reached exactly once, at input position (n0 + j) M div L - consumed and phase (n0 + j) M mod L, n0 = ceil(consumed L / M).
// The chunk split is nvx_stream_plan.h's with a shortest chunk of one tile: it is held against the plan's rule restated here.
// Built with -fsanitize=address,undefined by tests/test_resample.py; links the design (nvx_resample_design.c), no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvx_rs_host.h"

typedef unsigned __int128 u128;

static long g_checks = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        g_checks++;                                                             \
        if (!(cond)) {                                                          \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);          \
            fprintf(stderr, __VA_ARGS__);                                       \
            fprintf(stderr, "\n");                                              \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

struct where { uint32_t rate; unsigned long long consumed; size_t n_out; int wanted; };
#define AT "%u S/s, consumed %llu, %zu outputs, %d chunks wanted"
#define ATV(w) (w).rate, (w).consumed, (w).n_out, (w).wanted

// (steps * M) = q L + r with r < L
static void check_step(const where &w, const char *name, u128 steps, const nvx_rs_plan &p, uint32_t q, uint32_t r)
{
    const u128 pos = steps * (unsigned)p.M;
    CHECK((u128)q * (unsigned)p.L + r == pos && r < (uint32_t)p.L, AT ": step %s = (%u, %u)", ATV(w), name, q, r);
}

// The chunk split of the plan restated: at most a chunk per tile, equal shares, for no tiles one chunk of one tile.
// nvx_rs_fill_args gets it from nvx_stream_chunks(tiles, chunks, 1, ...).
static int split_in_equal_shares(int tiles, int chunks, int *tiles_per_chunk)
{
    if (chunks > tiles) chunks = tiles;
    *tiles_per_chunk = tiles ? (tiles + chunks - 1) / chunks : 1;
    return tiles ? (tiles + *tiles_per_chunk - 1) / *tiles_per_chunk : 1;
}

// nvx_stream_chunks with a shortest chunk of one tile is that split, for every chunks >= 1
static void check_split(void)
{
    static const int WANTED[] = { 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 64, 100, 255, 256, 257, 683, 1024, 2047, 2048, 2049, 65535, 1 << 20 };
    for (int tiles = 0; tiles <= 3000; tiles++)
        for (int wanted : WANTED) {
            int per_old, per_new;
            const int old_chunks = split_in_equal_shares(tiles, wanted, &per_old), new_chunks = nvx_stream_chunks(tiles, wanted, 1, &per_new);
            CHECK(old_chunks == new_chunks && per_old == per_new, "%d tiles, %d wanted: %d chunks of %d, nvx_stream_chunks %d of %d", tiles, wanted, old_chunks,
                  per_old, new_chunks, per_new);
        }
    for (int tiles = 0; tiles <= 300; tiles++)
        for (int wanted = 1; wanted <= 320; wanted++) {
            int per_old, per_new;
            const int old_chunks = split_in_equal_shares(tiles, wanted, &per_old), new_chunks = nvx_stream_chunks(tiles, wanted, 1, &per_new);
            CHECK(old_chunks == new_chunks && per_old == per_new, "%d tiles, %d wanted: %d chunks of %d, nvx_stream_chunks %d of %d", tiles, wanted, old_chunks,
                  per_old, new_chunks, per_new);
        }
}

static void check_case(const nvx_rs_plan &p, const where &w, uint64_t consumed, size_t n_in)
{
    const uint32_t L = (uint32_t)p.L;
    const size_t n_out = w.n_out;
    nvx_rs_args a;
    std::vector<uint32_t> out(1);
    const int chunks = nvx_rs_fill_args(p, 1, consumed, 1, out.data(), 12345, n_in, out.data(), 6789, 77, n_out, w.wanted, &a);

    // what is handed through
    CHECK(a.in == out.data() && a.out == out.data() && a.pitch_in == 12345 && a.pitch_out == 6789 && a.out_first == 77, AT ": operands", ATV(w));
    CHECK(a.hist_in == p.hist.d[1] + p.hist.words && a.hist_out == p.hist.d[0] + p.hist.words && a.taps == p.d_taps, AT ": history rows", ATV(w));
    CHECK((size_t)a.hist_pitch == p.hist.words && a.hist_valid == (consumed > 0) && (size_t)a.n_in == n_in && (size_t)a.n_out == n_out, AT ": counts", ATV(w));
    CHECK(a.L == p.L && a.M == p.M && a.T == p.T && a.Tp == p.Tp && a.row_dw == p.row_dw && a.tap_dw == p.tap_dw && a.K == p.K, AT ": plan", ATV(w));

    // tiles and chunks: every tile in exactly one chunk, no chunk empty, no more chunks than wanted
    const int tile_out = NVX_RS_THREADS * a.K;
    CHECK((size_t)a.tiles * tile_out >= n_out && (size_t)(a.tiles - 1) * tile_out < n_out, AT ": %d tiles", ATV(w), a.tiles);
    CHECK(chunks >= 1 && chunks <= w.wanted && a.tiles_per_chunk >= 1, AT ": %d chunks of %d tiles", ATV(w), chunks, a.tiles_per_chunk);
    CHECK((long)chunks * a.tiles_per_chunk >= a.tiles && (long)(chunks - 1) * a.tiles_per_chunk < a.tiles, AT ": %d chunks of %d tiles", ATV(w), chunks, a.tiles_per_chunk);
    if (w.wanted == 1) CHECK(chunks == 1 && a.tiles_per_chunk == a.tiles, AT ": one chunk", ATV(w));
    if (w.wanted >= a.tiles) CHECK(chunks == a.tiles && a.tiles_per_chunk == 1, AT ": a chunk per tile", ATV(w));
    int per;
    CHECK(chunks == split_in_equal_shares(a.tiles, w.wanted, &per) && a.tiles_per_chunk == per, AT ": %d chunks of %d tiles", ATV(w), chunks, a.tiles_per_chunk);

    // the steps, as (div L, mod L)
    check_step(w, "thread (m)", 1, p, a.m_div, a.m_mod);
    check_step(w, "256 outputs (d)", NVX_RS_THREADS, p, a.dq, a.dr);
    check_step(w, "tile", (u128)tile_out, p, a.tile_dq, a.tile_dr);
    check_step(w, "chunk", (u128)tile_out * a.tiles_per_chunk, p, a.chunk_dq, a.chunk_dr);
    check_step(w, "span", (u128)tile_out - 1, p, a.span_q, a.span_r);

    // the bounds of the kernel's divmod<12> (chunk starts) and divmod<8> (thread starts, from any tile start rt < L)
    CHECK((u128)a.r0 + (u128)(chunks - 1) * a.chunk_dr < ((u128)L << 12), AT ": r0 %u + %d chunk_dr %u", ATV(w), a.r0, chunks - 1, a.chunk_dr);
    CHECK((u128)(L - 1) + (u128)(NVX_RS_THREADS - 1) * a.m_mod < ((u128)L << 8), AT ": m_mod %u", ATV(w), a.m_mod);
    CHECK(a.r0 < L, AT ": r0 %u", ATV(w), a.r0);

    // output j of the call: position (n0 + j) M, as (div L - consumed, mod L)
    const u128 n0 = ((u128)consumed * L + (unsigned)p.M - 1) / (unsigned)p.M;
    auto q_of = [&](size_t j) { return (long long)((n0 + j) * (unsigned)p.M / L - consumed); };
    auto r_of = [&](size_t j) { return (uint32_t)((n0 + j) * (unsigned)p.M % L); };
    CHECK(q_of(0) >= 0 && a.qoff == q_of(0) && a.r0 == r_of(0), AT ": output 0 at (%d, %u)", ATV(w), a.qoff, a.r0);

    // the kernel's walk
    std::vector<uint8_t> reached(n_out, 0);
    for (int x = 0; x < chunks; x++) {
        const uint32_t v = a.r0 + (uint32_t)x * a.chunk_dr;
        uint32_t rt = v % L;
        int qt = a.qoff + (int)((uint32_t)x * a.chunk_dq + v / L);
        int q[NVX_RS_THREADS]; uint32_t r[NVX_RS_THREADS];
        for (int tid = 0; tid < NVX_RS_THREADS; tid++) {
            const uint32_t u = rt + (uint32_t)tid * a.m_mod;
            r[tid] = u % L;
            q[tid] = qt + (int)((uint32_t)tid * a.m_div + u / L);
        }
        const int tile0 = x * a.tiles_per_chunk, tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
        for (int tile = tile0; tile < tile1; tile++) {
            const size_t first = (size_t)tile * tile_out;
            const int tile_n = n_out - first < (size_t)tile_out ? (int)(n_out - first) : tile_out;
            CHECK(qt == q_of(first) && rt == r_of(first), AT ": tile %d starts at (%d, %u)", ATV(w), tile, qt, rt);
            // the last output of a full tile, and the span staged for it: fits the planes
            const int q_last = qt + (int)a.span_q + (rt + a.span_r >= L ? 1 : 0);
            CHECK(q_last == q_of(first + tile_out - 1), AT ": tile %d ends at %d", ATV(w), tile, q_last);
            const int lo = (qt - (p.T - 1)) & ~(NVX_RS_GROUP - 1), hi = (q_last + 2 * NVX_RS_GROUP - 1) & ~(NVX_RS_GROUP - 1);
            CHECK(hi - lo <= NVX_RS_PLANE, AT ": tile %d stages %d samples", ATV(w), tile, hi - lo);
            for (int k = 0; k < a.K; k++)
                for (int tid = 0; tid < NVX_RS_THREADS; tid++) {
                    const int jl = tid + k * NVX_RS_THREADS;
                    if (jl < tile_n) {
                        const size_t j = first + jl;
                        CHECK(q[tid] == q_of(j) && r[tid] == r_of(j), AT ": output %zu at (%d, %u)", ATV(w), j, q[tid], r[tid]);
                        // its window, from a multiple of 4 samples and Tp long, lies in the staged span
                        const int ws = q[tid] - (p.T - 1) - lo;
                        CHECK(ws >= 0 && (ws & ~(NVX_RS_ALIGN - 1)) + p.Tp <= hi - lo, AT ": output %zu's window leaves the staged span", ATV(w), j);
                        reached[j]++;
                    }
                    q[tid] += (int)a.dq; r[tid] += a.dr;
                    if (r[tid] >= L) { r[tid] -= L; q[tid]++; }
                }
            qt += (int)a.tile_dq; rt += a.tile_dr;
            if (rt >= L) { rt -= L; qt++; }
        }
    }
    for (size_t j = 0; j < n_out; j++) CHECK(reached[j] == 1, AT ": output %zu reached %d times", ATV(w), j, reached[j]);
}

int main(void)
{
    check_split();
    // taps in the LDS; L = 1008, taps in global memory; L = M = 1; the lowest rate (L > M); the largest LDS launch
    static const struct { uint32_t rate; bool taps_in_lds; } PLANS[] = { { 2048000, true }, { 1000250, false }, { 252000, true }, { 96000, true }, { 100100, true } };
    for (const auto &pl : PLANS) {
        nvx_rs_plan p("the harness", "row");
        int L, M, T;
        const char *why = "";
        CHECK(nvx_rs_plan_numbers(pl.rate, &L, &M, &T, &why) == NVX_OK, "%u S/s: %s", pl.rate, why);
        CHECK(nvx_rs_plan_shape(p, L, M, T), "%u S/s: a tile does not fit", pl.rate);
        CHECK(p.taps_in_lds == pl.taps_in_lds && p.K >= 1 && p.K <= NVX_RS_MAX_K, "%u S/s: tap table of %d bytes, K %d", pl.rate, p.tap_dw * 4, p.K);
        if (pl.rate == 1000250) CHECK(L == 1008, "L %d", L);
        if (pl.rate == 252000) CHECK(L == 1 && M == 1, "L %d M %d", L, M);
        p.n_inputs = 2;
        std::vector<uint32_t> hist(2 * 2 * p.hist.words + 1), taps(1);
        p.hist.d[0] = hist.data(); p.hist.d[1] = hist.data() + 2 * p.hist.words; p.d_taps = taps.data();

        const size_t tile = (size_t)NVX_RS_THREADS * p.K;
        const size_t n_outs[] = { 1, tile - 1, tile, tile + 1, 5 * tile };
        for (size_t n_out : n_outs) {
            const size_t n_in = (size_t)(((u128)n_out * (unsigned)M + L - 1) / (unsigned)L);      // samples that give about n_out outputs
            const uint64_t positions[] = { 0, 1, (uint64_t)M - 1, ((uint64_t)1 << 62) - 1 - n_in };
            const int tiles = (int)((n_out + tile - 1) / tile);
            const int wanted[] = { 1, 2, tiles };
            for (uint64_t consumed : positions)
                for (int chunks : wanted) {
                    const where w = { pl.rate, (unsigned long long)consumed, n_out, chunks };
                    CHECK(!((consumed + n_in) >> 62), AT ": position", ATV(w));
                    check_case(p, w, consumed, n_in);
                }
        }
        printf("%u S/s: L %d M %d T %d K %d, taps %s\n", pl.rate, L, M, T, p.K, p.taps_in_lds ? "in the LDS" : "in global memory");
    }
    printf("rs launch args ok: %ld checks\n", g_checks);
    return 0;
}
