// wanc_launch_args.cpp -- the multi-tap canceller's launch arithmetic (navtex_amd/wanc/nvx_wanc_plan.h) without a device: for a
// list of positions, call lengths, windows, tap counts and chunkings, nvx_wanc_fill_args' numbers against direct arithmetic in
// 128-bit integers.  The kernels' walk over chunks, tiles and the one or two parts of a tile is restated: every sample of the
// call lies in exactly one part of one tile of exactly one chunk; the block of every sample, counted from the call's first, is
// the pair's block and has a record and a weight record; the ring slot of the call's first block is the pair's; whole tiles
// (the ones loaded 16 bytes at a time) end inside the call; the halo in front of a tile is read from the row or from the
// carried words and nowhere else; the state row's parts lie side by side and fill it; and where out_vec is set every row of
// the output is 16-byte aligned.
// Built with -fsanitize=address,undefined by tests/test_wanc.py; no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvx_wanc_plan.h"

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

#define AT "consumed %llu, %zu samples, window_log2 %d, %d taps, %d chunks wanted"
#define ATV (unsigned long long)consumed, n_in, window_log2, K, wanted

static void check_case(uint64_t consumed, size_t n_in, int window_log2, int K, int wanted, int n_pairs, uintptr_t out_base, size_t pitch_out, size_t out_first,
                       bool walk = true)
{
    static int64_t state[2][8];
    static unsigned long long records[8], counters[4];
    static int32_t weights[8];
    static const char in[16] = { 0 }, in2[16] = { 0 };
    nvx_wanc_args a;
    const int chunks = nvx_wanc_fill_args(consumed, in, 12345, in2, 23456, n_in, (uint32_t *)out_base, pitch_out, out_first, n_pairs, state[0], state[1], records,
                                          weights, counters, window_log2, K, 13, wanted, &a);
    // what is handed through
    CHECK(a.in_main == in && a.pitch_main == 12345 && a.in_sense == in2 && a.pitch_sense == 23456 && a.out == (uint32_t *)out_base && a.pitch_out == pitch_out && a.out_first == out_first, AT ": operands", ATV);
    CHECK(a.state_in == state[0] && a.state_out == state[1] && a.records == records && a.weights == weights && a.counters == counters, AT ": state", ATV);
    CHECK((size_t)a.n_in == n_in && a.window_log2 == window_log2 && a.n_taps == K && a.load_log2 == 13 && a.n_pairs == n_pairs, AT ": numbers", ATV);
    // the state row: ring, partial sums, scalars, weights, sense words, main words, side by side
    const int W = 1 << window_log2, NS = NVX_WANC_SUMS(K);
    CHECK(NS == 4 * K + 1 && NVX_WANC_ST_SCALARS(K, window_log2) == NS * W + NS, AT ": sums", ATV);
    CHECK(NVX_WANC_ST_WEIGHTS(K, window_log2) == NVX_WANC_ST_SCALARS(K, window_log2) + NVX_WANC_STATE_SCALARS && NVX_WANC_SC_REASON < NVX_WANC_STATE_SCALARS, AT ": scalars", ATV);
    CHECK(NVX_WANC_ST_SENSE(K, window_log2) == NVX_WANC_ST_WEIGHTS(K, window_log2) + 2 * K && NVX_WANC_ST_MAIN(K, window_log2) == NVX_WANC_ST_SENSE(K, window_log2) + K - 1, AT ": words", ATV);
    CHECK(a.state_words == NVX_WANC_ST_MAIN(K, window_log2) + K / 2 && a.state_words == NS * (W + 1) + 8 + 2 * K + K - 1 + K / 2, AT ": %d state words", ATV, a.state_words);
    CHECK(NVX_WANC_WREC(K) >= 2 * K + 3 && NVX_WANC_PAD >= K - 1 && NVX_WANC_PAD % 4 == 0 && W <= 64 && 2 * K <= 64 && K / 2 <= 32, AT ": the kernels' shapes", ATV);

    // tiles and chunks
    CHECK((u128)a.tiles * NVX_WANC_TILE >= n_in && (u128)(a.tiles - 1) * NVX_WANC_TILE < n_in, AT ": %d tiles", ATV, a.tiles);
    CHECK(chunks >= 1 && chunks <= (wanted < 1 ? 1 : wanted) && a.tiles_per_chunk >= 1, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    CHECK((long)chunks * a.tiles_per_chunk >= a.tiles && (long)(chunks - 1) * a.tiles_per_chunk < a.tiles, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    if (chunks > 1) CHECK(a.tiles_per_chunk >= NVX_WANC_MIN_CHUNK_TILES && NVX_WANC_MIN_CHUNK_TILES * NVX_WANC_TILE >= 2 * NVX_WANC_BLOCK, AT ": a short chunk", ATV);
    if (wanted <= 1) CHECK(chunks == 1 && a.tiles_per_chunk == a.tiles, AT ": one chunk", ATV);
    CHECK(NVX_WANC_TILE < NVX_WANC_BLOCK && NVX_WANC_BLOCK % NVX_WANC_TILE == 0, "a tile holds at most one block end");

    // blocks, records and the ring
    const u128 block0 = (u128)consumed / NVX_WANC_BLOCK, last_block = ((u128)consumed + n_in - 1) / NVX_WANC_BLOCK;
    CHECK(a.off0 >= 0 && a.off0 < NVX_WANC_BLOCK && (u128)a.off0 == (u128)consumed % NVX_WANC_BLOCK, AT ": off0 %d", ATV, a.off0);
    CHECK((u128)a.blocks == last_block - block0 + 1, AT ": %d records", ATV, a.blocks);
    CHECK((u128)a.slot0 == block0 % W, AT ": slot0 %d", ATV, a.slot0);
    CHECK((u128)a.off0 + n_in < ((u128)1 << 31), AT ": the kernels count in int", ATV);
    CHECK((u128)65535 * a.blocks < ((u128)1 << 31), AT ": the solve kernel counts its lanes in int", ATV);

    // the kernels' walk (sample by sample, unless the call is too long for that)
    std::vector<uint8_t> reached(walk ? n_in : 0, 0);
    for (int x = 0; x < chunks; x++) {
        const int tile0 = x * a.tiles_per_chunk, tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
        CHECK(tile0 < tile1, AT ": chunk %d is empty", ATV, x);
        for (int tile = tile0; tile < tile1; tile++) {
            const bool full = (u128)(tile + 1) * NVX_WANC_TILE <= n_in;
            if (!full) CHECK(tile == a.tiles - 1, AT ": tile %d is not whole and not the last", ATV, tile);
            const int tbase = tile * NVX_WANC_TILE, boff = a.off0 + tbase;
            const int r = boff >> 16, n_a = NVX_WANC_BLOCK - (boff & (NVX_WANC_BLOCK - 1));
            const int hi = (int)n_in - tbase < NVX_WANC_TILE ? (int)n_in - tbase : NVX_WANC_TILE;
            const bool split = n_a < hi;
            CHECK(hi >= 1 && r >= 0 && r + (split ? 1 : 0) < a.blocks, AT ": tile %d touches record %d of %d", ATV, tile, r + (split ? 1 : 0), a.blocks);
            // the halo: samples tbase - PAD .. tbase - 1 of the row where they are not negative, the carried words K - 1 + s and
            // K / 2 + s for the K - 1 and K / 2 samples in front of the call, zeros further back
            for (int t = 0; t < NVX_WANC_PAD; t++) {
                const int s = tbase - NVX_WANC_PAD + t;
                if (s >= 0) CHECK((size_t)s < n_in, AT ": the halo reads sample %d", ATV, s);
                else if (s >= -(K - 1)) CHECK(K - 1 + s >= 0 && K - 1 + s < K - 1, AT ": the halo reads carried word %d", ATV, K - 1 + s);
            }
            for (int i = 0; i < K / 2; i++) {
                const int s = tbase - K / 2 + i;
                if (s >= 0) CHECK((size_t)s < n_in, AT ": the main halo reads sample %d", ATV, s);
                else CHECK(K / 2 + s >= 0 && K / 2 + s < K / 2, AT ": the main halo reads carried word %d", ATV, K / 2 + s);
            }
            for (int part = 0; part <= (int)split; part++) {
                const int lo = part ? n_a : 0, end = split && !part ? n_a : hi;
                CHECK(lo < end, AT ": tile %d part %d is empty", ATV, tile, part);
                for (int j = lo; walk && j < end; j++) {
                    reached[(size_t)tbase + j]++;
                    const u128 block = ((u128)consumed + tbase + j) / NVX_WANC_BLOCK;
                    CHECK(block - block0 == (u128)(r + part), AT ": sample %d lies in block %d of the call", ATV, tbase + j, r + part);
                }
            }
        }
    }
    for (size_t j = 0; walk && j < n_in; j++) CHECK(reached[j] == 1, AT ": sample %zu reached %d times", ATV, j, reached[j]);
    // the blocks that ended inside the call, as the state's writer counts them: the records it reads exist
    const int done = (a.off0 + (int)n_in) >> 16;
    CHECK((u128)done == ((u128)consumed + n_in) / NVX_WANC_BLOCK - block0, AT ": blocks done", ATV);
    CHECK(done - 1 < a.blocks && (((a.off0 + (int)n_in) & (NVX_WANC_BLOCK - 1)) == 0 || done < a.blocks), AT ": the state's writer reads record %d of %d", ATV, done, a.blocks);

    // 16-byte stores only where every row is 16-byte aligned
    bool aligned = true;
    for (int s = 0; s < n_pairs; s++) aligned = aligned && ((u128)out_base + ((u128)s * pitch_out + out_first) * 4) % 16 == 0;
    CHECK((a.out_vec != 0) == aligned, AT ": out_vec %d for base %#zx, pitch %zu, first %zu, %d pairs", ATV, a.out_vec, (size_t)out_base, pitch_out,
          out_first, n_pairs);
}

int main(void)
{
    const size_t T = NVX_WANC_TILE, B = NVX_WANC_BLOCK;
    const size_t lengths[] = { 1, 2, 3, 7, 15, 4095, 4096, 4097, B - 1, B, B + 1, 2 * B, 2 * B + 1, 31 * T + 5, 32 * T, 32 * T + 1, 5 * B + 13107 };
    const uint64_t positions[] = { 0, 1, 4095, 4096, B - 1, B, B + 1, 777, ((uint64_t)1 << 32) - 1000, ((uint64_t)1 << 40) + 5, ((uint64_t)1 << 62) - 1 - 40 * B };
    const int chunkings[] = { 0, 1, 2, 3, 683, 2048 };
    const int windows[] = { 2, 4, 6 };
    const int taps[] = { 4, 8, 16 };
    for (size_t n_in : lengths)
        for (uint64_t consumed : positions)
            for (int window_log2 : windows)
                for (int K : taps)
                    for (int wanted : chunkings) {
                        if ((window_log2 != 4 || K != 8) && wanted != 1) continue;      // the window and the taps move the state's layout and nothing else
                        CHECK(!((consumed + n_in) >> 62), "position %llu + %zu", (unsigned long long)consumed, n_in);
                        check_case(consumed, n_in, window_log2, K, wanted, 3, 0x7000000, 3000004, 8);
                    }
    // forty blocks spread over twenty chunks, and the longest call from the last offset of a block (not walked sample by sample)
    check_case(777, 40 * B, 2, 8, 2048, 1, 0x7000000, 0, 0);
    check_case(B - 1, NVX_WANC_MAX_IN, 4, 16, 2048, 1, 0x7000000, 0, 0, false);
    // the alignment of the output rows
    const struct { uintptr_t base; size_t pitch, first; int pairs; } OUTS[] = {
        { 0x7000000, 40020, 7, 2 }, { 0x7000000, 40020, 8, 2 }, { 0x7000000, 40021, 8, 2 }, { 0x7000000, 40021, 8, 1 }, { 0x7000004, 40020, 3, 2 },
        { 0x7000004, 40020, 0, 1 }, { 0x7000008, 40022, 2, 1 }, { 0x7000008, 40022, 2, 3 }, { 0x7000000, 0, 0, 1 },
    };
    for (const auto &o : OUTS) check_case(5, 40013, 4, 8, 1, o.pairs, o.base, o.pitch, o.first);
    printf("wanc launch args ok: %ld checks\n", g_checks);
    return 0;
}
