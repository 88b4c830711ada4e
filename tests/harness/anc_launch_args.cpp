// anc_launch_args.cpp -- the noise canceller's launch arithmetic (navtex_amd/anc/nvx_anc_plan.h) without a device: for a list of
// positions, call lengths, windows and chunkings, nvx_anc_fill_args' numbers against direct arithmetic in 128-bit integers.
// The kernels' walk over chunks and tiles is restated: every sample of the call lies in exactly one tile of exactly one
// chunk; a tile holds at most one block end, where the kernels compute it; the block of every sample, counted from the
// call's first, is the pair's block and has a record; the ring slot of the call's first block is the pair's; whole
// tiles (the ones read and written 16 bytes at a time) end inside the call; and where out_vec is set every row of the
// output is 16-byte aligned.
// Built with -fsanitize=address,undefined by tests/test_anc.py; no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvx_anc_plan.h"

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

#define AT "consumed %llu, %zu samples, window_log2 %d, %d chunks wanted"
#define ATV (unsigned long long)consumed, n_in, window_log2, wanted

static void check_case(uint64_t consumed, size_t n_in, int window_log2, int wanted, int n_pairs, uintptr_t out_base, size_t pitch_out, size_t out_first,
                       bool walk = true)
{
    static int64_t state[2][400];
    static unsigned long long records[8], counters[4];
    static const char in[16] = { 0 }, in2[16] = { 0 };
    nvx_anc_args a;
    const int chunks = nvx_anc_fill_args(consumed, in, 12345, in2, 23456, n_in, (uint32_t *)out_base, pitch_out, out_first, n_pairs, state[0], state[1], records, counters,
                                         window_log2, wanted, &a);
    // what is handed through
    CHECK(a.in_main == in && a.pitch_main == 12345 && a.in_sense == in2 && a.pitch_sense == 23456 && a.out == (uint32_t *)out_base && a.pitch_out == pitch_out && a.out_first == out_first, AT ": operands", ATV);
    CHECK(a.state_in == state[0] && a.state_out == state[1] && a.records == records && a.counters == counters, AT ": state", ATV);
    CHECK((size_t)a.n_in == n_in && a.window_log2 == window_log2, AT ": numbers", ATV);
    const int W = 1 << window_log2;
    CHECK(a.state_words == 4 * W + 4 + 8 && a.state_words <= 400, AT ": %d state words", ATV, a.state_words);

    // tiles and chunks
    CHECK((u128)a.tiles * NVX_ANC_TILE >= n_in && (u128)(a.tiles - 1) * NVX_ANC_TILE < n_in, AT ": %d tiles", ATV, a.tiles);
    CHECK(chunks >= 1 && chunks <= (wanted < 1 ? 1 : wanted) && a.tiles_per_chunk >= 1, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    CHECK((long)chunks * a.tiles_per_chunk >= a.tiles && (long)(chunks - 1) * a.tiles_per_chunk < a.tiles, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    if (chunks > 1) CHECK(a.tiles_per_chunk >= NVX_ANC_MIN_CHUNK_TILES && NVX_ANC_MIN_CHUNK_TILES * NVX_ANC_TILE >= 2 * NVX_ANC_BLOCK, AT ": a short chunk", ATV);
    if (wanted <= 1) CHECK(chunks == 1 && a.tiles_per_chunk == a.tiles, AT ": one chunk", ATV);
    CHECK(NVX_ANC_TILE < NVX_ANC_BLOCK && NVX_ANC_BLOCK % NVX_ANC_TILE == 0, "a tile holds at most one block end");

    // blocks, records and the ring
    const u128 block0 = (u128)consumed / NVX_ANC_BLOCK, last_block = ((u128)consumed + n_in - 1) / NVX_ANC_BLOCK;
    CHECK(a.off0 >= 0 && a.off0 < NVX_ANC_BLOCK && (u128)a.off0 == (u128)consumed % NVX_ANC_BLOCK, AT ": off0 %d", ATV, a.off0);
    CHECK((u128)a.blocks == last_block - block0 + 1, AT ": %d records", ATV, a.blocks);
    CHECK((u128)a.slot0 == block0 % W, AT ": slot0 %d", ATV, a.slot0);
    CHECK((u128)a.off0 + n_in < ((u128)1 << 31), AT ": the kernels count in int", ATV);

    // the kernels' walk (sample by sample, unless the call is too long for that)
    std::vector<uint8_t> reached(walk ? n_in : 0, 0);
    for (int x = 0; x < chunks; x++) {
        const int tile0 = x * a.tiles_per_chunk, tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
        CHECK(tile0 < tile1, AT ": chunk %d is empty", ATV, x);
        for (int tile = tile0; tile < tile1; tile++) {
            const bool full = (u128)(tile + 1) * NVX_ANC_TILE <= n_in;
            if (!full) CHECK(tile == a.tiles - 1, AT ": tile %d is not whole and not the last", ATV, tile);
            const int tbase = tile * NVX_ANC_TILE, boff = a.off0 + tbase;
            const int r = boff >> 16;
            int n_a = NVX_ANC_BLOCK - (boff & (NVX_ANC_BLOCK - 1));
            const bool split = n_a < NVX_ANC_TILE && (size_t)tbase + n_a < n_in;
            if (!split) n_a = NVX_ANC_TILE;
            CHECK(r >= 0 && r + (split ? 1 : 0) < a.blocks, AT ": tile %d touches record %d of %d", ATV, tile, r + (split ? 1 : 0), a.blocks);
            const size_t first = (size_t)tbase;
            for (size_t j = first; walk && j < first + NVX_ANC_TILE && j < n_in; j++) {
                reached[j]++;
                const u128 block = ((u128)consumed + j) / NVX_ANC_BLOCK;
                const int rel = r + ((int)(j - first) < n_a ? 0 : 1);
                CHECK(block - block0 == (u128)rel, AT ": sample %zu lies in block %d of the call", ATV, j, rel);
            }
        }
    }
    for (size_t j = 0; walk && j < n_in; j++) CHECK(reached[j] == 1, AT ": sample %zu reached %d times", ATV, j, reached[j]);
    // the blocks that end inside the call, as the state's writer counts them
    CHECK((u128)((a.off0 + (int)n_in) >> 16) == ((u128)consumed + n_in) / NVX_ANC_BLOCK - block0, AT ": blocks done", ATV);

    // 16-byte stores only where every row is 16-byte aligned
    bool aligned = true;
    for (int s = 0; s < n_pairs; s++) aligned = aligned && ((u128)out_base + ((u128)s * pitch_out + out_first) * 4) % 16 == 0;
    CHECK((a.out_vec != 0) == aligned, AT ": out_vec %d for base %#zx, pitch %zu, first %zu, %d pairs", ATV, a.out_vec, (size_t)out_base, pitch_out,
          out_first, n_pairs);
}

int main(void)
{
    const size_t T = NVX_ANC_TILE, K = NVX_ANC_BLOCK;
    const size_t lengths[] = { 1, 4095, 4096, 4097, K - 1, K, K + 1, 2 * K, 2 * K + 1, 31 * T + 5, 32 * T, 32 * T + 1, 5 * K + 13107 };
    const uint64_t positions[] = { 0, 1, 4095, 4096, K - 1, K, K + 1, 777, ((uint64_t)1 << 32) - 1000, ((uint64_t)1 << 40) + 5, ((uint64_t)1 << 62) - 1 - 40 * K };
    const int chunkings[] = { 0, 1, 2, 3, 683, 2048 };
    const int windows[] = { 2, 4, 6 };
    for (size_t n_in : lengths)
        for (uint64_t consumed : positions)
            for (int window_log2 : windows)
                for (int wanted : chunkings) {
                    if (window_log2 != 4 && wanted != 1) continue;             // the window moves the ring slot and nothing else
                    CHECK(!((consumed + n_in) >> 62), "position %llu + %zu", (unsigned long long)consumed, n_in);
                    check_case(consumed, n_in, window_log2, wanted, 3, 0x7000000, 3000004, 8);
                }
    // forty blocks spread over twenty chunks, and the longest call from the last offset of a block (not walked sample by sample)
    check_case(777, 40 * K, 2, 2048, 1, 0x7000000, 0, 0);
    check_case(K - 1, NVX_ANC_MAX_IN, 4, 2048, 1, 0x7000000, 0, 0, false);
    // the alignment of the output rows
    const struct { uintptr_t base; size_t pitch, first; int pairs; } OUTS[] = {
        { 0x7000000, 40020, 7, 2 }, { 0x7000000, 40020, 8, 2 }, { 0x7000000, 40021, 8, 2 }, { 0x7000000, 40021, 8, 1 }, { 0x7000004, 40020, 3, 2 },
        { 0x7000004, 40020, 0, 1 }, { 0x7000008, 40022, 2, 1 }, { 0x7000008, 40022, 2, 3 }, { 0x7000000, 0, 0, 1 },
    };
    for (const auto &o : OUTS) check_case(5, 40013, 4, 1, o.pairs, o.base, o.pitch, o.first);
    printf("anc launch args ok: %ld checks\n", g_checks);
    return 0;
}
