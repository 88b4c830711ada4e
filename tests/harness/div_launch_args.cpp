// div_launch_args.cpp -- the diversity combiner's launch arithmetic (navtex_amd/div/nvx_div_plan.h) without a device: for a
// list of positions, call lengths, windows and chunkings, nvx_div_fill_args' numbers against direct arithmetic in 128-bit
// integers.  The kernels' walk over chunks, tiles and steps is restated: every sample of the call lies in exactly one tile of
// exactly one chunk; the block of every sample, counted from the call's first, is the pair's block and has a record; a tile
// holds at most one cell end, where the apply kernel computes it, and the cell of every sample has an entry in the weight
// list; the blocks and cells that end inside the call are the pair's; whole tiles (the ones read and written 16 bytes at a
// time) end inside the call; and where out_vec is set every row of the output is 16-byte aligned.
// Built with -fsanitize=address,undefined by tests/test_div.py; no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvx_div_plan.h"

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

static void check_case(uint64_t consumed, size_t n_in, int window_log2, int wanted, int n_pairs, int n_targets, uintptr_t out_base, size_t pitch_out,
                       size_t out_first, bool walk = true)
{
    static int64_t state[2][400];
    static unsigned long long records[8], counters[4];
    static uint32_t cfg[64], table[4];
    static nvx_div_weight weights[4];
    static const char in[16] = { 0 }, in2[16] = { 0 };
    nvx_div_args a;
    const int chunks = nvx_div_fill_args(consumed, in, 12345, in2, 23456, n_in, (uint32_t *)out_base, pitch_out, out_first, n_pairs, n_targets, state[0], state[1],
                                         cfg, table, records, weights, counters, window_log2, wanted, &a);
    // what is handed through
    CHECK(a.in_main == in && a.pitch_main == 12345 && a.in_second == in2 && a.pitch_second == 23456 && a.out == (uint32_t *)out_base && a.pitch_out == pitch_out && a.out_first == out_first, AT ": operands", ATV);
    CHECK(a.state_in == state[0] && a.state_out == state[1] && a.cfg == cfg && a.table == table && a.records == records && a.weights == weights && a.counters == counters, AT ": state", ATV);
    CHECK((size_t)a.n_in == n_in && a.window_log2 == window_log2 && a.n_pairs == n_pairs && a.n_targets == n_targets, AT ": numbers", ATV);
    CHECK((uint64_t)a.position == consumed && a.in_lo == (uint32_t)(consumed & 0xffffffffu), AT ": position", ATV);
    const int W = 1 << window_log2;
    CHECK(a.state_words == 4 * W + 8 + 8 && a.state_words * n_targets <= 400 && a.cfg_words == 2 + 6 * n_targets && a.cfg_words <= 64, AT ": %d state words", ATV, a.state_words);

    // tiles and chunks
    CHECK((u128)a.tiles * NVX_DIV_TILE >= n_in && (u128)(a.tiles - 1) * NVX_DIV_TILE < n_in, AT ": %d tiles", ATV, a.tiles);
    CHECK(chunks >= 1 && chunks <= (wanted < 1 ? 1 : wanted) && a.tiles_per_chunk >= 1, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    CHECK((long)chunks * a.tiles_per_chunk >= a.tiles && (long)(chunks - 1) * a.tiles_per_chunk < a.tiles, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    if (chunks > 1) CHECK(a.tiles_per_chunk >= NVX_DIV_MIN_CHUNK_TILES, AT ": a short chunk", ATV);
    if (wanted <= 1) CHECK(chunks == 1 && a.tiles_per_chunk == a.tiles, AT ": one chunk", ATV);
    CHECK(NVX_DIV_TILE < NVX_DIV_CELL && NVX_DIV_CELL % NVX_DIV_TILE == 0 && NVX_DIV_TILE % NVX_DIV_BLOCK == 0, "a tile holds at most one cell end");

    // blocks, cells, records and weights
    const u128 block0 = (u128)consumed / NVX_DIV_BLOCK, last_block = ((u128)consumed + n_in - 1) / NVX_DIV_BLOCK;
    const u128 cell0 = (u128)consumed / NVX_DIV_CELL, last_cell = ((u128)consumed + n_in - 1) / NVX_DIV_CELL;
    CHECK(a.off0 >= 0 && a.off0 < NVX_DIV_BLOCK && (u128)a.off0 == (u128)consumed % NVX_DIV_BLOCK, AT ": off0 %d", ATV, a.off0);
    CHECK(a.cell_off >= 0 && a.cell_off < NVX_DIV_CELL && (u128)a.cell_off == (u128)consumed % NVX_DIV_CELL, AT ": cell_off %d", ATV, a.cell_off);
    CHECK((u128)a.blocks == last_block - block0 + 1 && (u128)a.cells == last_cell - cell0 + 1, AT ": %d records, %d weights", ATV, a.blocks, a.cells);
    CHECK((u128)a.done == ((u128)consumed + n_in) / NVX_DIV_BLOCK - block0, AT ": %d blocks done", ATV, a.done);
    CHECK((u128)a.cells_done == ((u128)consumed + n_in) / NVX_DIV_CELL - cell0, AT ": %d cells done", ATV, a.cells_done);
    CHECK(a.done <= a.blocks && a.done >= a.blocks - 1 && a.cells_done <= a.cells && a.cells_done >= a.cells - 1, AT ": one open block and cell at most", ATV);
    CHECK((u128)a.cell_off + n_in < ((u128)1 << 31), AT ": the kernels count in int", ATV);
    // the fold kernel's blocks of a cell: [jlo, jhi) of the call's records
    for (int jc = 0; jc < a.cells; jc++) {
        const __int128 c = (__int128)cell0 + jc;
        __int128 jlo = c * 256 - (__int128)block0, jhi = (c + 1) * 256 - (__int128)block0;
        if (jlo < 0) jlo = 0;
        if (jhi > a.done) jhi = a.done;
        CHECK(jlo <= jhi || jc == a.cells - 1, AT ": cell %d has blocks %d .. %d", ATV, jc, (int)jlo, (int)jhi);
        for (__int128 j = jlo; walk && j < jhi; j++) CHECK(((__int128)block0 + j) / 256 == c && j < a.blocks, AT ": block %d of cell %d", ATV, (int)j, jc);
    }

    // the kernels' walk (sample by sample, unless the call is too long for that)
    std::vector<uint8_t> reached(walk ? n_in : 0, 0);
    for (int x = 0; x < chunks; x++) {
        const int tile0 = x * a.tiles_per_chunk, tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
        CHECK(tile0 < tile1, AT ": chunk %d is empty", ATV, x);
        for (int tile = tile0; tile < tile1; tile++) {
            const bool full = (u128)(tile + 1) * NVX_DIV_TILE <= n_in;
            if (!full) CHECK(tile == a.tiles - 1, AT ": tile %d is not whole and not the last", ATV, tile);
            const int tbase = tile * NVX_DIV_TILE, coff = a.cell_off + tbase;
            const int jc = coff >> 16;
            int n_a = NVX_DIV_CELL - (coff & (NVX_DIV_CELL - 1));
            const bool split = n_a < NVX_DIV_TILE && (size_t)tbase + n_a < n_in;
            if (!split) n_a = NVX_DIV_TILE;
            CHECK(jc >= 0 && jc + (split ? 1 : 0) < a.cells, AT ": tile %d touches weight %d of %d", ATV, tile, jc + (split ? 1 : 0), a.cells);
            const size_t first = (size_t)tbase;
            for (size_t j = first; walk && j < first + NVX_DIV_TILE && j < n_in; j++) {
                reached[j]++;
                const u128 cell = ((u128)consumed + j) / NVX_DIV_CELL, block = ((u128)consumed + j) / NVX_DIV_BLOCK;
                const int rel = jc + ((int)(j - first) < n_a ? 0 : 1);
                CHECK(cell - cell0 == (u128)rel, AT ": sample %zu lies in cell %d of the call", ATV, j, rel);
                // the sums kernel's record: (off0 + j) >> 8
                CHECK(block - block0 == (u128)((a.off0 + (int)j) >> 8) && ((a.off0 + (int)j) >> 8) < a.blocks, AT ": sample %zu lies in block %d of the call", ATV, j, (a.off0 + (int)j) >> 8);
            }
        }
    }
    for (size_t j = 0; walk && j < n_in; j++) CHECK(reached[j] == 1, AT ": sample %zu reached %d times", ATV, j, reached[j]);

    // 16-byte stores only where every row is 16-byte aligned
    bool aligned = true;
    for (int s = 0; s < n_pairs * n_targets; s++) aligned = aligned && ((u128)out_base + ((u128)s * pitch_out + out_first) * 4) % 16 == 0;
    CHECK((a.out_vec != 0) == aligned, AT ": out_vec %d for base %#zx, pitch %zu, first %zu, %d rows", ATV, a.out_vec, (size_t)out_base, pitch_out,
          out_first, n_pairs * n_targets);
}

int main(void)
{
    const size_t T = NVX_DIV_TILE, K = NVX_DIV_CELL;
    const size_t lengths[] = { 1, 255, 256, 257, 4095, 4096, 4097, K - 1, K, K + 1, 2 * K, 2 * K + 1, 7 * T + 5, 8 * T, 8 * T + 1, 3 * K + 32768 };
    const uint64_t positions[] = { 0, 1, 255, 256, 4095, 4096, K - 1, K, K + 1, 777, ((uint64_t)1 << 32) - 1000, ((uint64_t)1 << 40) + 5, ((uint64_t)1 << 62) - 1 - 40 * K };
    const int chunkings[] = { 0, 1, 2, 3, 683, 2048 };
    const int windows[] = { 0, 1, 2, 4 };
    for (size_t n_in : lengths)
        for (uint64_t consumed : positions)
            for (int window_log2 : windows)
                for (int wanted : chunkings) {
                    if (window_log2 != 2 && wanted != 1) continue;             // the window moves the state's size and nothing else
                    CHECK(!((consumed + n_in) >> 62), "position %llu + %zu", (unsigned long long)consumed, n_in);
                    check_case(consumed, n_in, window_log2, wanted, 3, 2, 0x7000000, 3000004, 8);
                }
    // forty cells spread over chunks, and the longest call from the last offset of a cell (not walked sample by sample)
    check_case(777, 40 * K, 2, 2048, 1, 1, 0x7000000, 0, 0);
    check_case(K - 1, NVX_DIV_MAX_IN, 4, 2048, 1, 4, 0x7000000, NVX_DIV_MAX_IN, 0, false);
    // the alignment of the output rows: n_pairs * n_targets of them
    const struct { uintptr_t base; size_t pitch, first; int pairs, targets; } OUTS[] = {
        { 0x7000000, 40020, 7, 2, 1 }, { 0x7000000, 40020, 8, 2, 1 }, { 0x7000000, 40021, 8, 2, 1 }, { 0x7000000, 40021, 8, 1, 1 }, { 0x7000000, 40021, 8, 1, 2 },
        { 0x7000004, 40020, 3, 2, 2 }, { 0x7000004, 40020, 0, 1, 1 }, { 0x7000008, 40022, 2, 1, 1 }, { 0x7000008, 40022, 2, 1, 3 }, { 0x7000000, 0, 0, 1, 1 },
    };
    for (const auto &o : OUTS) check_case(5, 40013, 4, 1, o.pairs, o.targets, o.base, o.pitch, o.first);
    printf("div launch args ok: %ld checks\n", g_checks);
    return 0;
}
