// notch_launch_args.cpp -- the tone notch's launch arithmetic (navtex_amd/notch/nvx_notch_plan.h) without a device: for a list
// of positions, call lengths, widths, notch counts and chunkings, nvx_notch_fill_args' numbers against direct arithmetic in
// 128-bit integers.  The kernels' walk over chunks and tiles is restated: every word of the call lies in exactly one tile of
// exactly one chunk; the block of every sample, counted from the call's first, is the row's block and has a record; the two
// values of M every word interpolates between lie among the 18 its tile forms, and the block sums those are made of lie in
// the carried 2R + 2 or in the call's records; the two NCOs count from the low bits of the position and of the position less
// the delay; the parts of a row's state start 16-byte aligned and end inside the row; and where out_vec is set every row of the
// output is 16-byte aligned.
// Built with -fsanitize=address,undefined by tests/test_notch.py; no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvx_notch_plan.h"

typedef unsigned __int128 u128;
typedef __int128 i128;

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

#define AT "consumed %llu, %zu samples, width_log2 %d, %d notches, %d chunks wanted"
#define ATV (unsigned long long)consumed, n_in, r, K, wanted

static i128 floor_div(i128 a, i128 b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

static void check_case(uint64_t consumed, size_t n_in, int r, int K, int wanted, int n_rows, uintptr_t out_base, size_t pitch_out, size_t out_first,
                       bool walk = true)
{
    static int64_t state[2][4];
    static uint32_t cfg[16], table[4];
    static unsigned long long records[8];
    static const char in[16] = { 0 };
    nvx_notch_args a;
    const int chunks = nvx_notch_fill_args(consumed, in, 12345, n_in, (uint32_t *)out_base, pitch_out, out_first, n_rows, state[0], state[1], cfg, table, records,
                                           K, r, wanted, &a);
    const int R = 1 << r, D = (R + 1) * 256, H = 2 * R + 2;
    // what is handed through
    CHECK(a.in == in && a.pitch_in == 12345 && a.out == (uint32_t *)out_base && a.pitch_out == pitch_out && a.out_first == out_first, AT ": operands", ATV);
    CHECK(a.state_in == state[0] && a.state_out == state[1] && a.cfg == cfg && a.table == table && a.records == records, AT ": state", ATV);
    CHECK((size_t)a.n_in == n_in && a.n_rows == n_rows && a.n_notches == K && a.width_log2 == r, AT ": numbers", ATV);
    CHECK(a.delay == D && a.hist == H && a.notch_words == 2 * H + 6 && a.cfg_words == 2 + 2 * K, AT ": sizes", ATV);
    // the row's state: scalars, K notches, the delay line, each 16-byte aligned (in int64 words: even)
    CHECK(NVX_NOTCH_ROW_SCALARS % 2 == 0 && a.notch_words % 2 == 0 && NVX_NOTCH_DELAY_AT(r, K) == 2 + K * a.notch_words && NVX_NOTCH_DELAY_AT(r, K) % 2 == 0,
          AT ": the parts of a row", ATV);
    CHECK(a.state_words == NVX_NOTCH_DELAY_AT(r, K) + D / 2 && a.state_words % 2 == 0 && D % 8 == 0, AT ": %d state words", ATV, a.state_words);
    CHECK(2 * H + NVX_NOTCH_ST_FROM < a.notch_words && NVX_NOTCH_ST_PARTIAL % 2 == 0 && NVX_NOTCH_ST_X % 2 == 0, AT ": a notch's words", ATV);
    CHECK(a.position == (int64_t)consumed && a.in_lo == (uint32_t)(consumed & 0xffffffffu) &&
          a.out_lo == (uint32_t)(((u128)consumed + ((u128)1 << 64) - D) & 0xffffffffu), AT ": the NCOs' first samples", ATV);

    // tiles and chunks
    CHECK((u128)a.tiles * NVX_NOTCH_TILE >= n_in && (u128)(a.tiles - 1) * NVX_NOTCH_TILE < n_in, AT ": %d tiles", ATV, a.tiles);
    CHECK(chunks >= 1 && chunks <= (wanted < 1 ? 1 : wanted) && a.tiles_per_chunk >= 1, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    CHECK((long)chunks * a.tiles_per_chunk >= a.tiles && (long)(chunks - 1) * a.tiles_per_chunk < a.tiles, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    if (chunks > 1) CHECK(a.tiles_per_chunk >= NVX_NOTCH_MIN_CHUNK_TILES, AT ": a short chunk", ATV);
    if (wanted <= 1) CHECK(chunks == 1 && a.tiles_per_chunk == a.tiles, AT ": one chunk", ATV);
    CHECK(NVX_NOTCH_TILE % NVX_NOTCH_BLOCK == 0 && NVX_NOTCH_TILE / NVX_NOTCH_BLOCK + 2 == NVX_NOTCH_TILE_M && D % 512 == 256, "a tile, its values of M, the delay");

    // blocks and records
    const u128 block0 = (u128)consumed / NVX_NOTCH_BLOCK, last_block = ((u128)consumed + n_in - 1) / NVX_NOTCH_BLOCK;
    CHECK(a.off0 >= 0 && a.off0 < NVX_NOTCH_BLOCK && (u128)a.off0 == (u128)consumed % NVX_NOTCH_BLOCK, AT ": off0 %d", ATV, a.off0);
    CHECK((u128)a.blocks == last_block - block0 + 1, AT ": %d records", ATV, a.blocks);
    CHECK((u128)a.done == ((u128)consumed + n_in) / NVX_NOTCH_BLOCK - block0 && a.done <= a.blocks && a.done >= a.blocks - 1, AT ": %d blocks done", ATV, a.done);
    CHECK((u128)a.off0 + n_in + NVX_NOTCH_TILE < ((u128)1 << 31), AT ": the kernels count in int", ATV);
    CHECK(a.g0 == a.off0 - D - 128, AT ": g0 %d", ATV, a.g0);

    // the kernels' walk (word by word, unless the call is too long for that)
    std::vector<uint8_t> reached(walk ? n_in : 0, 0);
    for (int x = 0; x < chunks; x++) {
        const int tile0 = x * a.tiles_per_chunk, tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
        CHECK(tile0 < tile1, AT ": chunk %d is empty", ATV, x);
        for (int tile = tile0; tile < tile1; tile++) {
            const int tbase = tile * NVX_NOTCH_TILE;
            const int lo0 = (a.g0 + tbase) >> 8;
            // the block sums the tile's 18 values of M are made of: carried ones or records (those behind the call's last are taken as zero)
            CHECK(lo0 - (R - 1) >= -H, AT ": tile %d reads carried block %d of %d", ATV, tile, lo0 - (R - 1), H);
            for (size_t j = (size_t)tbase; walk && j < (size_t)tbase + NVX_NOTCH_TILE && j < n_in; j++) {
                reached[j]++;
                // the sample read at j: its block, counted from the call's first
                const u128 block = ((u128)consumed + j) / NVX_NOTCH_BLOCK;
                CHECK(block - block0 == (u128)((a.off0 + (int)j) >> 8) && (int)(block - block0) < a.blocks, AT ": sample %zu's block", ATV, j);
                // the word written at j is y[m], m = consumed + j - D: lo = (m - 128) div 256, f = (m - 128) mod 256
                const i128 m = (i128)consumed + (i128)j - D;
                const i128 lo = floor_div(m - 128, 256);
                const int g = a.g0 + (int)j, v = (g >> 8) - lo0;
                CHECK(lo - (i128)block0 == (i128)(g >> 8) && (i128)(g & 255) == m - 128 - lo * 256, AT ": word %zu interpolates at %d, %d", ATV, j, g >> 8, g & 255);
                CHECK(v >= 0 && v + 1 < NVX_NOTCH_TILE_M, AT ": word %zu reads value %d of its tile", ATV, j, v);
                // the newest block under M[lo + 1] has ended inside the call or in front of it
                CHECK((g >> 8) + 1 + (R - 1) <= a.blocks - 2 || (g >> 8) + 1 + (R - 1) < 0, AT ": word %zu needs block %d of %d", ATV, j, (g >> 8) + R, a.blocks);
                CHECK((uint32_t)(a.out_lo + (uint32_t)j) == (uint32_t)((u128)(m + ((i128)1 << 64)) & 0xffffffffu), AT ": word %zu's phase index", ATV, j);
            }
        }
    }
    for (size_t j = 0; walk && j < n_in; j++) CHECK(reached[j] == 1, AT ": word %zu reached %d times", ATV, j, reached[j]);

    // 16-byte stores only where every row is 16-byte aligned
    bool aligned = true;
    for (int s = 0; s < n_rows; s++) aligned = aligned && ((u128)out_base + ((u128)s * pitch_out + out_first) * 4) % 16 == 0;
    CHECK((a.out_vec != 0) == aligned, AT ": out_vec %d for base %#zx, pitch %zu, first %zu, %d rows", ATV, a.out_vec, (size_t)out_base, pitch_out, out_first,
          n_rows);
}

int main(void)
{
    const size_t T = NVX_NOTCH_TILE, G = NVX_NOTCH_BLOCK;
    const size_t lengths[] = { 1, 127, 128, 129, G - 1, G, G + 1, 1279, 1280, 1281, T - 1, T, T + 1, 7 * T + 5, 8 * T, 8 * T + 1, 16640, 40000 };
    const uint64_t positions[] = { 0, 1, 127, 128, 129, G - 1, G, G + 1, 777, T - 1, T, ((uint64_t)1 << 32) - 1000, ((uint64_t)1 << 32) + 1280,
                                   ((uint64_t)1 << 40) + 5, ((uint64_t)1 << 62) - 1 - 40000 };
    const int chunkings[] = { 0, 1, 2, 3, 8, 2048 };
    for (size_t n_in : lengths)
        for (uint64_t consumed : positions)
            for (int r = NVX_NOTCH_WIDTH_LOG2_MIN; r <= NVX_NOTCH_WIDTH_LOG2_MAX; r++)
                for (int wanted : chunkings) {
                    if (r != 2 && wanted != 1) continue;                       // the width moves the delay and the carried sums, not the chunks
                    CHECK(!((consumed + n_in) >> 62), "position %llu + %zu", (unsigned long long)consumed, n_in);
                    check_case(consumed, n_in, r, 1 + (r + (int)n_in) % 4, wanted, 3, 0x7000000, 3000004, 8);
                }
    // ten tiles spread over two chunks, and the longest call from the last offset of a block (not walked word by word)
    check_case(0, 40000, 2, 2, 8, 256, 0x7000000, 40000, 0);
    check_case(G - 1, NVX_NOTCH_MAX_IN, 6, 4, 2048, 1, 0x7000000, 0, 0, false);
    // the alignment of the output rows
    const struct { uintptr_t base; size_t pitch, first; int rows; } OUTS[] = {
        { 0x7000000, 40020, 7, 2 }, { 0x7000000, 40020, 8, 2 }, { 0x7000000, 40021, 8, 2 }, { 0x7000000, 40021, 8, 1 }, { 0x7000004, 40020, 3, 2 },
        { 0x7000004, 40020, 0, 1 }, { 0x7000008, 40022, 2, 1 }, { 0x7000008, 40022, 2, 3 }, { 0x7000000, 0, 0, 1 },
    };
    for (const auto &o : OUTS) check_case(5, 40013, 4, 3, 1, o.rows, o.base, o.pitch, o.first);
    printf("notch launch args ok: %ld checks\n", g_checks);
    return 0;
}
