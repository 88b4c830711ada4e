// stream_plan_core.cpp -- the launch arithmetic the same-rate companions share (navtex_amd/csrc/nvx_stream_plan.h) without a
// device, against arithmetic restated here.  The chunk split, for every number of tiles up to 300, every number of chunks
// wanted from -1 to 40 and two large ones, and the three shortest chunks a library allows: every tile lies in exactly one
// chunk, no chunk is empty, there are no more chunks than wanted, every chunk but the last has tiles_per_chunk tiles, at
// least the shortest allowed where there is more than one, and no tiles give one chunk.  The rule for `wanted`, for every
// number of rows around its threshold.  The alignment of the output rows, row by row, for the bases, pitches, firsts and row
// counts of real_launch_args.cpp's OUTS.
// Built with -fsanitize=address,undefined by tests/test_stream_plan.py; no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvx_stream_plan.h"

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

#define AT "%d tiles, %d chunks wanted, at least %d tiles a chunk"
#define ATV tiles, wanted, min_tiles

static void check_split(int tiles, int wanted, int min_tiles)
{
    int per = -12345;
    const int chunks = nvx_stream_chunks(tiles, wanted, min_tiles, &per);
    const int most = wanted > 1 ? wanted : 1;
    CHECK(per >= 1 && chunks >= 1 && chunks <= most, AT ": %d chunks of %d", ATV, chunks, per);
    if (tiles == 0) { CHECK(chunks == 1, AT ": %d chunks", ATV, chunks); return; }
    if (chunks > 1) CHECK(per >= min_tiles, AT ": chunks of %d", ATV, per);
    // the walk of a grid's x: chunk x takes tiles [x * per, (x + 1) * per) below `tiles`
    std::vector<int> reached((size_t)tiles, 0);
    for (int x = 0; x < chunks; x++) {
        const int tile0 = x * per, tile1 = tile0 + per < tiles ? tile0 + per : tiles;
        CHECK(tile0 < tile1, AT ": chunk %d is empty", ATV, x);
        if (x < chunks - 1) CHECK(tile1 - tile0 == per, AT ": chunk %d has %d tiles, not %d", ATV, x, tile1 - tile0, per);
        for (int t = tile0; t < tile1; t++) reached[(size_t)t]++;
    }
    for (int t = 0; t < tiles; t++) CHECK(reached[(size_t)t] == 1, AT ": tile %d lies in %d chunks", ATV, t, reached[(size_t)t]);
    // the split itself, restated: the fewest tiles a chunk that reach every tile with `most` chunks, not below the shortest
    // allowed, not above the row
    int expect = 1;
    while ((long)expect * most < tiles) expect++;
    if (expect < min_tiles) expect = min_tiles;
    if (expect > tiles) expect = tiles;
    CHECK(per == expect, AT ": chunks of %d, not %d", ATV, per, expect);
}

int main(void)
{
    const int mins[] = { 1, 4, 32 };
    for (int min_tiles : mins)
        for (int tiles = 0; tiles <= 300; tiles++) {
            for (int wanted = -1; wanted <= 40; wanted++) check_split(tiles, wanted, min_tiles);
            check_split(tiles, 683, min_tiles);
            check_split(tiles, 2048, min_tiles);
        }

    // a workgroup per row from 1024 rows on; below that the fewest workgroups a row that give the grid `target`
    const int targets[] = { 1, 2047, 2048, 4096 };
    for (int target : targets)
        for (int rows = 1; rows <= 70000; rows += rows < 3000 ? 1 : 997) {
            const int wanted = nvx_stream_wanted(rows, target);
            if (rows >= 1024) { CHECK(wanted == 1, "%d rows, target %d: %d wanted", rows, target, wanted); continue; }
            CHECK(wanted >= 1 && (long)wanted * rows >= target && (long)(wanted - 1) * rows < target, "%d rows, target %d: %d wanted", rows, target, wanted);
        }

    // the alignment of the output rows
    const struct { uintptr_t base; size_t pitch, first; int rows; } OUTS[] = {
        { 0x7000000, 40020, 7, 2 }, { 0x7000000, 40020, 8, 2 }, { 0x7000000, 40021, 8, 2 }, { 0x7000000, 40021, 8, 1 }, { 0x7000004, 40020, 3, 2 },
        { 0x7000004, 40020, 0, 1 }, { 0x7000008, 40022, 2, 1 }, { 0x7000008, 40022, 2, 3 }, { 0x7000000, 0, 0, 1 },
    };
    int set = 0;
    for (const auto &o : OUTS) {
        bool aligned = true;
        for (int r = 0; r < o.rows; r++) aligned = aligned && ((u128)o.base + ((u128)r * o.pitch + o.first) * 4) % 16 == 0;
        const int got = nvx_stream_rows_aligned16((const void *)o.base, o.pitch, o.first, o.rows);
        CHECK((got != 0) == aligned, "aligned %d for base %#zx, pitch %zu, first %zu, %d rows", got, (size_t)o.base, o.pitch, o.first, o.rows);
        set += got != 0;
    }
    CHECK(set > 0 && set < (int)(sizeof OUTS / sizeof OUTS[0]), "%d of the rows' layouts are aligned: both answers are to be seen", set);
    printf("stream plan core ok: %ld checks\n", g_checks);
    return 0;
}
