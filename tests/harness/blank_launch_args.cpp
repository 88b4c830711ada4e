// blank_launch_args.cpp -- the blanker's launch arithmetic (navtex_amd/blank/nvx_blank_plan.h) without a device: for a list
// of positions, call lengths and chunkings, nvx_blank_fill_args' numbers against direct arithmetic in 128-bit integers.  The
// kernel's walk over chunks, tiles and wave regions is restated: every sample of the call lies in exactly one live tile of
// exactly one chunk; a later chunk's pre-roll lies inside the call and consists of whole tiles; every region's block end falls
// on the last sample of a block of the stream; whole tiles (the ones read and written 16 bytes at a time) end inside the
// call; and where out_vec is set every row of the output is 16-byte aligned.
// Built with -fsanitize=address,undefined by tests/test_blank.py; no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvx_blank_plan.h"

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

#define AT "consumed %llu, %zu samples, %d chunks wanted"
#define ATV (unsigned long long)consumed, n_in, wanted

static void check_case(uint64_t consumed, size_t n_in, int wanted, int n_streams, uintptr_t out_base, size_t pitch_out, size_t out_first)
{
    static uint32_t state[2][16];
    static unsigned long long counters[4];
    static const char in[16] = { 0 };
    nvx_blank_args a;
    const int chunks = nvx_blank_fill_args(consumed, in, 12345, n_in, (uint32_t *)out_base, pitch_out, out_first, n_streams, state[0], state[1], counters,
                                           1024, 32, 64, wanted, &a);
    // what is handed through
    CHECK(a.in == in && a.pitch_in == 12345 && a.out == (uint32_t *)out_base && a.pitch_out == pitch_out && a.out_first == out_first, AT ": operands", ATV);
    CHECK(a.state_in == state[0] && a.state_out == state[1] && a.counters == counters, AT ": state", ATV);
    CHECK((size_t)a.n_in == n_in && a.thr_q8 == 1024 && a.hold == 32 && a.floor == 64, AT ": numbers", ATV);

    // tiles and chunks
    CHECK((u128)a.tiles * NVX_BLANK_TILE >= n_in && (u128)(a.tiles - 1) * NVX_BLANK_TILE < n_in, AT ": %d tiles", ATV, a.tiles);
    CHECK(chunks >= 1 && chunks <= (wanted < 1 ? 1 : wanted) && a.tiles_per_chunk >= 1, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    CHECK((long)chunks * a.tiles_per_chunk >= a.tiles && (long)(chunks - 1) * a.tiles_per_chunk < a.tiles, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    if (chunks > 1) CHECK(a.tiles_per_chunk >= NVX_BLANK_MIN_CHUNK_TILES && NVX_BLANK_MIN_CHUNK_TILES >= 16 * NVX_BLANK_PREROLL_TILES, AT ": a short chunk", ATV);
    if (wanted <= 1) CHECK(chunks == 1 && a.tiles_per_chunk == a.tiles, AT ": one chunk", ATV);

    // the block ends
    const u128 phase = (u128)consumed % NVX_BLANK_BLOCK;
    CHECK(a.off >= 1 && a.off <= NVX_BLANK_BLOCK && (u128)a.off == NVX_BLANK_BLOCK - phase, AT ": off %d", ATV, a.off);

    // the kernel's walk
    std::vector<uint8_t> reached(n_in, 0);
    for (int x = 0; x < chunks; x++) {
        const int tile0 = x * a.tiles_per_chunk, tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
        int tile = x == 0 ? 0 : tile0 - NVX_BLANK_PREROLL_TILES;
        CHECK(tile >= 0 && tile0 < tile1, AT ": chunk %d walks from tile %d", ATV, x, tile);
        int whole_ends = 0;
        for (; tile < tile1; tile++) {
            const bool live = tile >= tile0, full = (u128)(tile + 1) * NVX_BLANK_TILE <= n_in;
            if (!live) CHECK(full, AT ": chunk %d: pre-roll tile %d is not a whole one", ATV, x, tile);
            if (!full) CHECK(tile == a.tiles - 1, AT ": tile %d is not whole and not the last", ATV, tile);
            for (int w = 0; w < NVX_BLANK_WAVES; w++) {
                const u128 end = (u128)tile * NVX_BLANK_TILE + (u128)w * NVX_BLANK_BLOCK + a.off - 1;       // of the call
                CHECK(((u128)consumed + end) % NVX_BLANK_BLOCK == NVX_BLANK_BLOCK - 1, AT ": tile %d region %d ends a block at %llu", ATV, tile, w,
                      (unsigned long long)end);
                if (!live && end >= NVX_BLANK_BLOCK - 1) whole_ends++;          // a whole block of the call ends here
            }
            if (live) {
                const size_t first = (size_t)tile * NVX_BLANK_TILE;
                for (size_t j = first; j < first + NVX_BLANK_TILE && j < n_in; j++) reached[j]++;
            }
        }
        // behind its pre-roll a later chunk has seen the ends of at least five whole blocks: four sums for the level of the
        // block that lies `hold` back, and that block's own
        if (x > 0) CHECK(whole_ends >= 5, AT ": chunk %d has %d whole blocks in its pre-roll", ATV, x, whole_ends);
    }
    for (size_t j = 0; j < n_in; j++) CHECK(reached[j] == 1, AT ": sample %zu reached %d times", ATV, j, reached[j]);

    // 16-byte stores only where every row is 16-byte aligned
    bool aligned = true;
    for (int s = 0; s < n_streams; s++) aligned = aligned && ((u128)out_base + ((u128)s * pitch_out + out_first) * 4) % 16 == 0;
    CHECK((a.out_vec != 0) == aligned, AT ": out_vec %d for base %#zx, pitch %zu, first %zu, %d streams", ATV, a.out_vec, (size_t)out_base, pitch_out,
          out_first, n_streams);
}

int main(void)
{
    const size_t T = NVX_BLANK_TILE, lengths[] = { 1, 1023, 1024, 1025, T - 1, T, T + 1, 31 * T + 5, 32 * T, 32 * T + 1, 64 * T, 74 * T - 77, 300000 };
    const uint64_t positions[] = { 0, 1, 1023, 1024, 1025, ((uint64_t)1 << 32) - 1000, ((uint64_t)1 << 40) + 5, ((uint64_t)1 << 62) - 1 - 400000 };
    const int chunkings[] = { 0, 1, 2, 3, 683, 2048 };
    for (size_t n_in : lengths)
        for (uint64_t consumed : positions)
            for (int wanted : chunkings) {
                CHECK(!((consumed + n_in) >> 62), "position %llu + %zu", (unsigned long long)consumed, n_in);
                check_case(consumed, n_in, wanted, 3, 0x7000000, 300004, 8);
            }
    // the alignment of the output rows
    const struct { uintptr_t base; size_t pitch, first; int streams; } OUTS[] = {
        { 0x7000000, 40020, 7, 2 }, { 0x7000000, 40020, 8, 2 }, { 0x7000000, 40021, 8, 2 }, { 0x7000000, 40021, 8, 1 }, { 0x7000004, 40020, 3, 2 },
        { 0x7000004, 40020, 0, 1 }, { 0x7000008, 40022, 2, 1 }, { 0x7000008, 40022, 2, 3 }, { 0x7000000, 0, 0, 1 },
    };
    for (const auto &o : OUTS) check_case(5, 40013, 1, o.streams, o.base, o.pitch, o.first);
    printf("blank launch args ok: %ld checks\n", g_checks);
    return 0;
}
