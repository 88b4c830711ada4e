// nb_launch_args.cpp -- the narrowband interpolator's launch arithmetic (navtex_amd/narrow/nvx_narrow_plan.h) without a device:
// for a list of rates, positions, call lengths and chunkings, nvx_nb_fill_shape's and nvx_nb_fill_args' numbers against
// direct arithmetic in 128-bit integers.  The kernel's walk over chunks, tiles, windows and a window's outputs is restated with
// the functions the kernel itself runs (nvx_nb_chunk_start, nvx_nb_tile_next, nvx_nb_window_first, nvx_nb_divmod): every output
// of the call is produced exactly once, by the window q = n M div L of its stream position n, at phase r = n M mod L; the row of
// the tap table it reads exists; the samples its window reaches over lie in the tile's staged span, and that span in the LDS;
// its word lies in the tile's output image; the image is stored between the tile's first output and the next tile's; the
// state's writer takes every sample from the input or from the row read.
// Built with -fsanitize=address,undefined by tests/test_narrow.py; no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvx_narrow_plan.h"

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

#define AT "L %d M %d T %d, consumed %llu, %zu samples, %d chunks wanted"
#define ATV L, M, T, (unsigned long long)consumed, n_in, wanted

static void check_case(int L, int M, int T, uint64_t consumed, size_t n_in, int wanted, bool walk = true)
{
    static uint32_t state[2][NVX_NB_STATE_WORDS], table[4];
    static const char in[16] = { 0 };
    nvx_nb_args a = {};
    nvx_nb_fill_shape(L, M, T, &a);
    // the shape
    const int jmax = (L + M - 1) / M, parts = 1 << a.pshift;
    CHECK(a.tq >= 1 && a.tq <= 4 && 8 * a.tq >= T && 8 * (a.tq - 1) < T && (a.row_quads & 1) && a.row_quads >= a.tq && a.row_quads <= a.tq + 1, AT ": rows", ATV);
    CHECK(a.table_quads == L * a.row_quads && (size_t)a.table_quads * 16 <= (size_t)NVX_NB_MAX_PHASES * 5 * 16, AT ": the table", ATV);
    CHECK(a.jlo * M + a.lr == L && a.lr >= 0 && a.lr < M, AT ": jlo, lr", ATV);
    CHECK(a.part <= NVX_NB_PART_OUTPUTS && a.part * parts >= jmax && a.windows * parts == NVX_NB_THREADS, AT ": %d parts of %d", ATV, parts, a.part);
    CHECK((size_t)a.windows * jmax + 3 <= NVX_NB_OUT_WORDS && a.windows + 8 * a.tq - 1 <= NVX_NB_STAGE_WORDS, AT ": the LDS", ATV);
    CHECK((u128)a.tile_di * M + a.tile_dr == (u128)a.windows * L && a.tile_dr < (uint32_t)M, AT ": the tile's step", ATV);

    const int chunks = nvx_nb_fill_args(consumed, in, 12345, n_in, (uint32_t *)0x7000000, 54321, 8, state[0], state[1], table, wanted, &a);
    CHECK(a.in == in && a.pitch_in == 12345 && a.out == (uint32_t *)0x7000000 && a.pitch_out == 54321 && a.out_first == 8, AT ": operands", ATV);
    CHECK(a.state_in == state[0] && a.state_out == state[1] && a.table == table, AT ": state", ATV);
    // the counts, directly
    const u128 before = ((u128)consumed * L + M - 1) / M, after = ((u128)(consumed + n_in) * L + M - 1) / M;
    CHECK((u128)a.n_in == n_in && (u128)a.n_out == after - before && a.n_out > 0, AT ": %d outputs", ATV, a.n_out);
    CHECK((u128)a.e0 == before * M - (u128)consumed * L && a.e0 < (uint32_t)M, AT ": e0 %u", ATV, a.e0);
    // tiles and chunks
    CHECK((u128)a.tiles * a.windows >= n_in && (u128)(a.tiles - 1) * a.windows < n_in, AT ": %d tiles", ATV, a.tiles);
    CHECK(chunks >= 1 && chunks <= NVX_NB_MAX_CHUNKS && chunks <= (wanted < 1 ? 1 : wanted) && a.tiles_per_chunk >= 1, AT ": %d chunks", ATV, chunks);
    CHECK((long)chunks * a.tiles_per_chunk >= a.tiles && (long)(chunks - 1) * a.tiles_per_chunk < a.tiles, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    if (chunks > 1) CHECK(a.tiles_per_chunk >= NVX_NB_MIN_CHUNK_TILES, AT ": a short chunk", ATV);
    CHECK((u128)a.chunk_di * M + a.chunk_dr == (u128)a.tiles_per_chunk * a.windows * L && a.chunk_dr < (uint32_t)M, AT ": the chunk's step", ATV);
    CHECK((u128)(chunks - 1) * a.chunk_dr + M < ((u128)1 << 23), AT ": the chunk's divider has 23 bits", ATV);

    const int Tp = 8 * a.tq;
    std::vector<uint8_t> reached(walk ? a.n_out : 0, 0);
    for (int x = 0; x < chunks; x++) {
        const int tile0 = x * a.tiles_per_chunk, tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
        CHECK(tile0 < tile1, AT ": chunk %d is empty", ATV, x);
        uint32_t ti, tr;
        nvx_nb_chunk_start(a, (uint32_t)x, &ti, &tr);
        for (int tile = tile0; tile < tile1; tile++) {
            const long kb = (long)tile * a.windows;
            CHECK(kb < (long)n_in, AT ": tile %d starts behind the call", ATV, tile);
            // the tile's first output, directly: i = ceil((kb L - e0) / M), with the stream's positions
            const u128 first = ((u128)(consumed + kb) * L + M - 1) / M;
            CHECK((u128)ti == first - before && (u128)tr == first * M - (u128)(consumed + kb) * L, AT ": tile %d starts at output %u, phase %u", ATV, tile, ti, tr);
            uint32_t ni, nr;
            nvx_nb_tile_next(a, ti, tr, &ni, &nr);
            const uint32_t i_end = kb + a.windows >= (long)n_in ? (uint32_t)a.n_out : ni, image0 = ti & ~3u;
            CHECK(i_end > ti && i_end <= (uint32_t)a.n_out && i_end - image0 <= NVX_NB_OUT_WORDS - 4 + 3, AT ": tile %d ends at %u", ATV, tile, i_end);
            // the staged span: samples kb - (Tp - 1) .. kb + windows - 1 at stage[0 ...]
            CHECK(a.windows + Tp - 1 <= NVX_NB_STAGE_WORDS, "the stage");
            if (walk || tile == tile0 || tile == tile1 - 1) {
                u128 made = 0;
                for (int tid = 0; tid < NVX_NB_THREADS; tid++) {
                    const int w = tid >> a.pshift, first_j = (tid & (parts - 1)) * a.part;
                    if (kb + w >= (long)n_in) continue;
                    uint32_t aw, bw, i0, r0;
                    int count;
                    CHECK((u128)w * L < ((u128)1 << 19), "the window's divider has 19 bits");
                    nvx_nb_divmod((uint32_t)w * (uint32_t)L, (uint32_t)M, 19, &aw, &bw);
                    CHECK((u128)aw * M + bw == (u128)w * L && bw < (uint32_t)M, "divmod");
                    nvx_nb_window_first(a, ti, tr, aw, bw, &i0, &r0, &count);
                    const u128 q = (u128)consumed + kb + w, wfirst = (q * L + M - 1) / M, wnext = ((q + 1) * L + M - 1) / M;
                    CHECK((u128)i0 == wfirst - before && (u128)count == wnext - wfirst && (u128)r0 == wfirst * M - q * L, AT ": window %ld", ATV, kb + w);
                    // its samples in the stage: w .. w + Tp - 1, the last one the window's own
                    CHECK(w + Tp - 1 < a.windows + Tp - 1 && w + Tp - 1 < NVX_NB_STAGE_WORDS, "the window in the stage");
                    const int last_j = first_j + a.part < count ? first_j + a.part : count;
                    for (int j = first_j; j < last_j; j++) {
                        const u128 n = wfirst + j, pos = n * M;
                        const uint32_t r = r0 + (uint32_t)j * (uint32_t)M;
                        CHECK(pos / L == q && pos % L == r && r < (uint32_t)L, AT ": output %u + %d of window %ld", ATV, i0, j, kb + w);
                        CHECK((size_t)(r * (uint32_t)a.row_quads + a.tq) <= (size_t)a.table_quads, "the row in the table");
                        const uint32_t i = i0 + j;
                        CHECK(i >= ti && i < i_end && i - image0 < NVX_NB_OUT_WORDS, AT ": output %u outside tile %d's image", ATV, i, tile);
                        if (walk) reached[i]++;
                        made++;
                    }
                }
                // the store: slots [ti - image0, i_end - image0), read 16 bytes at a time
                for (uint32_t s = 0; s < i_end - image0; s += 4) CHECK(s + 3 < NVX_NB_OUT_WORDS, "the image read 16 bytes at a time");
                CHECK(made == i_end - ti, AT ": tile %d made %llu of %u outputs", ATV, tile, (unsigned long long)made, i_end - ti);
            }
            ti = ni; tr = nr;
        }
    }
    for (size_t j = 0; walk && j < reached.size(); j++) CHECK(reached[j] == 1, AT ": output %zu reached %d times", ATV, j, reached[j]);
    // the state's writer: sample n_in - (T - 1) + t of the call, from the input or from the row read
    for (int t = 0; t < T - 1; t++) {
        const long at = (long)n_in - (T - 1) + t;
        if (at >= 0) CHECK(at < (long)n_in, AT ": state sample %d", ATV, t);
        else CHECK(T - 1 + at >= 0 && T - 1 + at < T - 1 && T - 1 <= NVX_NB_STATE_WORDS, AT ": state sample %d", ATV, t);
    }
}

int main(void)
{
    // L, M, T of 12000, 8000, 11025, 11025 / 2, 12500, 96000, 64000, 88200, 2000, 4000, 6250, 44100, 48000, 3000, 95999 / 2;
    // then the rows of three 16-byte words -- 72000 (T = 20), 67200 (24: the row is full), 75600 and 73332 (18) --, the full
    // two-word row of 84000 (16) and the four-word row behind six zeros of 64800 (26)
    const int PLANS[][3] = { { 21, 1, 30 }, { 63, 2, 30 }, { 160, 7, 30 }, { 320, 7, 30 }, { 504, 25, 30 }, { 21, 8, 12 }, { 63, 16, 28 }, { 20, 7, 14 },
                             { 126, 1, 30 }, { 63, 1, 30 }, { 1008, 25, 30 }, { 40, 7, 30 }, { 21, 4, 30 }, { 84, 1, 30 }, { 1000, 381, 12 },
                             { 7, 2, 20 }, { 15, 4, 24 }, { 10, 3, 18 }, { 1000, 291, 18 }, { 3, 1, 16 }, { 35, 9, 26 } };
    const size_t lengths[] = { 1, 2, 10, 28, 29, 30, 63, 64, 65, 255, 256, 257, 800, 1027, 3 * 256 + 37 };
    const uint64_t positions[] = { 0, 1, 7, 29, 30, 4097, ((uint64_t)1 << 32) - 1000, ((uint64_t)1 << 40) + 6, ((uint64_t)1 << 62) - 5000 };
    const int chunkings[] = { 0, 1, 2, 3, 683, 2048 };
    for (const auto &p : PLANS)
        for (size_t n : lengths)
            for (uint64_t consumed : positions)
                for (int wanted : chunkings) check_case(p[0], p[1], p[2], consumed, n, wanted);
    // a stream spread over many chunks, and long calls (walked at the ends of every chunk only)
    check_case(21, 1, 30, 54, 12000, 32);
    check_case(160, 7, 30, 54, 11025, 2048);
    check_case(1000, 381, 12, 3, 400000, 2048);
    check_case(21, 8, 12, 2, NVX_NB_MAX_IN / 2, 2048, false);
    check_case(21, 8, 12, 2, NVX_NB_MAX_IN / 2, 1, false);
    check_case(21, 1, 30, ((uint64_t)1 << 61) + 5, 100000000, 4096, false);
    printf("narrow launch args ok: %ld checks\n", g_checks);
    return 0;
}
