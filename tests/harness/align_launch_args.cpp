// align_launch_args.cpp -- the row aligner's launch arithmetic (navtex_amd/align/nvx_align_plan.h) without a device: for lists of
// call lengths, delays, chunkings, lags and windows, nvx_align_fill_args' and nvx_align_fill_measure_args' numbers against
// direct arithmetic in 128-bit integers.  The kernels' walks are restated.  Apply: every output of the call lies in exactly one
// tile of exactly one chunk; every sample a tile's window and its main row read lies in the carried samples or in the call;
// every carried word of the next call is written by exactly one workgroup; the delays split as the header says; where a vec
// flag is set every row of that output is 16-byte aligned.  Measure: the window is the header's, every main sample of it lies
// in one wave's share of one tile of one chunk, every lag in one workgroup, every sample read inside the call, and a 32-bit
// partial holds its 128 terms at the rails.
// Built with -fsanitize=address,undefined by tests/test_align.py; no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvx_align_plan.h"

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

// the library's nvx_align_window (nvx_align_find.c), compiled in: the harness links nothing
#include "../../navtex_amd/align/nvx_align_find.c"

#define AT "%zu samples, delay %d of max %d, %d chunks wanted"
#define ATV n_in, delay, max_delay, wanted

static void check_apply(size_t n_in, int delay, int max_delay, int wanted, int n_pairs, uintptr_t om_base, size_t pitch_om, uintptr_t os_base, size_t pitch_os,
                        size_t out_first, bool walk = true)
{
    static const char in[16] = { 0 }, in2[16] = { 0 };
    static uint32_t state[2][8], taps[256];
    static int32_t delays[4];
    nvx_align_args a;
    const int chunks = nvx_align_fill_args(in, 12345, in2, 23456, n_in, (uint32_t *)om_base, pitch_om, (uint32_t *)os_base, pitch_os, out_first, n_pairs, state[0],
                                           state[1], delays, taps, max_delay, wanted, &a);
    CHECK(a.in_main == in && a.pitch_main == 12345 && a.in_sense == in2 && a.pitch_sense == 23456 && a.out_main == (uint32_t *)om_base &&
          a.out_sense == (uint32_t *)os_base && a.pitch_out_main == pitch_om && a.pitch_out_sense == pitch_os && a.out_first == out_first, AT ": operands", ATV);
    CHECK(a.state_in == state[0] && a.state_out == state[1] && a.delays == delays && a.taps == taps && (size_t)a.n_in == n_in, AT ": state", ATV);
    const int H = max_delay + NVX_ALIGN_TAPS;
    CHECK(a.history == H && a.state_words == 2 * H, AT ": history %d", ATV, a.history);

    // tiles and chunks
    CHECK((u128)a.tiles * NVX_ALIGN_TILE >= n_in && (u128)(a.tiles - 1) * NVX_ALIGN_TILE < n_in, AT ": %d tiles", ATV, a.tiles);
    CHECK(chunks >= 1 && chunks <= (wanted < 1 ? 1 : wanted) && a.tiles_per_chunk >= 1, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    CHECK((long)chunks * a.tiles_per_chunk >= a.tiles && (long)(chunks - 1) * a.tiles_per_chunk < a.tiles, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    if (chunks > 1) CHECK(a.tiles_per_chunk >= NVX_ALIGN_MIN_CHUNK_TILES, AT ": a short chunk", ATV);
    CHECK((u128)a.tiles * NVX_ALIGN_TILE + NVX_ALIGN_TAPS < ((u128)1 << 31), AT ": the kernel counts in int", ATV);

    // the delays
    int dm, ds, f;
    nvx_align_split_delay(delay, &dm, &ds, &f);
    CHECK(dm >= 0 && ds >= 0 && f >= 0 && f < 32 && dm <= max_delay && ds <= max_delay && (dm == 0 || ds == 0), AT ": split %d %d %d", ATV, dm, ds, f);
    // the sense row leaves G + ds + f/32 late, the main row G + dm: their difference is the delay
    CHECK((i128)32 * dm - ((i128)32 * ds + f) == delay, AT ": split %d %d %d", ATV, dm, ds, f);

    // the kernel's walk
    std::vector<uint8_t> reached(walk ? n_in : 0, 0);
    for (int x = 0; x < chunks; x++) {
        const int tile0 = x * a.tiles_per_chunk, tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
        CHECK(tile0 < tile1, AT ": chunk %d is empty", ATV, x);
        for (int tile = tile0; tile < tile1; tile++) {
            const bool full = (u128)(tile + 1) * NVX_ALIGN_TILE <= n_in;
            if (!full) CHECK(tile == a.tiles - 1, AT ": tile %d is not whole and not the last", ATV, tile);
            const long tbase = (long)tile * NVX_ALIGN_TILE;
            // the window: word j holds sample tbase - ds - T + j, from the carried samples where that is negative
            const long lo = tbase - ds - NVX_ALIGN_TAPS;
            CHECK(lo >= -(long)H, AT ": tile %d reads carried word %ld", ATV, tile, H + lo);
            for (long o = 0; walk && o < NVX_ALIGN_TILE && tbase + o < (long)n_in; o++) {
                reached[tbase + o]++;
                // the taps reach samples n - ds - 15 .. n - ds, words o + 1 .. o + 16 of the window; a lane reads the twenty from its group of four on
                CHECK(tbase + o - ds - (NVX_ALIGN_TAPS - 1) == lo + o + 1 && (o & ~3L) + 19 < NVX_ALIGN_TILE + NVX_ALIGN_TAPS, AT ": output %ld", ATV, tbase + o);
                const long m = tbase + o - NVX_ALIGN_GROUP_DELAY - dm;
                CHECK(m < (long)n_in && H + m >= 0, AT ": output %ld reads main sample %ld", ATV, tbase + o, m);
            }
        }
    }
    for (size_t j = 0; walk && j < n_in; j++) CHECK(reached[j] == 1, AT ": output %zu reached %d times", ATV, j, reached[j]);

    // the carried words of the next call
    std::vector<uint8_t> written(H, 0);
    for (int x = 0; x < chunks; x++) {
        const int j0 = x * a.history_per_chunk, j1 = j0 + a.history_per_chunk < H ? j0 + a.history_per_chunk : H;
        for (int j = j0; j < j1; j++) {
            written[j]++;
            const i128 s = (i128)n_in - H + j;
            CHECK(s < (i128)n_in && (s >= 0 || ((i128)n_in + j >= 0 && (i128)n_in + j < H)), AT ": carried word %d", ATV, j);
        }
    }
    for (int j = 0; j < H; j++) CHECK(written[j] == 1, AT ": carried word %d written %d times", ATV, j, written[j]);

    // 16-byte stores only where every row is 16-byte aligned
    bool am = true, as = true;
    for (int s = 0; s < n_pairs; s++) {
        am = am && ((u128)om_base + ((u128)s * pitch_om + out_first) * 4) % 16 == 0;
        as = as && ((u128)os_base + ((u128)s * pitch_os + out_first) * 4) % 16 == 0;
    }
    CHECK((a.vec_main != 0) == am && (a.vec_sense != 0) == as, AT ": vec %d %d", ATV, a.vec_main, a.vec_sense);
}

static void check_measure(size_t n_in, int lag_first, int n_lags, int n_pairs)
{
    static const char in[16] = { 0 }, in2[16] = { 0 };
    static unsigned long long table[4], power[4];
    nvx_align_measure_args a;
    const int chunks = nvx_align_fill_measure_args(in, 111, in2, 222, n_in, lag_first, n_lags, n_pairs, table, power, &a);
    const i128 lag_last = (i128)lag_first + n_lags - 1;
    const i128 span = (lag_last > 0 ? lag_last : 0) - (lag_first < 0 ? lag_first : 0);
    const i128 window = ((i128)n_in - span) / 256 * 256;
    const bool ok = n_lags >= 64 && n_lags <= NVX_ALIGN_MAX_LAGS && n_lags % 64 == 0 && (i128)n_in - span >= NVX_ALIGN_MIN_WINDOW && n_in <= NVX_ALIGN_MAX_IN;
    CHECK((chunks > 0) == ok, "%zu samples, lags %d + %d: %d chunks", n_in, lag_first, n_lags, chunks);
    CHECK(nvx_align_window(n_in, lag_first, n_lags) == (ok ? (uint64_t)window : 0), "%zu samples, lags %d + %d: the window", n_in, lag_first, n_lags);
    if (!ok) return;
    CHECK(a.in_main == in && a.pitch_main == 111 && a.in_sense == in2 && a.pitch_sense == 222 && a.table == table && a.power == power, "operands");
    CHECK(a.window == window && a.n0 == (lag_first < 0 ? -lag_first : 0) && a.lag_first == lag_first && a.n_lags == n_lags && (size_t)a.n_in == n_in, "numbers");
    CHECK(a.window % 256 == 0 && (i128)a.tiles * NVX_ALIGN_M_TILE >= a.window && (i128)(a.tiles - 1) * NVX_ALIGN_M_TILE < a.window, "%d tiles", a.tiles);
    CHECK(chunks <= 65535 && n_lags / NVX_ALIGN_M_LAGS <= 65535 && (long)chunks * a.tiles_per_chunk >= a.tiles && (long)(chunks - 1) * a.tiles_per_chunk < a.tiles,
          "%d chunks of %d tiles", chunks, a.tiles_per_chunk);
    // a 32-bit partial: NVX_ALIGN_M_FOLD terms of at most 2 * 2048^2
    CHECK((i128)NVX_ALIGN_M_FOLD * 2 * 2048 * 2048 < ((i128)1 << 31) && (i128)2 * NVX_ALIGN_M_FOLD * 2 * 2048 * 2048 >= ((i128)1 << 31), "the fold");
    // every main sample of the window in one wave's share of one tile of one chunk; everything read lies inside the call
    long samples = 0;
    for (int y = 0; y < chunks; y++) {
        const int tile0 = y * a.tiles_per_chunk, tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
        CHECK(tile0 < tile1, "chunk %d is empty", y);
        for (int tile = tile0; tile < tile1; tile++) {
            const int left = a.window - tile * NVX_ALIGN_M_TILE, have = left < NVX_ALIGN_M_TILE ? left : NVX_ALIGN_M_TILE;
            CHECK(have > 0 && have % 256 == 0, "tile %d has %d samples", tile, have);
            for (int wave = 0; wave < 4; wave++)
                if (wave * 256 < have) samples += 256;
            const i128 first = (i128)a.n0 + (i128)tile * NVX_ALIGN_M_TILE;
            CHECK(first >= 0 && first + have <= (i128)n_in, "tile %d: main samples", tile);
            // the samples the dot products take: main sample first + i against sense sample first + i + lag, every lag of the table
            CHECK(first + lag_first >= 0 && first + have - 1 + lag_last < (i128)n_in, "tile %d: sense samples %lld .. %lld of %zu", tile,
                  (long long)(first + lag_first), (long long)(first + have - 1 + lag_last), n_in);
        }
    }
    CHECK(samples == a.window, "%ld samples walked of %d", samples, a.window);
}

int main(void)
{
    const size_t T = NVX_ALIGN_TILE;
    const size_t lengths[] = { 1, 15, 16, 17, 4095, 4096, 4097, 4 * T, 4 * T + 1, 5 * T, 9 * T + 5 };
    const int max_delays[] = { 1, 50, 4096 };
    const int chunkings[] = { 0, 1, 2, 3, 2048 };
    for (size_t n_in : lengths)
        for (int max_delay : max_delays) {
            const int delays[] = { 0, 1, 31, 32, 33, -1, -31, -32, -33, 32 * max_delay, -32 * max_delay, 32 * max_delay - 1, -32 * max_delay + 1 };
            for (int delay : delays)
                for (int wanted : chunkings)
                    if (delay >= -32 * max_delay && delay <= 32 * max_delay) check_apply(n_in, delay, max_delay, wanted, 3, 0x7000000, 3000004, 0x9000000, 3000008, 8);
        }
    // the longest call and the largest delay, not walked sample by sample
    check_apply(NVX_ALIGN_MAX_IN, 32 * NVX_ALIGN_MAX_DELAY_LIMIT, NVX_ALIGN_MAX_DELAY_LIMIT, 2048, 1, 0x7000000, 0, 0x9000000, 0, 0, false);
    check_apply(NVX_ALIGN_MAX_IN, -32 * NVX_ALIGN_MAX_DELAY_LIMIT, NVX_ALIGN_MAX_DELAY_LIMIT, 1, 1, 0x7000000, 0, 0x9000000, 0, 0, false);
    // the alignment of the output rows
    const struct { uintptr_t base; size_t pitch, first; int pairs; } OUTS[] = {
        { 0x7000000, 40020, 7, 2 }, { 0x7000000, 40020, 8, 2 }, { 0x7000000, 40021, 8, 2 }, { 0x7000000, 40021, 8, 1 }, { 0x7000004, 40020, 3, 2 },
        { 0x7000004, 40020, 0, 1 }, { 0x7000008, 40022, 2, 1 }, { 0x7000008, 40022, 2, 3 }, { 0x7000000, 0, 0, 1 },
    };
    for (const auto &o : OUTS) {
        check_apply(40013, 45, 64, 1, o.pairs, o.base, o.pitch, 0x9000000, 40020, o.first);
        check_apply(40013, 45, 64, 1, o.pairs, 0x9000000, 40020, o.base, o.pitch, o.first);
    }
    // the measurement
    const size_t m_lengths[] = { 1023, 1024, 1087, 1088, 1279, 1280, 4096 + 63, 5000, 65536 + 255, 100000, NVX_ALIGN_MAX_IN, (size_t)NVX_ALIGN_MAX_IN + 1 };
    const int firsts[] = { 0, 1, -1, -63, -64, -100, 40, -4096, 4033, -(1 << 20), (1 << 20) - 63 };
    const int counts[] = { 0, 63, 64, 128, 192, 8192, 8256 };
    for (size_t n_in : m_lengths)
        for (int lag_first : firsts)
            for (int n_lags : counts)
                for (int n_pairs : { 1, 3 }) check_measure(n_in, lag_first, n_lags, n_pairs);
    printf("align launch args ok: %ld checks\n", g_checks);
    return 0;
}
