// real_launch_args.cpp -- the real-input converter's launch arithmetic (navtex_amd/real/nvx_real_plan.h) without a device: for
// a list of positions, call lengths and chunkings, nvx_real_fill_args' numbers against direct arithmetic in 128-bit integers.
// The kernel's walk over chunks, tiles and groups of four outputs is restated: every output of the call lies in exactly one
// group of one tile of one chunk; whole tiles (the ones read and written 16 bytes at a time) end inside the call; a tile's
// halo is the state row in front of the call's first tile and lies inside the call's input everywhere else; the LDS image
// holds everything staged and read; the sign of every output is the contract's, and that of a group's first output is the
// same for the whole launch; the state's writer takes every pair from the input or from the row read; and where out_vec is
// set every row of the output is 16-byte aligned.
// Built with -fsanitize=address,undefined by tests/test_real.py; no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvx_real_plan.h"

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

#define AT "consumed %llu, %zu samples, %d chunks wanted"
#define ATV (unsigned long long)consumed, n_in, wanted

static void check_case(uint64_t consumed, size_t n_in, int wanted, int invert, int n_streams, uintptr_t out_base, size_t pitch_out, size_t out_first,
                       bool walk = true)
{
    static uint32_t state[2][NVX_REAL_STATE_WORDS * 3];
    static const char in[16] = { 0 };
    nvx_real_args a;
    const int chunks = nvx_real_fill_args(consumed, in, 12345, n_in, (uint32_t *)out_base, pitch_out, out_first, n_streams, state[0], state[1], invert, wanted, &a);
    const int T = NVX_REAL_TILE;
    // what is handed through
    CHECK(a.in == in && a.pitch_in == 12345 && a.out == (uint32_t *)out_base && a.pitch_out == pitch_out && a.out_first == out_first, AT ": operands", ATV);
    CHECK(a.state_in == state[0] && a.state_out == state[1] && a.invert == invert, AT ": state", ATV);
    CHECK(n_in % 2 == 0 && (u128)a.n * 2 == n_in && a.n >= 0, AT ": %d outputs", ATV, a.n);
    const size_t n = n_in / 2;

    // tiles and chunks
    CHECK((u128)a.tiles * T >= n && (n == 0 || (u128)(a.tiles - 1) * T < n), AT ": %d tiles", ATV, a.tiles);
    CHECK(chunks >= 1 && chunks <= (wanted < 1 ? 1 : wanted) && a.tiles_per_chunk >= 1, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    if (n) CHECK((long)chunks * a.tiles_per_chunk >= a.tiles && (long)(chunks - 1) * a.tiles_per_chunk < a.tiles, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    if (chunks > 1) CHECK(a.tiles_per_chunk >= NVX_REAL_MIN_CHUNK_TILES, AT ": a short chunk", ATV);
    if (wanted <= 1 && n) CHECK(chunks == 1 && a.tiles_per_chunk == a.tiles, AT ": one chunk", ATV);
    CHECK((u128)a.tiles * T < ((u128)1 << 31), AT ": the kernel counts in int", ATV);

    // the sign: s = +1 where m - K is even, m the stream's output
    const i128 m0 = (i128)(consumed / 2);
    CHECK(a.par == 0 || a.par == 1, AT ": par %d", ATV, a.par);
    const size_t probes[] = { 0, 1, 2, 3, n ? n - 1 : 0, n / 2, 4097 };
    for (size_t i : probes) {
        i128 d = m0 + (i128)i - NVX_REAL_K;
        const bool even = (d % 2) == 0;
        CHECK((((a.par + (int)(i & 1)) & 1) == 0) == even, AT ": the sign of output %zu", ATV, i);
    }

    // the LDS image
    CHECK(NVX_REAL_TILE == 4 * NVX_REAL_THREADS * 4 && NVX_REAL_TILE == NVX_REAL_WAVES * NVX_REAL_REGION, "a tile is four groups of four outputs a thread");
    CHECK(NVX_REAL_HALO_AT >= NVX_REAL_HISTORY && NVX_REAL_HISTORY == 2 * NVX_REAL_K + 2 && NVX_REAL_STATE_WORDS == NVX_REAL_HISTORY, "the halo");
    for (int spt = 4; spt <= 8; spt += 4)
        for (int wave = 0; wave < NVX_REAL_WAVES; wave++)
            for (int lane = 0; lane < 64; lane += 63)
                for (int j = 0; j < NVX_REAL_REGION / (64 * spt); j++) {
                    const int at = NVX_REAL_HALO_AT + wave * NVX_REAL_REGION + lane * spt + j * 64 * spt;
                    CHECK(at >= NVX_REAL_HALO_AT && at + spt <= NVX_REAL_LDS_ENTRIES && (at * 2) % (spt * 2) == 0, "staging at %d", at);
                }

    // the kernel's walk (output by output, unless the call is too long for that)
    std::vector<uint8_t> reached(walk ? n : 0, 0);
    for (int x = 0; x < chunks && n; x++) {
        const int tile0 = x * a.tiles_per_chunk, tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
        CHECK(tile0 < tile1, AT ": chunk %d is empty", ATV, x);
        for (int tile = tile0; tile < tile1; tile++) {
            const bool full = (u128)(tile + 1) * T <= n;
            if (!full) CHECK(tile == a.tiles - 1, AT ": tile %d is not whole and not the last", ATV, tile);
            const long tbase = (long)tile * T;
            CHECK(tbase < (long)n, AT ": tile %d starts behind the call", ATV, tile);
            // the halo: the state row in front of the first tile, the input in front of the others
            if (tbase) CHECK(tbase - NVX_REAL_HISTORY >= 0 && tbase - 1 < (long)n, AT ": the halo of tile %d", ATV, tile);
            for (int g = 0; walk && g < 4; g++)
                for (int tid = 0; tid < NVX_REAL_THREADS; tid++) {
                    const int i0 = (g * NVX_REAL_THREADS + tid) * 4;
                    // the odd samples: 16 words from an 8-byte aligned entry; the even ones: 3 words
                    const int po = NVX_REAL_HALO_AT - NVX_REAL_HISTORY + i0, pe = NVX_REAL_HALO_AT - NVX_REAL_K - 1 + i0;
                    CHECK(po >= 0 && (po * 2) % 8 == 0 && po + 32 <= NVX_REAL_LDS_ENTRIES && pe >= 0 && (pe * 2) % 4 == 0 && pe + 6 <= NVX_REAL_LDS_ENTRIES, "group at %d", i0);
                    // output r reaches over pairs i0 + r - 27 .. i0 + r, which lie at entries po + 1 + r .. po + 28 + r
                    CHECK(po + 1 == NVX_REAL_HALO_AT + i0 - (NVX_REAL_HISTORY - 1) && pe + 1 == NVX_REAL_HALO_AT + i0 - NVX_REAL_K, "reach at %d", i0);
                    CHECK((tbase + i0) % 4 == 0, "a group's first output");
                    for (int r = 0; r < 4; r++)
                        if (tbase + i0 + r < (long)n) reached[tbase + i0 + r]++;
                        else CHECK(!full, AT ": a whole tile reaches behind the call", ATV);
                }
        }
    }
    for (size_t j = 0; walk && j < n; j++) CHECK(reached[j] == 1, AT ": output %zu reached %d times", ATV, j, reached[j]);
    // the state's writer: pair n - 28 + t of the call, from the input or from the row read
    for (int t = 0; t < NVX_REAL_HISTORY; t++) {
        const long at = (long)a.n - NVX_REAL_HISTORY + t;
        if (at >= 0) CHECK(at < (long)n, AT ": state pair %d", ATV, t);
        else CHECK(NVX_REAL_HISTORY + at >= 0 && NVX_REAL_HISTORY + at < NVX_REAL_STATE_WORDS, AT ": state pair %d", ATV, t);
    }

    // 16-byte stores only where every row is 16-byte aligned
    bool aligned = true;
    for (int s = 0; s < n_streams; s++) aligned = aligned && ((u128)out_base + ((u128)s * pitch_out + out_first) * 4) % 16 == 0;
    CHECK((a.out_vec != 0) == aligned, AT ": out_vec %d for base %#zx, pitch %zu, first %zu, %d streams", ATV, a.out_vec, (size_t)out_base, pitch_out,
          out_first, n_streams);
}

int main(void)
{
    const size_t T = NVX_REAL_TILE;
    const size_t outputs[] = { 0, 1, 2, 27, 28, 29, 4095, 4096, 4097, 3 * T + 6, 4 * T, 4 * T + 1, 8 * T, 8 * T + 1, 12 * T + 5, 40 * T + 13107 };
    const uint64_t positions[] = { 0, 2, 4, 54, 56, 58, 8192, ((uint64_t)1 << 32) - 1000, ((uint64_t)1 << 40) + 6, ((uint64_t)1 << 62) - 2 - 100 * T };
    const int chunkings[] = { 0, 1, 2, 3, 683, 2048 };
    for (size_t n : outputs)
        for (uint64_t consumed : positions)
            for (int wanted : chunkings) {
                CHECK(!((consumed + 2 * n) >> 62), "position %llu + %zu", (unsigned long long)consumed, 2 * n);
                check_case(consumed, 2 * n, wanted, (int)(n & 1), 3, 0x7000000, 3000004, 8);
            }
    // a stream spread over many chunks, and the longest call (not walked output by output)
    check_case(54, 2 * 600 * T, 2048, 0, 1, 0x7000000, 0, 0);
    check_case(2, NVX_REAL_MAX_IN, 2048, 1, 1, 0x7000000, 0, 0, false);
    check_case(2, NVX_REAL_MAX_IN, 1, 1, 1, 0x7000000, 0, 0, false);
    // the alignment of the output rows
    const struct { uintptr_t base; size_t pitch, first; int streams; } OUTS[] = {
        { 0x7000000, 40020, 7, 2 }, { 0x7000000, 40020, 8, 2 }, { 0x7000000, 40021, 8, 2 }, { 0x7000000, 40021, 8, 1 }, { 0x7000004, 40020, 3, 2 },
        { 0x7000004, 40020, 0, 1 }, { 0x7000008, 40022, 2, 1 }, { 0x7000008, 40022, 2, 3 }, { 0x7000000, 0, 0, 1 },
    };
    for (const auto &o : OUTS) check_case(6, 2 * 20007, 1, 0, o.streams, o.base, o.pitch, o.first);
    printf("real launch args ok: %ld checks\n", g_checks);
    return 0;
}
