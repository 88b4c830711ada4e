// zoom_launch_args.cpp -- the zoom bank's launch arithmetic (navtex_amd/zoom/nvx_zoom_plan.h) without a device: for every k,
// a list of positions, call lengths around D, H, a tile and a chunk, and chunkings, nvx_zoom_fill_args' numbers against direct
// arithmetic in 128-bit integers.  The kernel's walk over chunks, warm-up blocks, blocks, stages and groups of four outputs is
// restated: every output of the call lies in exactly one group of one tile of one chunk; the window of input samples an
// output depends on lies inside the state row plus the call, and inside what its chunk has walked; a block's loads touch
// the state row, the call's input or nothing; every LDS access of the mix, the stages and the carry stays inside its plane
// and the planes inside the launch's LDS; the state's writer takes every sample from the input or from the row read; and
// where out_vec is set every row of the output is 16-byte aligned.
// Built with -fsanitize=address,undefined by tests/test_zoom.py; no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvx_zoom_plan.h"

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

#define AT "k %d, consumed %llu, %zu samples, %d chunks wanted"
#define ATV k, (unsigned long long)consumed, n_in, wanted

// the LDS of one launch: every plane inside its zoom's entries, the zooms inside the dynamic part, all of it inside a workgroup's
static void check_lds(int k, int Z)
{
    const int B = NVX_ZOOM_BLOCK;
    CHECK(NVX_ZOOM_LDS_STATIC == 4096 * 4 + B * 4 && NVX_ZOOM_LDS_STATIC + NVX_ZOOM_LDS_DYNAMIC(k, Z) <= NVX_ZOOM_LDS_MAX, "k %d, %d zooms: the LDS", k, Z);
    long at = 0;
    for (int s = 1; s <= k; s++) {
        CHECK(NVX_ZOOM_STAGE_AT(s) == at && at % 4 == 0 && NVX_ZOOM_PLANE(s) % 4 == 0 && NVX_ZOOM_PLANE(s) == NVX_ZOOM_LINE_AT + (B >> s), "k %d: stage %d at %ld", k, s, at);
        at += 4 * NVX_ZOOM_PLANE(s);
    }
    CHECK(NVX_ZOOM_ZOOM_ENTRIES(k) == at && (size_t)Z * at * 2 == NVX_ZOOM_LDS_DYNAMIC(k, Z), "k %d: %ld entries a zoom", k, at);
    // the mix: thread tid writes one word at entry LINE_AT + 2 tid of each plane of stage 1
    for (int tid = 0; tid < NVX_ZOOM_THREADS; tid += NVX_ZOOM_THREADS - 1)
        CHECK(NVX_ZOOM_LINE_AT + 2 * tid + 2 <= NVX_ZOOM_PLANE(1) && tid * 4 + 4 <= B, "the mix of thread %d", tid);
    // the stages: groups of four outputs; the reads of a group, and the words it writes into the next stage's planes
    for (int s = 1; s <= k; s++) {
        const int outs = B >> s, log2_groups = 8 - s, plane = NVX_ZOOM_PLANE(s);
        CHECK((1 << log2_groups) * 4 == outs, "stage %d: %d outputs", s, outs);
        std::vector<int> seen((size_t)Z * outs, 0);
        for (int w = 0; w < (Z << log2_groups); w++) {
            const int z = w >> log2_groups, i0 = (w & ((1 << log2_groups) - 1)) * 4;
            const int po = NVX_ZOOM_LINE_AT - NVX_REAL_HISTORY + i0, pe = NVX_ZOOM_LINE_AT - NVX_REAL_K - 1 + i0;
            CHECK(z < Z && po >= 0 && (po * 2) % 8 == 0 && po + 32 <= plane && pe >= 0 && (pe * 2) % 4 == 0 && pe + 6 <= plane, "stage %d: group at %d", s, i0);
            // output r reaches over the odd samples of pairs i0 + r - 27 .. i0 + r, entries po + 1 + r .. po + 28 + r, and has its
            // centre at pair i0 + r - 13, entry pe + 1 + r
            CHECK(po + 1 == NVX_ZOOM_LINE_AT + i0 - 27 && pe + 1 == NVX_ZOOM_LINE_AT + i0 - 13, "stage %d: reach at %d", s, i0);
            if (s < k) CHECK(NVX_ZOOM_LINE_AT + i0 / 2 + 2 <= NVX_ZOOM_PLANE(s + 1) && (i0 / 2) % 2 == 0, "stage %d: the words of group %d", s, i0);
            for (int r = 0; r < 4; r++) seen[(size_t)z * outs + i0 + r]++;
        }
        for (int v : seen) CHECK(v == 1, "stage %d: an output computed %d times", s, v);
    }
    // the carry: a thread per plane, all different, source and destination inside the plane
    CHECK(Z * k * 4 <= NVX_ZOOM_THREADS, "a thread per plane");
    std::vector<int> planes((size_t)Z * NVX_ZOOM_ZOOM_ENTRIES(k), 0);
    for (int tid = 0; tid < Z * k * 4; tid++) {
        const int p = tid & 3, q = tid >> 2, cz = q / k, cs = q - cz * k + 1;
        const long first = (long)cz * NVX_ZOOM_ZOOM_ENTRIES(k) + NVX_ZOOM_STAGE_AT(cs) + p * NVX_ZOOM_PLANE(cs);
        CHECK(cz < Z && cs >= 1 && cs <= k && first + NVX_ZOOM_PLANE(cs) <= (long)planes.size() && planes[first] == 0, "the plane of thread %d", tid);
        planes[first] = 1;
        CHECK(NVX_ZOOM_PLANE(cs) - NVX_REAL_HISTORY >= NVX_ZOOM_LINE_AT - NVX_REAL_HISTORY && (NVX_ZOOM_PLANE(cs) - NVX_REAL_HISTORY) % 2 == 0, "the carry of stage %d", cs);
    }
}

static void check_case(int k, uint64_t consumed, size_t n_in, int wanted, int n_inputs, int Z, uintptr_t out_base, size_t pitch_out, size_t out_first,
                       bool walk = true)
{
    static uint32_t state[2][NVX_ZOOM_STATE_WORDS(NVX_ZOOM_MAX_LOG2) * 3];
    static const char in[16] = { 0 };
    static const int kz[24] = { 0 };
    static const uint32_t table[1] = { 0 };
    nvx_zoom_args a;
    const int chunks = nvx_zoom_fill_args(consumed, in, 12345, n_in, (uint32_t *)out_base, pitch_out, out_first, n_inputs, Z, k, state[0], state[1], kz, table,
                                          wanted, &a);
    const long B = NVX_ZOOM_BLOCK, D = 1L << k, T = NVX_ZOOM_TILE(k), H = NVX_ZOOM_HISTORY(k);
    // what is handed through
    CHECK(a.in == in && a.pitch_in == 12345 && a.out == (uint32_t *)out_base && a.pitch_out == pitch_out && a.out_first == out_first, AT ": operands", ATV);
    CHECK(a.state_in == state[0] && a.state_out == state[1] && a.kz == kz && a.table == table && a.log2_decim == k && a.n_zooms == Z, AT ": state", ATV);
    CHECK(n_in % D == 0 && (u128)a.n_in == n_in && (u128)a.n_out * D == n_in && a.n_out >= 0, AT ": %d outputs", ATV, a.n_out);
    CHECK(a.hist == H && H == 53 * (D - 1) && T * D == B, AT ": the history", ATV);
    CHECK(a.n0 < 4096 && (u128)a.n0 == (u128)consumed % 4096, AT ": n0 %u", ATV, a.n0);
    const long n = (long)n_in, n_out = a.n_out;

    // tiles and chunks; the warm-up covers the history
    CHECK((u128)a.tiles * B >= n_in && (n == 0 || (u128)(a.tiles - 1) * B < n_in), AT ": %d tiles", ATV, a.tiles);
    CHECK(a.warm_tiles == NVX_ZOOM_WARM(k) && (long)a.warm_tiles * B >= H && (long)(a.warm_tiles - 1) * B < H, AT ": %d warm-up tiles", ATV, a.warm_tiles);
    CHECK(chunks >= 1 && chunks <= (wanted < 1 ? 1 : wanted) && a.tiles_per_chunk >= 1, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    if (n) CHECK((long)chunks * a.tiles_per_chunk >= a.tiles && (long)(chunks - 1) * a.tiles_per_chunk < a.tiles, AT ": %d chunks of %d tiles", ATV, chunks, a.tiles_per_chunk);
    if (chunks > 1) CHECK(a.tiles_per_chunk >= NVX_ZOOM_MIN_CHUNK_WARMS * a.warm_tiles, AT ": a short chunk", ATV);
    if (wanted <= 1 && n) CHECK(chunks == 1 && a.tiles_per_chunk == a.tiles, AT ": one chunk", ATV);
    CHECK((u128)(a.tiles + a.warm_tiles) * B < ((u128)1 << 31), AT ": the kernel counts in int", ATV);

    // the kernel's walk (output by output, unless the call is too long for that)
    std::vector<uint8_t> reached(walk ? n_out : 0, 0);
    for (int x = 0; x < chunks && n; x++) {
        const int tile0 = x * a.tiles_per_chunk, tile1 = tile0 + a.tiles_per_chunk < a.tiles ? tile0 + a.tiles_per_chunk : a.tiles;
        CHECK(tile0 < tile1, AT ": chunk %d is empty", ATV, x);
        const long walked_from = (long)(tile0 - a.warm_tiles) * B;
        for (int tile = tile0 - a.warm_tiles; tile < tile1; tile++) {
            const long base = (long)tile * B;
            CHECK(base < n, AT ": tile %d starts behind the call", ATV, tile);
            // the loads: a group of 4 or 8 samples is whole inside the call, or read sample by sample from the call, the state
            // row, or not at all
            for (int spt = 4; spt <= 8 && walk; spt += 4)
                for (int tid = 0; tid < B / spt; tid++) {
                    const long s0 = base + (long)tid * spt;
                    CHECK(s0 % spt == 0 || s0 < 0, AT ": a group's first sample %ld", ATV, s0);
                    if (s0 >= 0 && s0 + spt <= n) continue;
                    for (int t = 0; t < spt; t++) {
                        const long i = s0 + t;
                        if (i >= 0) continue;               // read where i < n
                        if (i >= -H) CHECK(H + i >= 0 && H + i < NVX_ZOOM_STATE_WORDS(k), AT ": state word %ld", ATV, H + i);
                    }
                }
            if (tile < tile0) continue;
            // the last stage's groups: the outputs stored
            for (int w = 0; walk && w < (1 << (8 - k)); w++) {
                const long m0 = (long)tile * T + w * 4;
                CHECK(m0 % 4 == 0, "a group's first output");
                for (int r = 0; r < 4; r++) {
                    const long m = m0 + r;
                    if (m >= n_out) continue;
                    reached[m]++;
                    // what output m depends on: samples D m - H .. D m + D - 1
                    const long lo = D * m - H, hi = D * m + D - 1;
                    CHECK(lo >= -H && hi < n, AT ": output %ld reaches outside the state and the call", ATV, m);
                    CHECK(lo >= walked_from && hi < base + B && hi >= base, AT ": output %ld reaches outside what chunk %d walked", ATV, m, x);
                }
            }
        }
    }
    for (long j = 0; walk && j < n_out; j++) CHECK(reached[j] == 1, AT ": output %ld reached %d times", ATV, j, reached[j]);
    // the state's writer: sample n - H + j of the call, from the input or from the row read
    for (long j = 0; j < H; j++) {
        const long at = n - H + j;
        if (at >= 0) CHECK(at < n, AT ": state sample %ld", ATV, j);
        else CHECK(n + j >= 0 && n + j < NVX_ZOOM_STATE_WORDS(k), AT ": state sample %ld", ATV, j);
    }

    // 16-byte stores only where every row is 16-byte aligned
    bool aligned = true;
    for (int s = 0; s < n_inputs * Z; s++) aligned = aligned && ((u128)out_base + ((u128)s * pitch_out + out_first) * 4) % 16 == 0;
    CHECK((a.out_vec != 0) == aligned, AT ": out_vec %d for base %#zx, pitch %zu, first %zu, %d rows", ATV, a.out_vec, (size_t)out_base, pitch_out,
          out_first, n_inputs * Z);
}

int main(void)
{
    const int chunkings[] = { 0, 1, 2, 3, 683, 1024 };
    for (int k = NVX_ZOOM_MIN_LOG2; k <= NVX_ZOOM_MAX_LOG2; k++) {
        for (int Z = 1; Z <= NVX_ZOOM_MAX_ZOOMS; Z++) check_lds(k, Z);
        const size_t D = (size_t)1 << k, T = NVX_ZOOM_TILE(k), H = NVX_ZOOM_HISTORY(k), C = (size_t)NVX_ZOOM_MIN_CHUNK_WARMS * NVX_ZOOM_WARM(k) * T;
        // call lengths, in outputs: around D samples, H samples, a tile and a chunk
        const size_t outputs[] = { 0, 1, 2, 3, H / D - 1, H / D, H / D + 1, H / D + 2, T - 1, T, T + 1, 3 * T + 5, 4 * T, C - 1, C, C + 1, 2 * C, 2 * C + 1, 12 * T + 5,
                                   40 * T + 13 };
        const uint64_t positions[] = { 0, D, 4096 - D, 4096, 53 * D, ((uint64_t)1 << 32) - 1000 * D, ((uint64_t)1 << 40) + 6 * D,
                                       ((uint64_t)1 << 62) - D - 100 * NVX_ZOOM_BLOCK };
        for (size_t n : outputs)
            for (uint64_t consumed : positions)
                for (int wanted : chunkings) {
                    CHECK(!((consumed + D * n) >> 62), "position %llu + %zu", (unsigned long long)consumed, D * n);
                    check_case(k, consumed, D * n, wanted, 3, 1 + (int)(n % 8), 0x7000000, 3000004, 8);
                }
        // an input spread over many chunks, and the longest call (not walked output by output)
        check_case(k, 53 * D, 3000 * NVX_ZOOM_BLOCK, 1024, 1, 2, 0x7000000, 3000 * T, 0);
        check_case(k, D, NVX_ZOOM_MAX_IN, 1024, 1, 1, 0x7000000, 0, 0, false);
        check_case(k, D, NVX_ZOOM_MAX_IN, 1, 1, 1, 0x7000000, 0, 0, false);
        // the alignment of the output rows
        const struct { uintptr_t base; size_t pitch, first; int inputs, zooms; } OUTS[] = {
            { 0x7000000, 40020, 7, 2, 1 }, { 0x7000000, 40020, 8, 2, 1 }, { 0x7000000, 40021, 8, 1, 2 }, { 0x7000000, 40021, 8, 1, 1 }, { 0x7000004, 40020, 3, 2, 3 },
            { 0x7000004, 40020, 0, 1, 1 }, { 0x7000008, 40022, 2, 1, 1 }, { 0x7000008, 40022, 2, 3, 1 }, { 0x7000000, 0, 0, 1, 1 },
        };
        for (const auto &o : OUTS) check_case(k, 6 * D, D * 20007, 1, o.inputs, o.zooms, o.base, o.pitch, o.first);
    }
    printf("zoom launch args ok: %ld checks\n", g_checks);
    return 0;
}
