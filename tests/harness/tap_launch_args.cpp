// The channel tap's launch arithmetic (navtex_amd/tap/nvx_tap_plan.h) walked on the host against 128-bit integers, without a
// device: for plans of every form and calls from positions up to 2^62, every output of a call is taken by exactly one thread
// of one tile with the (q, r) of the header's rule; its window lies inside the tile's staged span, starts at a multiple of 4
// samples of it and is met by the row of its offset e; the staged span reads the input only inside [1 - T, n_in) (zeros
// elsewhere); where the plan says its taps are wave-uniform the lanes of a wave share phase and offset; the LDS stays
// within the budget; the mixer's and the pitch's first indices are the positions mod 4096.  Host code only; built with
// -fsanitize=address,undefined and run directly (tests/test_tap.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvx_tap_plan.h"

typedef unsigned __int128 u128;
static long long checks = 0;
#define REQUIRE(cond, ...) do { checks++; if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static void walk(int L, int M, int T, uint64_t consumed, size_t n_in)
{
    nvx_tap_args a = {};
    nvx_tap_fill_shape(L, M, T, &a);
    REQUIRE(a.tile_out == 256 || a.tile_out == 128, "tile %d", a.tile_out);
    REQUIRE(nvx_tap_lds_bytes(&a) <= NVX_TAP_LDS_BUDGET && a.stage_len % 8 == 0, "L %d M %d T %d: %zu bytes", L, M, T, nvx_tap_lds_bytes(&a));
    REQUIRE(a.R % 8 == 0 && a.R >= T + NVX_TAP_OFFSETS - 1 && a.G * 8 == a.R, "R %d", a.R);
    const int tiles = nvx_tap_fill_args(consumed, n_in, &a);
    const u128 before = ((u128)consumed * L + (M - 1)) / M, after = ((u128)(consumed + n_in) * L + (M - 1)) / M;
    REQUIRE((u128)a.n_out == after - before && tiles >= 1 && tiles == (a.n_out ? (a.n_out + a.tile_out - 1) / a.tile_out : 1), "n_out %d tiles %d", a.n_out, tiles);
    REQUIRE(a.n0 == consumed % 4096 && a.m0 == (uint64_t)(before % 4096), "n0 %u m0 %u", a.n0, a.m0);
    std::vector<int> taken((size_t)a.n_out, 0);
    for (int tile = 0; tile < tiles; tile++) {
        uint32_t qt, rt;
        nvx_tap_tile_start(a, (uint32_t)tile, &qt, &rt);
        const u128 pos_t = (before + (u128)tile * a.tile_out) * M;
        REQUIRE((u128)qt + consumed == pos_t / L && rt == (uint32_t)(pos_t % L), "tile %d: q %u r %u", tile, qt, rt);
        const int lo = nvx_tap_stage_first(a, qt);
        REQUIRE((lo & 3) == 0 && lo <= (int)qt - (T - 1), "lo %d", lo);
        // the staged span: what it reads of the input and of the state row
        for (int v = 0; v < a.stage_len; v++) {
            const long long idx = (long long)lo + v;
            if (idx < 0 && idx >= 1 - T) REQUIRE(T - 1 + idx >= 0 && T - 1 + idx < T - 1, "state index %lld", T - 1 + idx);
        }
        int wave_e[4] = { -1, -1, -1, -1 }, wave_r[4] = { -1, -1, -1, -1 };
        for (int tid = 0; tid < a.tile_out; tid++) {
            const int o = nvx_tap_thread_output(a.tile_out, tid);
            REQUIRE(o >= 0 && o < a.tile_out, "o %d", o);
            const uint64_t i = (uint64_t)tile * a.tile_out + o;
            if (i >= (uint64_t)a.n_out) continue;
            taken[i]++;
            const uint32_t pl = rt + (uint32_t)(o * M);
            REQUIRE(pl < ((uint32_t)L << 18) && pl < (1u << 31), "pl %u", pl);
            const uint32_t dq = pl / L, r = pl % L;
            const u128 pos = (before + i) * M;
            REQUIRE((u128)qt + dq + consumed == pos / L && r == (uint32_t)(pos % L), "output %llu", (unsigned long long)i);
            REQUIRE(qt + dq < n_in, "q %u of %zu", qt + dq, n_in);
            const int u0 = (int)(qt + dq) - (T - 1) - lo, e = u0 & 3, ub = u0 - e;
            REQUIRE(u0 >= 0 && ub % 4 == 0 && ub + a.R <= a.stage_len, "window %d + %d of %d", ub, a.R, a.stage_len);
            // entry j of row e meets staged sample ub + j: tap t = T - 1 - (j - e) meets x[q - t]
            REQUIRE(lo + ub + (T - 1 + e) == (int)(qt + dq), "the newest sample");
            if (a.uniform) {
                const int w = tid >> 6;
                if (wave_e[w] < 0) { wave_e[w] = e; wave_r[w] = (int)r; }
                REQUIRE(wave_e[w] == e && wave_r[w] == (int)r && r == 0, "wave %d: e %d r %u", w, e, r);
            }
        }
    }
    for (int i = 0; i < a.n_out; i++) REQUIRE(taken[i] == 1, "output %d taken %d times", i, taken[i]);
}

int main(void)
{
    // (L, M, T) of the case rates and of the plans at the edges of the forms: 2016 S/s (L = 1, M odd, two waves), 2000 S/s
    // (the longest span), 6250 S/s (the largest L), 96 kS/s (the shortest window)
    static const int plans[][3] = { { 1, 21, 602 }, { 1, 126, 3602 }, { 1, 125, 3574 }, { 25, 1008, 1154 }, { 2, 63, 902 }, { 7, 160, 654 }, { 2, 21, 302 },
                                    { 4, 21, 152 }, { 8, 21, 32 }, { 2, 63, 3602 }, { 7, 160, 3602 }, { 1, 21, 3602 }, { 7, 40, 3602 }, { 4, 21, 3602 },
                                    { 1, 63, 3602 }, { 1, 84, 3602 }, { 1, 5, 3602 }, { 1, 3, 64 } };
    static const uint64_t starts[] = { 0, 1, 20, 12345, (1ull << 32) - 1000, (1ull << 40) + 6, (1ull << 62) - 100000 };
    static const size_t calls[] = { 1, 2, 37, 40, 600, 3601, 3602, 20000, 70001 };
    for (const auto &p : plans)
        for (uint64_t s : starts)
            for (size_t n : calls) walk(p[0], p[1], p[2], s, n);
    // the 64-bit divider against the machine's
    for (uint64_t n = 0; n < (1ull << 36); n += 0x3fffffd1ull)
        for (uint32_t d = 1; d <= 1024; d += 7) {
            uint32_t q, r;
            if (n / d >> 32) continue;
            nvx_tap_divmod64(n, d, 36, &q, &r);
            REQUIRE(q == n / d && r == n % d, "%llu / %u", (unsigned long long)n, d);
        }
    printf("tap launch args ok: %lld checks\n", checks);
    return 0;
}
