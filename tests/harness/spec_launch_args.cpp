// nvx_spec_fill_args (navtex_amd/spec/nvx_spec_plan.h) walked without a device, against 128-bit integers and a ring that
// holds the absolute index of the sample in every word: which samples a line reads from the ring and which from the call's
// input, the lines a call completes, what it leaves in the ring, at positions up to 2^62 and for calls cut at and next to H,
// N, a line's hop and a line's span.  A stand-alone program: tests/test_spec.py builds it under ASan + UBSan and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvx_spec_plan.h"

typedef unsigned __int128 u128;
static const uint64_t SILENCE = ~(uint64_t)0;
static long long checks = 0;
#define CHECK(cond)                                                                                             \
    do {                                                                                                        \
        checks++;                                                                                               \
        if (!(cond)) { printf("FAILED %s:%d: %s (n_log2 %d avg %d consumed %llu n_in %zu)\n", __FILE__, __LINE__, #cond, n_log2, avg, (unsigned long long)consumed, n_in); exit(1); } \
    } while (0)

// the lines complete at p, by the header's words: line l spans (A + 1) H samples from l A H on
static u128 lines_by_definition(u128 p, u128 hop, u128 span)
{
    u128 lo = 0, hi = p / hop + 2;                          // the largest l with (l - 1) hop + span <= p
    while (lo < hi) {
        const u128 mid = (lo + hi + 1) / 2;
        if ((mid - 1) * hop + span <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

static void walk(int n_log2, int avg, uint64_t start, const std::vector<size_t> &cuts)
{
    const uint64_t H = (uint64_t)1 << (n_log2 - 1), hop = (uint64_t)avg * H, span = hop + H;
    uint64_t consumed = start;
    size_t n_in = 0;
    CHECK((uint64_t)NVX_SPEC_SPAN(n_log2, avg) == span && (uint64_t)NVX_SPEC_HOP(n_log2, avg) == hop);
    CHECK(NVX_SPEC_RING_WORDS(n_log2, avg) >= span && NVX_SPEC_RING_WORDS(n_log2, avg) % 4 == 0);
    std::vector<uint64_t> ring(span, SILENCE);               // as after a reset at `start`: silence in front of it
    for (size_t cut : cuts) {
        n_in = cut;
        nvx_spec_args a;
        nvx_spec_fill_args(consumed, n_in, n_log2, avg, &a);
        const u128 before = lines_by_definition(consumed, hop, span), after = lines_by_definition((u128)consumed + n_in, hop, span);
        CHECK(nvx_spec_lines_at(consumed, n_log2, avg) == (uint64_t)before && nvx_spec_lines_at(consumed + n_in, n_log2, avg) == (uint64_t)after);
        CHECK(a.lines >= 0 && (u128)a.lines == after - before && a.n_in == (int)n_in && a.span == (int)span);
        CHECK(a.carried >= 0 && (uint64_t)a.carried < span && (u128)a.carried == (u128)consumed - before * hop);
        CHECK(a.ring0 < span && (u128)a.ring0 == (before * hop) % span);
        // every sample of the first two and the last two lines the call completes
        for (int j = 0; j < a.lines; j++) {
            if (j >= 2 && j < a.lines - 2) continue;
            const int64_t g_line = (int64_t)j * (int64_t)hop - a.carried;
            for (uint64_t o = 0; o < span; o++) {
                const int64_t g = g_line + (int64_t)o;
                const u128 absolute = (before + (u128)j) * hop + o;
                if (g >= 0) {
                    CHECK((uint64_t)g < n_in && (u128)consumed + (u128)g == absolute);
                } else {
                    uint32_t at = a.ring0 + (uint32_t)(a.carried + g);
                    if (at >= (uint32_t)a.span) at -= (uint32_t)a.span;
                    CHECK(a.carried + g >= 0 && at < span && (u128)at == absolute % span);
                    CHECK(ring.at(at) == (absolute < start ? SILENCE : (uint64_t)absolute));
                }
            }
        }
        // what the call leaves behind its last complete line
        CHECK(a.keep >= 0 && (uint64_t)a.keep < span && (u128)a.keep == (u128)consumed + n_in - after * hop);
        CHECK(a.keep_first >= 0 && (size_t)a.keep_first <= n_in && ((size_t)a.keep < n_in ? (size_t)a.keep_first == n_in - (size_t)a.keep : a.keep_first == 0));
        CHECK(a.keep_ring < span && (u128)a.keep_ring == ((u128)consumed + (u128)a.keep_first) % span);
        const int n = a.n_in - a.keep_first;
        CHECK(n >= 0 && (uint64_t)n < span + (n_in == 0));
        for (int j = 0; j < n; j++) {
            uint32_t at = a.keep_ring + (uint32_t)j;
            if (at >= (uint32_t)a.span) at -= (uint32_t)a.span;
            ring.at(at) = consumed + (uint64_t)a.keep_first + (uint64_t)j;
        }
        consumed += n_in;
        for (u128 s = after * hop; s < consumed; s++) CHECK(ring.at((size_t)(s % span)) == (s < start ? SILENCE : (uint64_t)s));
    }
}

int main()
{
    const uint64_t starts[] = { 0, 1, 127, ((uint64_t)1 << 32) - 1000, ((uint64_t)1 << 40) + 5, ((uint64_t)1 << 62) - ((uint64_t)1 << 31) };
    const int plans[][2] = { { 8, 1 }, { 8, 2 }, { 8, 5 }, { 8, 512 }, { 9, 3 }, { 10, 4 }, { 11, 8 }, { 11, 1 }, { 12, 3 }, { 12, 8 }, { 12, 32 } };
    srand(7);
    for (const auto &plan : plans)
        for (uint64_t start : starts) {
            const size_t H = (size_t)1 << (plan[0] - 1), N = 2 * H, hop = (size_t)plan[1] * H, span = hop + H;
            std::vector<size_t> cuts = { H - 1, 1, 0, N, hop + 1, 0, 1, H, H + 1, N - 1, N + 1, hop - 1, hop, span - 1, span, span + 1, 3 * span + 7, 5 * hop };
            for (int k = 0; k < 12; k++) cuts.push_back((size_t)rand() % (2 * span));
            if (plan[1] <= 8) cuts.push_back(40 * hop + 3);
            walk(plan[0], plan[1], start, cuts);
        }
    // the longest call at the highest position the library takes
    walk(8, 1, ((uint64_t)1 << 62) - ((uint64_t)1 << 30) - 1, { (size_t)1 << 30 });
    walk(12, 16, ((uint64_t)1 << 33) + 12345, { (size_t)1 << 30, 1 });
    printf("spec launch args ok: %lld checks\n", checks);
    return 0;
}
