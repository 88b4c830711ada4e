// AddressSanitizer / LeakSanitizer driver for the life of a handle (navtex_amd/csrc/nvx_api.cpp) without a GPU:
// nvx_create, nvx_destroy, nvx_enable_debug, nvx_reset and nvx_stream_reset run for real over a HIP stand-in that hands
// out host memory, copies and sets synchronously, checks that every copy and set lies inside one live allocation, counts
// what it creates and releases per kind (stream, event, device buffer, pinned buffer) and fails one creating call on
// request.  The kernels are never launched on these paths.
// Checked, for a 252 kS/s handle, raw-rate handles in both stage-0 forms, a push-mode handle and wideband handles with one
// and two inputs and mixed chain masks:
//  (a) create then destroy releases every stream, event and buffer exactly once, the streams last; so with the three
//      debug buffers on, and after they have been switched off again (each made and released once);
//  (b) whichever creating call of nvx_create fails (hipErrorOutOfMemory), the result is NVX_ERR_NOMEM, no handle and
//      nothing left outstanding;
//  (c) with every device buffer filled with a pattern and the per-stream host fields set, nvx_stream_reset(s) leaves the
//      rows of stream s equal, byte for byte, to a fresh handle's and every other byte and field as it was;
//  (d) after the same, nvx_reset leaves every byte of carried state equal to a fresh handle's, and every field too.
// Which bytes a stream owns is written out here from the layouts in nvx_kernels.h, not taken from the library.
// Built by tests/test_sanitizers.py with -fsanitize=address (leaks of the host objects show up at exit).
#include "nvx_handle.h"

#include <map>

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s [%s]\n", __FILE__, __LINE__, #c, g_what); if (++g_bad > 40) exit(1); } } while (0)
static const char *g_what = "";

// ---- the HIP stand-in
enum Kind { STREAM, EVENT, DEV, HOST, NKIND };
static const char *const kind_name[NKIND] = { "stream", "event", "device buffer", "pinned buffer" };
struct Alloc { Kind kind; size_t bytes; };
static std::map<const char *, Alloc> g_live;
static long g_made[NKIND], g_freed[NKIND];
static int g_calls = 0, g_fail_at = 0;       // creating calls so far; the one to fail (1-based, 0 = none)
static bool g_order = false;                 // a single handle is being destroyed: its streams go after everything else

static hipError_t make(Kind k, void **p, size_t bytes)
{
    if (++g_calls == g_fail_at) return hipErrorOutOfMemory;
    char *q = (char *)malloc(bytes ? bytes : 1);
    memset(q, 0x5a, bytes);                  // (what a fresh buffer holds is not anybody's business: not zero)
    g_live[q] = Alloc{ k, bytes };
    g_made[k]++;
    *p = q;
    return hipSuccess;
}
static hipError_t release(Kind k, void *p)
{
    if (!p) { CHECK(k == DEV || k == HOST); return k == DEV || k == HOST ? hipSuccess : hipErrorInvalidValue; }
    auto it = g_live.find((const char *)p);
    if (it == g_live.end() || it->second.kind != k) {
        fprintf(stderr, "%s %p released twice, or as another kind\n", kind_name[k], p);
        g_bad++;
        return hipErrorInvalidValue;
    }
    if (k == STREAM && g_order)
        for (auto &a : g_live) CHECK(a.second.kind == STREAM);
    g_live.erase(it);
    g_freed[k]++;
    free(p);
    return hipSuccess;
}
static void inside(const void *p, size_t bytes)          // [p, p + bytes) lies in one live buffer
{
    auto it = g_live.upper_bound((const char *)p);
    bool ok = it != g_live.begin();
    if (ok) { --it; ok = (it->second.kind == DEV || it->second.kind == HOST) && (const char *)p + bytes <= it->first + it->second.bytes; }
    if (!ok) { fprintf(stderr, "copy or set of %zu bytes at %p outside every buffer\n", bytes, p); g_bad++; exit(1); }
}

hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "stand-in error"; }
hipError_t hipMemGetAddressRange(hipDeviceptr_t *, size_t *, hipDeviceptr_t) { return hipErrorNotSupported; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int) { return make(STREAM, (void **)s, 1); }
hipError_t hipStreamDestroy(hipStream_t s) { return release(STREAM, s); }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned int) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { return make(EVENT, (void **)e, 1); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return make(EVENT, (void **)e, 1); }
hipError_t hipEventDestroy(hipEvent_t e) { return release(EVENT, e); }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
hipError_t hipMalloc(void **p, size_t n) { return make(DEV, p, n); }
hipError_t hipFree(void *p) { return release(DEV, p); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned int) { return make(HOST, p, n); }
hipError_t hipHostFree(void *p) { return release(HOST, p); }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind)
{
    inside(d, n);
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t) { return hipMemcpy(d, s, n, k); }
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t)
{
    inside(d, n);
    memset(d, v, n);
    return hipSuccess;
}
hipError_t hipMemset2DAsync(void *d, size_t pitch, int v, size_t w, size_t rows, hipStream_t s)
{
    for (size_t r = 0; r < rows; r++) hipMemsetAsync((char *)d + r * pitch, v, w, s);
    return hipSuccess;
}
// none of the calls under test launches anything
extern "C" {
hipError_t nvx_launch_wideband_fused(const nvx_wideband_args *, nvx_forms *, hipStream_t) { g_bad++; return hipErrorUnknown; }
hipError_t nvx_launch_cascade(const nvx_cascade_args *, int, int, nvx_forms *, hipStream_t) { g_bad++; return hipErrorUnknown; }
hipError_t nvx_launch_fir3(const nvx_fir3_args *, hipStream_t) { g_bad++; return hipErrorUnknown; }
int nvx_front_tile_wgs(const nvx_demod_args *, int) { return 0; }
hipError_t nvx_launch_demod_front(const nvx_demod_args *, hipStream_t) { g_bad++; return hipErrorUnknown; }
hipError_t nvx_launch_demod_fsm(const nvx_demod_args *, hipStream_t) { g_bad++; return hipErrorUnknown; }
int add_message(char *, char *, int) { g_bad++; return 0; }
}

static long outstanding() { return (long)g_live.size(); }

// ---- the handle's buffers by name, and who owns which byte of them
struct Buf { std::string name; char *p; size_t bytes; };
static std::vector<Buf> device_buffers(nvx_handle *h)
{
    std::vector<std::pair<std::string, void *>> v = {
        { "whist0", h->d_whist[0] }, { "whist1", h->d_whist[1] }, { "y2_0", h->d_y2[0] }, { "y2_1", h->d_y2[1] },
        { "y2row", h->d_y2row }, { "masks", h->d_masks }, { "active", h->d_active }, { "cstate0", h->d_cstate[0] },
        { "cstate1", h->d_cstate[1] }, { "y3_0", h->d_y3[0] }, { "y3_1", h->d_y3[1] }, { "dd0", h->d_dd[0] }, { "dd1", h->d_dd[1] },
        { "dphi", h->d_dphi }, { "corr", h->d_corr }, { "csum", h->d_csum }, { "di", h->d_di }, { "fsm_tab", h->d_fsm_tab }, { "words", h->d_words }, { "ties", h->d_ties },
        { "ctrl", h->d_ctrl }, { "in", h->d_in } };
    for (int k = 0; k < RESULT_SLOTS; k++) {
        v.push_back({ "bits" + std::to_string(k), h->res[k].d_bits });
        v.push_back({ "nbits" + std::to_string(k), h->res[k].d_nbits });
        v.push_back({ "part" + std::to_string(k), h->res[k].d_part });
    }
    std::vector<Buf> out;
    for (auto &b : v)
        if (b.second) {
            auto it = g_live.find((const char *)b.second);
            CHECK(it != g_live.end() && it->second.kind == DEV);
            if (it != g_live.end()) out.push_back(Buf{ b.first, (char *)b.second, it->second.bytes });
        }
    return out;
}
static bool table(const std::string &n) { return n == "masks" || n == "active" || n == "y2row" || n == "fsm_tab"; }

// the input stream whose carried state byte `off` of buffer `n` is; -2: the handle's (tie statistics); -1: no carried state
static int owner(const nvx_handle *h, const std::string &n, size_t off)
{
    const int per = h->cfg.wideband ? NVX_WB_SUBBANDS : 1;        // decoded streams per input stream
    if (n == "cstate0" || n == "cstate1") return (int)(off / NVX_CASCADE_STATE_BYTES) / per;
    if (n == "dd0" || n == "dd1") return (int)(off / (NVX_DEMOD_DOUBLES * sizeof(double))) / (2 * per);
    if (n == "di") return (int)(off / sizeof(int) % h->n_slots) / (2 * per);
    if (n == "whist0" || n == "whist1") return (int)(off / (40 * 4));
    if (n == "y2_0" || n == "y2_1") {
        const size_t row = off / (h->y2_pitch * sizeof(double2)), col = off % (h->y2_pitch * sizeof(double2));
        if (col >= NVX_Y2_PREFIX * sizeof(double2)) return -1;
        for (int i = 0; i < h->n_slots; i++) if (h->y2row[i] == (int)row) return i / (2 * per);
        return -1;
    }
    if (n == "ties") return -2;
    return -1;
}
static uint8_t pattern(size_t off) { return (uint8_t)(0x40 + off % 61); }      // never 0x00, 0xff, 0x7f or 0x80

// ---- the host fields a stream carries: set to values no reset leaves
static const unsigned long long G_DIRTY = 5 * NVX_FRAME_Y3;
static void dirty(nvx_handle *h, std::vector<ArrivalClock> &clocks)
{
    for (auto &b : device_buffers(h))
        if (!table(b.name)) for (size_t i = 0; i < b.bytes; i++) b.p[i] = (char)pattern(i);
    for (auto &s : h->slots) { s.bits = "BYB"; s.base = 7; s.polled = 9; }
    for (int s = 0; s < h->n_in; s++) {
        h->parity[s] = 1; h->g0s[s] = G_DIRTY; h->ended[s] = 1;
        h->arrival[s] = &clocks[s]; clocks[s].base = 5;
    }
    if (!h->fill.empty())
        for (int s = 0; s < h->n_in; s++) {
            h->fill[s] = 3; h->active[s] = 0; h->last_push_ns[s] = 1; h->cur[s] = 1;
            h->set_launch[0][s] = 4; h->set_launch[1][s] = 5;
        }
    h->copies_synced = 3;
    *h->h_ties = nvx_tie_stats{ 1, 2, 3, 4 };
    h->diverged = true;
}

static nvx_handle *create(const nvx_config &c)
{
    nvx_handle *h = nullptr;
    const int rc = nvx_create(&c, &h);
    CHECK(rc == NVX_OK && h);
    if (rc != NVX_OK) { fprintf(stderr, "%s\n", nvx_last_error()); exit(1); }
    return h;
}

// the fields of stream s (slots included) are a fresh handle's (`fresh`) or what dirty() left
static void check_stream_fields(const nvx_handle *h, int s, bool fresh, int64_t t0)
{
    const int per = h->cfg.wideband ? NVX_WB_SUBBANDS : 1;
    for (int i = 2 * per * s; i < 2 * per * (s + 1); i++) {
        const Slot &sl = h->slots[i];
        CHECK(fresh ? (sl.bits.empty() && sl.base == 0 && sl.polled == 0) : (sl.bits == "BYB" && sl.base == 7 && sl.polled == 9));
    }
    CHECK(h->g0s[s] == (fresh ? 0 : G_DIRTY));
    CHECK(h->ended[s] == (fresh ? 0 : 1));
    CHECK(h->arrival[s]->base == (fresh ? UINT64_MAX : 5));
    if (!h->fill.empty()) {
        CHECK(h->fill[s] == (fresh ? 0u : 3u));
        CHECK(h->active[s] == (fresh ? 1 : 0));
        CHECK(fresh ? h->last_push_ns[s] >= t0 : h->last_push_ns[s] == 1);
        CHECK(h->cur[s] == 1);                                    // nobody's staging set flips
    }
}

static void lifecycle(const char *what, nvx_config c)
{
    g_what = what;
    const int bad0 = g_bad;
    c.struct_size = sizeof c;
    // (a) everything made is released once, the streams last -- with the debug buffer too
    for (int debug = 0; debug < 3; debug++) {
        std::fill(g_made, g_made + NKIND, 0); std::fill(g_freed, g_freed + NKIND, 0);
        nvx_handle *h = create(c);
        // every device buffer the handle holds is one the byte checks below know by name
        CHECK(device_buffers(h).size() == (size_t)g_made[DEV]);
        const long dev0 = g_made[DEV];
        if (debug) {
            // the three debug buffers (delta-phi, |corr|, class sums) come and go together; asking twice makes nothing more
            CHECK(nvx_enable_debug(h, 1) == NVX_OK && h->d_dphi && h->d_corr && h->d_csum);
            CHECK(nvx_enable_debug(h, 1) == NVX_OK && g_made[DEV] == dev0 + 3);
            CHECK(device_buffers(h).size() == (size_t)(g_made[DEV] - g_freed[DEV]));
        }
        if (debug == 2) {
            CHECK(nvx_enable_debug(h, 0) == NVX_OK && !h->d_dphi && !h->d_corr && !h->d_csum && g_freed[DEV] == 3);
            CHECK(nvx_enable_debug(h, 0) == NVX_OK && g_freed[DEV] == 3);
        }
        g_order = true;
        nvx_destroy(h);
        g_order = false;
        for (int k = 0; k < NKIND; k++) CHECK(g_made[k] == g_freed[k] && g_made[k] > 0);
        CHECK(outstanding() == 0);
    }
    // a failure at any of nvx_enable_debug's three buffers leaves none of them
    for (int k = 1; k <= 3; k++) {
        nvx_handle *h = create(c);
        const long live0 = outstanding();
        g_calls = 0; g_fail_at = k;
        CHECK(nvx_enable_debug(h, 1) == NVX_ERR_NOMEM && !h->d_dphi && !h->d_corr && !h->d_csum && outstanding() == live0);
        g_fail_at = 0;
        nvx_destroy(h);
        CHECK(outstanding() == 0);
    }
    // (b) a failure at every creating call of nvx_create unwinds completely
    g_calls = 0;
    nvx_destroy(create(c));
    const int n_calls = g_calls;
    for (int k = 1; k <= n_calls; k++) {
        g_calls = 0; g_fail_at = k;
        nvx_handle *h = (nvx_handle *)&g_calls;
        CHECK(nvx_create(&c, &h) == NVX_ERR_NOMEM);
        CHECK(h == nullptr);
        CHECK(outstanding() == 0);
    }
    g_fail_at = 0;

    nvx_handle *f = create(c);                                   // the fresh handle the others are held against
    std::vector<Buf> fb = device_buffers(f);
    const int n_in = f->n_in;
    std::vector<ArrivalClock> clocks(n_in);
    // (c) one stream starts anew, the others keep everything
    for (int s = 0; s < n_in; s++) {
        nvx_handle *h = create(c);
        dirty(h, clocks);
        const int64_t t0 = nvx_now_ns();
        CHECK(nvx_stream_reset(h, s) == NVX_OK);
        std::vector<Buf> hb = device_buffers(h);
        CHECK(hb.size() == fb.size());
        for (size_t b = 0; b < hb.size(); b++) {
            CHECK(hb[b].name == fb[b].name && hb[b].bytes == fb[b].bytes);
            const bool tab = table(hb[b].name);
            size_t wrong = 0;
            for (size_t i = 0; i < hb[b].bytes; i++) {
                const uint8_t want = (tab || owner(h, hb[b].name, i) == s) ? (uint8_t)fb[b].p[i] : pattern(i);
                wrong += (uint8_t)hb[b].p[i] != want;
            }
            if (wrong) fprintf(stderr, "stream_reset(%d): %zu bytes of %s\n", s, wrong, hb[b].name.c_str());
            CHECK(wrong == 0);
        }
        for (int t = 0; t < n_in; t++) check_stream_fields(h, t, t == s, t0);
        for (int t = 0; t < n_in; t++) CHECK(h->parity[t] == 1);
        CHECK(h->diverged == (n_in > 1));
        CHECK(h->h_ties->near_ties == 1 && h->copies_synced == 3);
        if (!h->fill.empty()) for (int t = 0; t < n_in; t++) CHECK(h->set_launch[0][t] == 4 && h->set_launch[1][t] == 5);
        nvx_destroy(h);
    }
    // (d) the whole handle starts anew: carried state as fresh, results in flight dropped
    {
        nvx_handle *h = create(c);
        dirty(h, clocks);
        h->launched = h->collected + 2;
        for (auto &r : h->res) r.pending = true;
        h->launch_done_valid = true; h->demod_pending[0] = h->demod_pending[1] = true;
        h->poisoned = true; h->poison_why = "test";
        const int64_t t0 = nvx_now_ns();
        CHECK(nvx_reset(h) == NVX_OK);
        std::vector<Buf> hb = device_buffers(h);
        for (size_t b = 0; b < hb.size(); b++) {
            const bool tab = table(hb[b].name);
            size_t wrong = 0;
            for (size_t i = 0; i < hb[b].bytes; i++) {
                const uint8_t want = (tab || owner(h, hb[b].name, i) != -1) ? (uint8_t)fb[b].p[i] : pattern(i);
                wrong += (uint8_t)hb[b].p[i] != want;
            }
            if (wrong) fprintf(stderr, "reset: %zu bytes of %s\n", wrong, hb[b].name.c_str());
            CHECK(wrong == 0);
        }
        for (int t = 0; t < n_in; t++) check_stream_fields(h, t, true, t0);
        for (int t = 0; t < n_in; t++) CHECK(h->parity[t] == 0);
        CHECK(!h->diverged && !h->poisoned && h->poison_why.empty() && !h->launch_done_valid);
        CHECK(!h->demod_pending[0] && !h->demod_pending[1]);
        CHECK(h->collected == h->launched);
        for (auto &r : h->res) CHECK(!r.pending);
        CHECK(memcmp(h->h_ties, f->h_ties, sizeof(nvx_tie_stats)) == 0);
        CHECK(h->copies_synced == 3);
        if (!h->fill.empty()) for (int t = 0; t < n_in; t++) CHECK(h->set_launch[0][t] == 0 && h->set_launch[1][t] == 0);
        nvx_destroy(h);
    }
    nvx_destroy(f);
    CHECK(outstanding() == 0);
    printf("%-28s %d creating calls, (a)-(d) %s\n", what, n_calls, g_bad == bad0 ? "ok" : "FAILED");
}

int main()
{
    nvx_config c;
    nvx_config_default(&c);
    c.max_frames = 2;
    c.n_streams = 3;
    lifecycle("252 kS/s", c);
    nvx_config r = c;
    r.raw_rate = 1; r.n_streams = 2;
    r.stage0_order = 1; lifecycle("raw rate, stage 0 order 1", r);
    r.stage0_order = 3; lifecycle("raw rate, stage 0 order 3", r);
    nvx_config p = c;
    p.push_mode = 1;
    lifecycle("push mode", p);
    static const uint8_t masks[2 * NVX_WB_SUBBANDS] = { 1, 2, 3, 3, 1, 2, 2, 1, 3, 1, 1, 2, 3, 2, 1, 3 };
    nvx_config w = c;
    w.wideband = 1; w.chain_masks = masks;
    w.n_streams = 1; lifecycle("wideband, one input", w);
    w.n_streams = 2; lifecycle("wideband, two inputs", w);
    if (g_bad) { printf("handle lifecycle FAILED: %d checks\n", g_bad); return 1; }
    printf("handle lifecycle ok\n");
    return 0;
}
