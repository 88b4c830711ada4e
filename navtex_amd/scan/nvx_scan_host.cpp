// nvx_scan_host.cpp -- the band scan's device entry points (include/navtex_amd_scan.h): argument and span checks, the
// choice of kernel form, HIP-event timing.  The library stands alone: it shares no state with libnavtex_amd.so.
#include <mutex>

#include "nvx_companion.h"
#include "nvx_scan_kernels.h"

static const char NOUN[] = "the scan";

extern "C" const char *nvx_scan_last_error(void) { return nvx_error_text(); }

static struct ScanState {
    std::mutex mu;
    int form = 0;
    nvx_event_timer timer;
    struct { int form; dim3 grid; size_t scratch_bytes; } last = {};        // nvx_scan_debug_last_launch
    int64_t launches = 0;
} g_st;

static const size_t SCRATCH_ROWS_MAX = 16384;       // form 2's frame rows: 256 MB

extern "C" int nvx_scan_set_form(int form)
{
    if (form < 0 || form > 2) { set_error("nvx_scan_set_form: form %d (0, 1 or 2)", form); return NVX_ERR_ARG; }
    std::lock_guard<std::mutex> lk(g_st.mu);
    g_st.form = form;
    return NVX_OK;
}

extern "C" void nvx_scan_timing(int enable) { std::lock_guard<std::mutex> lk(g_st.mu); g_st.timer.enabled = enable != 0; }

extern "C" int nvx_scan_time_stats(double *sum_ms, uint64_t *launches, int reset)
{
    std::lock_guard<std::mutex> lk(g_st.mu);
    return g_st.timer.collect(sum_ms, launches, reset);
}

extern "C" int64_t nvx_scan_debug_last_launch(int *form, int *grid_x, int *grid_y, size_t *scratch_bytes)
{
    std::lock_guard<std::mutex> lk(g_st.mu);
    if (g_st.launches) {
        if (form) *form = g_st.last.form;
        if (grid_x) *grid_x = (int)g_st.last.grid.x;
        if (grid_y) *grid_y = (int)g_st.last.grid.y;
        if (scratch_bytes) *scratch_bytes = g_st.last.scratch_bytes;
    }
    return g_st.launches;
}

static int scan_mode(int raw_rate, int stage0_order, const char *what, int *mode)
{
    if (raw_rate != 0 && raw_rate != 1) { set_error("%s: raw_rate %d (0 or 1)", what, raw_rate); return NVX_ERR_ARG; }
    if (raw_rate ? (stage0_order != 0 && stage0_order != 1 && stage0_order != 3) : (stage0_order != 0 && stage0_order != 1)) {
        set_error("%s: stage0_order %d (1 or 3 at raw rate; 252 kS/s input has no stage 0)", what, stage0_order); return NVX_ERR_ARG;
    }
    *mode = !raw_rate ? NVX_SCAN_MODE_252K : (stage0_order == 3 ? NVX_SCAN_MODE_RAW3 : NVX_SCAN_MODE_RAW1);
    return NVX_OK;
}

extern "C" int nvx_scan_resident(int device, const void *d_iq, size_t pitch_samples, size_t first_frame, int n_frames,
                                 int n_streams, int raw_rate, int stage0_order, void *d_power, void *hip_stream)
{
    const char *what = "nvx_scan_resident";
    int mode = 0;
    int rc = scan_mode(raw_rate, stage0_order, what, &mode); if (rc != NVX_OK) return rc;
    if (!d_iq || !d_power || n_frames < 1 || n_streams < 1 || ((uintptr_t)d_iq & 15) || ((uintptr_t)d_power & 7) || (pitch_samples & 3)) {
        set_error("%s: bad argument (null pointer, no frames or streams, input not 16-byte aligned or pitch not a multiple of 4)", what);
        return NVX_ERR_ARG;
    }
    const size_t frame_len = raw_rate ? NVX_SCAN_FRAME_RAW : NVX_SCAN_FRAME_IN;
    // every stream's last scanned sample, in samples of its row and in bytes of the whole operand: nothing may wrap
    size_t end_frame, row_end, in_bytes, out_bytes;
    if (__builtin_add_overflow(first_frame, (size_t)n_frames, &end_frame) || __builtin_mul_overflow(end_frame, frame_len, &row_end) ||
        !span_bytes((size_t)(n_streams - 1), pitch_samples, row_end, 4, &in_bytes) ||
        !span_bytes((size_t)n_streams, NVX_SCAN_FFT, 0, sizeof(double), &out_bytes)) {
        set_error("%s: the span of %d frames from frame %zu of %d streams at pitch %zu overflows", what, n_frames, first_frame, n_streams, pitch_samples);
        return NVX_ERR_ARG;
    }
    if (n_streams > 1 && row_end > pitch_samples) {
        set_error("%s: frames up to %zu need %zu samples per stream, the pitch is %zu", what, end_frame, row_end, pitch_samples);
        return NVX_ERR_ARG;
    }
    if ((rc = select_device(device, NOUN)) != NVX_OK) return rc;
    if ((rc = check_device_span(d_iq, in_bytes, what, "input")) != NVX_OK) return rc;
    if ((rc = check_device_span(d_power, out_bytes, what, "power rows")) != NVX_OK) return rc;

    nvx_scan_args a{};
    a.iq = (const uint32_t *)d_iq; a.pitch = pitch_samples; a.first_frame = first_frame;
    a.n_frames = n_frames; a.n_streams = n_streams; a.mode = mode; a.power = (double *)d_power;

    int form;
    {
        std::lock_guard<std::mutex> lk(g_st.mu);
        form = g_st.form;
    }
    // a workgroup per stream fills the chip from about two workgroups per CU on; below that the frames are spread out too
    const bool rows_fit = (size_t)n_streams * (size_t)n_frames <= SCRATCH_ROWS_MAX && n_streams <= 65535;
    if (form == 0) form = n_streams >= 512 ? 1 : 2;
    if (form == 2 && !rows_fit) form = 1;

    hipStream_t s = (hipStream_t)hip_stream;
    const size_t scratch_bytes = form == 2 ? (size_t)n_streams * n_frames * NVX_SCAN_FFT * sizeof(double) : 0;
    if (form == 2) HIP_TRY(hipMallocAsync((void **)&a.rows, scratch_bytes, s));
    {
        std::lock_guard<std::mutex> lk(g_st.mu);
        nvx_event_timer::events ev;
        dim3 grid;
        if ((rc = g_st.timer.begin(s, ev)) != NVX_OK) return rc;
        HIP_TRY(nvx_scan_launch(&a, form, s, &grid));
        g_st.last = { form, grid, scratch_bytes };
        g_st.launches++;
        if ((rc = g_st.timer.end(s, ev)) != NVX_OK) return rc;
    }
    if (form == 2) HIP_TRY(hipFreeAsync(a.rows, s));
    return NVX_OK;
}

extern "C" int nvx_scan_iq(int device, const int16_t *iq, size_t n, int raw_rate, int stage0_order, double *power, int *frames_used)
{
    const char *what = "nvx_scan_iq";
    int mode = 0;
    int rc = scan_mode(raw_rate, stage0_order, what, &mode); if (rc != NVX_OK) return rc;
    const size_t frame_len = raw_rate ? NVX_SCAN_FRAME_RAW : NVX_SCAN_FRAME_IN;
    if (!iq || !power || n < frame_len || n / frame_len > 0x7fffffff) {
        set_error("%s: bad argument (null pointer, or fewer samples than one frame of %zu)", what, frame_len);
        return NVX_ERR_ARG;
    }
    const int n_frames = (int)(n / frame_len);
    if ((rc = select_device(device, NOUN)) != NVX_OK) return rc;
    const size_t bytes = (size_t)n_frames * frame_len * 4;
    void *d_iq = nullptr, *d_power = nullptr;
    hipError_t e = hipMalloc(&d_iq, bytes);
    if (e == hipSuccess) e = hipMalloc(&d_power, NVX_SCAN_FFT * sizeof(double));
    if (e != hipSuccess) { (void)hipFree(d_iq); set_error("%s: hipMalloc failed: %s", what, hipGetErrorString(e)); return NVX_ERR_NOMEM; }
    e = hipMemcpy(d_iq, iq, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = nvx_scan_resident(device, d_iq, (size_t)n_frames * frame_len, 0, n_frames, 1, raw_rate, stage0_order, d_power, nullptr);
        if (rc == NVX_OK) e = hipMemcpy(power, d_power, NVX_SCAN_FFT * sizeof(double), hipMemcpyDeviceToHost);   // waits for the null stream
    }
    (void)hipFree(d_iq); (void)hipFree(d_power);
    if (rc != NVX_OK) return rc;
    if (e != hipSuccess) { set_error("%s: copy failed: %s", what, hipGetErrorString(e)); return NVX_ERR_HIP; }
    if (frames_used) *frames_used = n_frames;
    return NVX_OK;
}
