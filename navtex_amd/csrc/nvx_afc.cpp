// nvx_afc.cpp -- automatic frequency control (include/navtex_amd_afc.h): the group forms -- the member that owns the
// stream, with its own index of it, as nvx_tune.cpp routes -- and the law's host twin.  The handle forms are in nvx_api.cpp,
// the update kernel in navtex_amd/afc/nvx_afc.hip.
#include "nvx_handle.h"
#include "navtex_amd_afc.h"

// (member handle, its stream index) of global stream s; NVX_ERR_STATE for a wideband group (its members refuse tracking)
static int route(nvx_group *g, int s, const char *what, nvx_handle **h, int *local)
{
    nvx_handle *h0 = nullptr;
    if (!g || s < 0 || nvx_group_member(g, 0, nullptr, nullptr, nullptr, &h0) != NVX_OK || !h0) {
        nvx_set_error("%s: null group or bad stream", what); return NVX_ERR_ARG;
    }
    if (h0->cfg.wideband) { nvx_set_error("%s: not for wideband groups", what); return NVX_ERR_STATE; }
    const int mi = nvx_group_member_of(g, s);
    int first = 0;
    if (mi < 0 || nvx_group_member(g, mi, nullptr, &first, nullptr, h) != NVX_OK) { nvx_set_error("%s: stream %d is not in the group", what, s); return NVX_ERR_ARG; }
    *local = s - first;
    return NVX_OK;
}

extern "C" int nvx_group_afc_enable(nvx_group *g, int s, int chain, const nvx_afc_config *cfg)
{
    nvx_handle *h = nullptr; int local = 0;
    const int rc = route(g, s, "nvx_group_afc_enable", &h, &local);
    return rc != NVX_OK ? rc : nvx_afc_enable(h, local, chain, cfg);
}

extern "C" int nvx_group_afc_disable(nvx_group *g, int s, int chain, int keep)
{
    nvx_handle *h = nullptr; int local = 0;
    const int rc = route(g, s, "nvx_group_afc_disable", &h, &local);
    return rc != NVX_OK ? rc : nvx_afc_disable(h, local, chain, keep);
}

extern "C" int nvx_group_afc_read(nvx_group *g, int s, int chain, nvx_afc_status *out)
{
    nvx_handle *h = nullptr; int local = 0;
    const int rc = route(g, s, "nvx_group_afc_read", &h, &local);
    return rc != NVX_OK ? rc : nvx_afc_read(h, local, chain, out);
}

extern "C" int nvx_group_afc_trace(nvx_group *g, int s, int chain, int32_t *k, size_t cap)
{
    nvx_handle *h = nullptr; int local = 0;
    const int rc = route(g, s, "nvx_group_afc_trace", &h, &local);
    return rc != NVX_OK ? rc : nvx_afc_trace(h, local, chain, k, cap);
}

// host-callable copy of the law the update kernel runs (nvx_afc_law.h), for tests (tests/test_afc.py)
extern "C" __attribute__((visibility("default"))) int nvx_afc_step_host(int gain_shift, int max_step, int range_k, int min_samples, double contrast_min,
        int kc, int k0, int k1, unsigned samples, unsigned b_samples, double sum_dphi_b, double sum_dphi_y, double sum_mf_hi, double sum_mf_lo, unsigned *flags)
{
    nvx_afc_par p{};
    p.track = 1; p.kc = kc; p.gain_shift = gain_shift; p.max_step = max_step; p.range_k = range_k; p.min_samples = min_samples;
    p.contrast_min = contrast_min;
    unsigned f = 0;
    const int k2 = nvx_afc_step(&p, k0, k1, samples, b_samples, sum_dphi_b, sum_dphi_y, sum_mf_hi, sum_mf_lo, &f);
    if (flags) *flags = f;
    return k2;
}
