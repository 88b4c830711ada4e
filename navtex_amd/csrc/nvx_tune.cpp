// nvx_tune.cpp -- the group form of carrier tuning (include/navtex_amd_tune.h): the member that owns the stream, with its
// own index of it, through the public group calls.  The handle form is in nvx_api.cpp.
#include "nvx_handle.h"
#include "navtex_amd_tune.h"

// (member handle, its stream index) of global stream s; NVX_ERR_STATE for a wideband group (its members refuse tuning)
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

extern "C" int nvx_group_set_carrier(nvx_group *g, int s, int chain, double offset_hz, double *applied_hz)
{
    nvx_handle *h = nullptr; int local = 0;
    const int rc = route(g, s, "nvx_group_set_carrier", &h, &local);
    return rc != NVX_OK ? rc : nvx_set_carrier(h, local, chain, offset_hz, applied_hz);
}

extern "C" int nvx_group_get_carrier(nvx_group *g, int s, int chain, double *offset_hz, int *reference_mixer)
{
    nvx_handle *h = nullptr; int local = 0;
    const int rc = route(g, s, "nvx_group_get_carrier", &h, &local);
    return rc != NVX_OK ? rc : nvx_get_carrier(h, local, chain, offset_hz, reference_mixer);
}
