// nvx_afc.hip -- the update kernel of automatic frequency control (include/navtex_amd_afc.h), part of libnavtex_amd.so.
// One lane per chain slot, behind nvx_demod_fsm of launch L on the demodulator's stream: K[L+2] from the slot's record of
// launch L, K[L] and K[L+1] by the law of nvx_afc_law.h, and a note of what it did.  Plain vector loads and stores, no
// atomics, no LDS: the next reader of the array it writes, the cascade of launch L + 2 (one scalar load per unit), is a
// later kernel that waits for the event recorded behind this one.
#include <hip/hip_runtime.h>
#include "nvx_kernels.h"
#include "nvx_afc_law.h"

#define NVX_AFC_THREADS 256

// whether `stream` is among the launch's participants (ascending by stream)
__device__ __forceinline__ bool afc_took_part(const nvx_part *part, int n_part, int stream)
{
    int lo = 0, hi = n_part;                             // the first entry with .stream >= stream lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (part[mid].stream < stream) lo = mid + 1; else hi = mid;
    }
    return lo < n_part && part[lo].stream == stream;
}

__global__ __launch_bounds__(NVX_AFC_THREADS) void nvx_afc_update(nvx_afc_args a)
{
    const int slot = (int)(blockIdx.x * NVX_AFC_THREADS + threadIdx.x);
    if (slot >= a.n_slots) return;
    const nvx_afc_par p = a.par[slot];
    const int k0 = a.k_rw[slot], k1 = a.k_next[slot];
    const bool part = a.part ? afc_took_part(a.part, a.n_part, slot >> 1) : true;
    unsigned flags = (p.track ? NVX_AFC_F_TRACK : 0u) | (part ? NVX_AFC_F_PART : 0u);
    int k2 = k1;
    if (p.track && part) {
        const nvx_sig_rec r = a.sig[slot];
        unsigned f;
        k2 = nvx_afc_step(&p, k0, k1, r.samples, r.b_samples, r.sum_dphi_b, r.sum_dphi_y, r.sum_mf_hi, r.sum_mf_lo, &f);
        flags |= f;
    }
    a.k_rw[slot] = k2;
    nvx_afc_note n;
    n.k = k0; n.step = (short)(k2 - k1); n.flags = (unsigned short)flags;
    a.note[slot] = n;
}

extern "C" hipError_t nvx_launch_afc_update(const nvx_afc_args *a, hipStream_t s)
{
    if (a->n_slots < 1 || !a->sig || !a->par || !a->k_rw || !a->k_next || !a->note || a->k_rw == a->k_next) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nvx_afc_update, dim3((unsigned)((a->n_slots + NVX_AFC_THREADS - 1) / NVX_AFC_THREADS)), dim3(NVX_AFC_THREADS), 0, s, *a);
    return hipGetLastError();
}
