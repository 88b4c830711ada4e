/* nvx_spec_plan.h -- what the spectrum monitor's host side (nvx_spec_host.cpp) and its kernels (nvx_spec.hip) share: the
 * kernels' arguments, the layout of a row's survey and ring, the launch arithmetic (nvx_spec_fill_args, a pure function:
 * tests/harness/spec_launch_args.cpp walks it without a device), and the tests' three hooks.  Internal. */
#ifndef NVX_SPEC_PLAN_H
#define NVX_SPEC_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "navtex_amd_spec.h"
#include "nvx_stream_plan.h"

#define NVX_SPEC_MAX_IN (1u << 30)          /* samples per call and row */
#define NVX_SPEC_FOLD_THREADS 256
#define NVX_SPEC_CARRY_THREADS 256
#define NVX_SPEC_SCRATCH_BYTES ((size_t)1 << 30)     /* the scratch rows of a launch stay below this: a call's lines go in batches */
/* A row's survey: SP, SC.re, SC.im, [N] doubles each, in the order of an output line.  Its line count lies in an array of
 * its own.  A row's ring: (A + 1) H packed words (I in the low half), rounded up to a multiple of four; sample n lies at
 * word n mod (A + 1) H. */
#define NVX_SPEC_SURVEY_WORDS(n) (3 * (size_t)(n))
#define NVX_SPEC_SPAN(n_log2, avg) (((avg) + 1) << ((n_log2) - 1))
#define NVX_SPEC_HOP(n_log2, avg) ((avg) << ((n_log2) - 1))
#define NVX_SPEC_RING_WORDS(n_log2, avg) ((size_t)((NVX_SPEC_SPAN(n_log2, avg) + 3) & ~3))
/* A row's configuration for one call, in uint32 words: flags, and how many of the call's first lines do not count for the
 * survey (they begin in front of its restart). */
#define NVX_SPEC_CFG_WORDS 2
#define NVX_SPEC_ROW_RESTART 1u             /* the survey starts anew with this call */

#ifdef __cplusplus
extern "C" {
#endif

/* For tests: the shape of the plan's last call that launched -- the lines it completed per row, the lines of a full batch,
 * the batches, and the words it carried in (the samples in front of the call that its first line reads).  Returns the kernel
 * launches made since creation (0: nothing was written); any pointer may be NULL. */
NVX_API int64_t nvx_spec_debug_last_launch(nvx_spectrum *s, int *lines, int *batch_lines, int *batches, int *carried);
/* For tests: `row` (-1: every row) stands at `position` as after a reset there: the samples in front of it count as silence,
 * and the survey starts there. */
NVX_API int nvx_spec_debug_set_position(nvx_spectrum *s, int row, uint64_t position);
/* For tests: the scratch rows of a launch stay below `bytes` (NVX_SPEC_SCRATCH_BYTES after create; a batch is one line at
 * least), so that a small call goes in several batches as a large one does. */
NVX_API int nvx_spec_debug_set_scratch(nvx_spectrum *s, size_t bytes);

#ifdef __cplusplus
}

/* how many lines are complete at position p */
static inline uint64_t nvx_spec_lines_at(uint64_t p, int n_log2, int avg)
{
    const uint64_t span = (uint64_t)NVX_SPEC_SPAN(n_log2, avg), hop = (uint64_t)NVX_SPEC_HOP(n_log2, avg);
    return p < span ? 0 : (p - span) / hop + 1;
}

struct nvx_spec_args {
    const void *in;           /* [n_rows][pitch_in] samples in the plan's format */
    size_t pitch_in;          /* samples */
    uint16_t *levels;         /* [n_rows][line_cap][N], or NULL */
    size_t line_cap;
    uint32_t *ring;           /* [n_rows][ring_words] */
    size_t ring_words;
    double *scratch;          /* [n_rows][batch_lines][3][N]: P_line, C_line.re, C_line.im in the order of an output line */
    double *survey;           /* [n_rows][3][N] */
    unsigned long long *count;           /* [n_rows] */
    const uint32_t *cfg;      /* [n_rows][NVX_SPEC_CFG_WORDS] */
    int n_in, n_rows, n_log2, avg;
    int span;                 /* (A + 1) H: the ring's length */
    int lines;                /* the call completes so many per row */
    int carried;              /* the samples in front of the call its lines read: sample g < 0 of the call is ring word
                               * ring0 + carried + g (less span where that passes it); line j begins at g = j A H - carried */
    uint32_t ring0;
    int line0, batch_lines;   /* this launch: lines [line0, line0 + batch_lines) of the call */
    int keep;                 /* the samples behind the last complete line once the call is in: below span */
    int keep_first;           /* the call's first sample that is kept: max(0, n_in - keep) */
    uint32_t keep_ring;       /* its ring word */
};

/* The arguments of one call of n_in samples over rows that stand at `consumed`; the pointers and the batch are the caller's. */
static inline void nvx_spec_fill_args(uint64_t consumed, size_t n_in, int n_log2, int avg, nvx_spec_args *out)
{
    nvx_spec_args a = {};
    const uint64_t hop = (uint64_t)NVX_SPEC_HOP(n_log2, avg), span = (uint64_t)NVX_SPEC_SPAN(n_log2, avg);
    const uint64_t before = nvx_spec_lines_at(consumed, n_log2, avg), after = nvx_spec_lines_at(consumed + n_in, n_log2, avg);
    a.n_in = (int)n_in; a.n_log2 = n_log2; a.avg = avg; a.span = (int)span;
    a.lines = (int)(after - before);
    a.carried = (int)(consumed - before * hop);
    a.ring0 = (uint32_t)((before * hop) % span);
    a.keep = (int)(consumed + n_in - after * hop);
    a.keep_first = (uint64_t)a.keep < n_in ? (int)(n_in - (uint64_t)a.keep) : 0;
    a.keep_ring = (uint32_t)((consumed + (uint64_t)a.keep_first) % span);
    *out = a;
}

#include <hip/hip_runtime.h>
/* on s: the line kernel over lines [line0, line0 + batch_lines) of every row and the fold of their scratch rows */
hipError_t nvx_spec_launch_lines(const nvx_spec_args *a, int format, hipStream_t s);
/* on s: the samples the call leaves behind its last complete line, into the ring */
hipError_t nvx_spec_launch_carry(const nvx_spec_args *a, int format, hipStream_t s);
#endif

#endif
