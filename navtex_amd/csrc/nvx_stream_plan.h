/* nvx_stream_plan.h -- the launch arithmetic the companions that carry rows of streams share (the blanker, the IQ corrector,
 * the real-input converter, the noise canceller, the zoom bank, the row aligner, the multi-tap noise canceller, the diversity combiner; the polyphase plan and the narrowband interpolator for the first
 * two): how a
 * row's tiles are spread over workgroups, and when a launch may store 16 bytes at a time.  Pure C, no HIP: each library's
 * nvx_*_fill_args calls these with its own constants, and tests/harness/stream_plan_core.cpp walks them without a device.
 * Internal. */
#ifndef NVX_STREAM_PLAN_H
#define NVX_STREAM_PLAN_H

#include <stddef.h>
#include <stdint.h>

/* How many workgroups the host would spread a row over: a workgroup per row fills the chip from a few workgroups per CU on;
 * below that a row's tiles are spread out until the grid has about target_workgroups. */
static inline int nvx_stream_wanted(int n_rows, int target_workgroups)
{
    return n_rows >= 1024 ? 1 : (target_workgroups + n_rows - 1) / n_rows;
}

/* The chunks (workgroups) a row of `tiles` tiles gets where `wanted` are asked for, returned, and the tiles of every chunk
 * but the last: at least min_chunk_tiles where there is more than one chunk.  No tiles: one chunk. */
static inline int nvx_stream_chunks(int tiles, int wanted, int min_chunk_tiles, int *tiles_per_chunk)
{
    int per;
    if (wanted < 1) wanted = 1;
    per = tiles ? (tiles + wanted - 1) / wanted : 1;
    if (per < min_chunk_tiles) per = min_chunk_tiles;
    if (per > tiles && tiles) per = tiles;
    *tiles_per_chunk = per;
    return tiles ? (tiles + per - 1) / per : 1;
}

/* Every one of n_rows rows of 4-byte words, `pitch` words apart, is 16-byte aligned at its word `first`. */
static inline int nvx_stream_rows_aligned16(const void *base, size_t pitch, size_t first, int n_rows)
{
    return (((uintptr_t)base + (uintptr_t)first * 4) & 15) == 0 && (n_rows == 1 || (pitch & 3) == 0);
}

#endif
