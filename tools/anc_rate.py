#!/usr/bin/env python3
"""Rate of the antenna noise canceller (include/navtex_amd_anc.h) against the IQ corrector: HIP-event time per call (both
kernels and the zeroing of the block records: nvx_anc_time_stats / nvx_iqc_time_stats), after a warm-up, over ten calls of
each, interleaved in one process (canceller, corrector, canceller, ...), median, minimum and maximum.  The rows go on from call
to call as a stream does, so the windows are full and every block start is solved.  Shape: 2048 pairs x
252 000 samples (1 s at 252 kS/s) as int16 and as unsigned 8-bit; the corrector runs on the same 4096 rows, which lie in one
buffer (the main rows, then the sense rows), into an output of its own.  The canceller's bytes are counted as two reads of both
rows and one write per pair-sample (CS16: 20), the corrector's as two reads and one write per sample (CS16: 12): by bytes the
canceller costs 20/12 of the corrector per output row in CS16 and 12/8 in CU8.  Prints one JSON line per format.  DESIGN 3.14
records them.

    python tools/anc_rate.py [--reps 10] [--pairs 2048] [--samples 252000] [--formats cs16,cu8]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import navtex_amd as nv               # noqa: E402
import navtex_amd.anc as an           # noqa: E402
import navtex_amd.iqc as iq           # noqa: E402

STREAMING_TB_S = 6.29
FORMATS = {"cs16": an.CS16, "cu8": an.CU8, "cs8": an.CS8, "cf32": an.CF32}


class _At:
    def __init__(self, ptr):
        self.ptr = ptr


def _cancel(c, d_rows, d_out, pairs, n, bps):
    c.resident(d_rows, n, _At(d_rows.ptr + pairs * n * bps), n, n, d_out, n)
    ms, calls = c.time_stats(reset=True)
    assert calls == 1
    return ms


def _correct(q, d_rows, d_out2, n):
    q.resident(d_rows, n, n, d_out2, n)
    ms, calls = q.time_stats(reset=True)
    assert calls == 1
    return ms


def run(fmt_name, pairs, n, reps):
    fmt = FORMATS[fmt_name]
    bps = an.BYTES_PER_SAMPLE[fmt]
    # common noise at 0.8 e^{j 2.1} on the sense row over a little own noise, the same in every pair: the time does not depend on the data
    rng = np.random.default_rng(1)
    loc = rng.uniform(-6000, 6000, n) + 1j * rng.uniform(-6000, 6000, n)
    rows = [loc + rng.uniform(-150, 150, n) + 1j * rng.uniform(-150, 150, n), 0.8 * np.exp(2.1j) * loc + rng.uniform(-150, 150, n) + 1j * rng.uniform(-150, 150, n)]

    def to_format(z):
        x = np.stack([z.real, z.imag], axis=1)
        return {an.CS16: lambda: np.rint(x).astype(np.int16), an.CU8: lambda: np.clip(np.rint(x * 3 / 256 + 127.5), 0, 255).astype(np.uint8),
                an.CS8: lambda: np.clip(np.rint(x * 3 / 256), -128, 127).astype(np.int8), an.CF32: lambda: (x / 32768.0).astype(np.float32)}[fmt]()

    d_rows = nv.DeviceBuffer(2 * pairs * n * bps)               # [2 pairs rows][n]: the main rows, then the sense rows
    d_out = nv.DeviceBuffer(pairs * n * 4); d_out2 = nv.DeviceBuffer(2 * pairs * n * 4)
    for k, z in enumerate(rows):
        row = to_format(z)
        for s in range(pairs):
            d_rows.upload(row, (k * pairs + s) * n * bps)
    with an.Canceller(fmt, n_pairs=pairs) as c, iq.Corrector(fmt, n_streams=2 * pairs) as q:
        c.timing(True); q.timing(True)
        _cancel(c, d_rows, d_out, pairs, n, bps); _correct(q, d_rows, d_out2, n)                    # warm-up
        t_c, t_q = [], []
        for _ in range(reps):
            t_c.append(_cancel(c, d_rows, d_out, pairs, n, bps))
            t_q.append(_correct(q, d_rows, d_out2, n))
        shape, shape_q = c.debug_last_launch(), q.debug_last_launch()
        status = c.get(0)
    for d in (d_rows, d_out, d_out2):
        d.free()
    mc, mq = statistics.median(t_c), statistics.median(t_q)
    anc_bytes = pairs * n * (4 * bps + 4)
    iqc_bytes = 2 * pairs * n * (2 * bps + 4)
    anc_tb, iqc_tb = anc_bytes / (mc * 1e-3) / 1e12, iqc_bytes / (mq * 1e-3) / 1e12
    # per output row: the canceller writes `pairs` rows, the corrector twice as many
    per_row = (mc / pairs) / (mq / (2 * pairs))
    return {"format": fmt_name, "pairs": pairs, "samples_per_row": n, "runs_each": reps,
            "anc_ms_median": round(mc, 4), "anc_ms_min": round(min(t_c), 4), "anc_ms_max": round(max(t_c), 4),
            "iqc_ms_median": round(mq, 4), "iqc_ms_min": round(min(t_q), 4), "iqc_ms_max": round(max(t_q), 4), "iqc_rows": 2 * pairs,
            "anc_GB_two_reads_of_both_rows_one_write": round(anc_bytes / 1e9, 3), "iqc_GB_two_reads_one_write": round(iqc_bytes / 1e9, 3),
            "anc_TB_per_s": round(anc_tb, 3), "iqc_TB_per_s": round(iqc_tb, 3),
            "anc_over_iqc_time_per_output_row": round(per_row, 3), "by_bytes": round((4 * bps + 4) / (2 * bps + 4), 3),
            "anc_of_streaming": round(anc_tb / STREAMING_TB_S, 3), "streaming_TB_per_s": STREAMING_TB_S,
            "anc_chunks": shape["chunks"], "anc_tiles_per_chunk": shape["tiles_per_chunk"], "iqc_chunks": shape_q["chunks"],
            "weight_pair0": status["weight"], "coherence_pair0": status["coherence_q14"], "blocks_solved_pair0": status["blocks_solved"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=252000)
    ap.add_argument("--formats", default="cs16,cu8")
    a = ap.parse_args()
    n = a.samples // 8 * 8                                   # every row starts 16-byte aligned in every format
    if nv.device_count() < 1:
        raise SystemExit("tools/anc_rate.py needs a GPU: there is no CPU path and nothing to time without one")
    for name in a.formats.split(","):
        print(json.dumps(run(name, a.pairs, n, max(1, a.reps))), flush=True)


if __name__ == "__main__":
    main()
