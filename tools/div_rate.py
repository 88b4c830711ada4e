#!/usr/bin/env python3
"""Rate of the diversity combiner (include/navtex_amd_div.h) against the antenna noise canceller: HIP-event time per call (all
three kernels and, where a call starts inside a block, the zeroing of the block records: nvx_div_time_stats /
nvx_anc_time_stats), after a warm-up, over ten calls of each, interleaved in one process (combiner, canceller, combiner, ...),
median, minimum and maximum.  The rows go on from call to call as a stream does, so the windows are full and every cell start
is solved.  Shape: 2048 pairs x 252 000 samples (1 s at 252 kS/s) as int16 and as unsigned 8-bit, with 1 target and with 4; the
canceller runs on the same rows, which lie in one buffer (the main rows, then the second rows), into an output of its own.
By bytes one target reads what the canceller reads (both rows twice) and writes the same (4 bytes per pair-sample; CS16: 20
in all); each further target adds 4 bytes written.  Prints one JSON line per format and number of targets.  DESIGN 3.20
records them.

    python tools/div_rate.py [--reps 10] [--pairs 2048] [--samples 252000] [--formats cs16,cu8] [--targets 1,4]"""
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
import navtex_amd.div as dv           # noqa: E402

STREAMING_TB_S = 6.29
FORMATS = {"cs16": dv.CS16, "cu8": dv.CU8, "cs8": dv.CS8, "cf32": dv.CF32}
RATE = 252000.0
TARGETS_HZ = (-14000.0, 14000.0, -3500.0, 21000.0)


class _At:
    def __init__(self, ptr):
        self.ptr = ptr


def _combine(c, d_rows, d_out, pairs, n, bps):
    c.resident(d_rows, n, _At(d_rows.ptr + pairs * n * bps), n, n, d_out, n)
    ms, calls = c.time_stats(reset=True)
    assert calls == 1
    return ms


def run(fmt_name, pairs, n, reps, targets):
    fmt = FORMATS[fmt_name]
    bps = dv.BYTES_PER_SAMPLE[fmt]
    # a carrier at each target on both rows (gains 1 and 0.5 e^{j 1.0}) over own noise, the same in every pair: the time does not depend on the data
    rng = np.random.default_rng(1)
    t = np.arange(n)
    s = sum(1500 * np.exp(2j * np.pi * hz / RATE * t) for hz in TARGETS_HZ)
    rows = [s + rng.uniform(-1500, 1500, n) + 1j * rng.uniform(-1500, 1500, n), 0.5 * np.exp(1.0j) * s + rng.uniform(-1500, 1500, n) + 1j * rng.uniform(-1500, 1500, n)]

    def to_format(z):
        x = np.stack([z.real, z.imag], axis=1)
        return {dv.CS16: lambda: np.rint(x).astype(np.int16), dv.CU8: lambda: np.clip(np.rint(x * 3 / 256 + 127.5), 0, 255).astype(np.uint8),
                dv.CS8: lambda: np.clip(np.rint(x * 3 / 256), -128, 127).astype(np.int8), dv.CF32: lambda: (x / 32768.0).astype(np.float32)}[fmt]()

    d_rows = nv.DeviceBuffer(2 * pairs * n * bps)               # [2 pairs rows][n]: the main rows, then the second rows
    d_out = nv.DeviceBuffer(pairs * targets * n * 4); d_out2 = nv.DeviceBuffer(pairs * n * 4)
    for k, z in enumerate(rows):
        row = to_format(z)
        for p in range(pairs):
            d_rows.upload(row, (k * pairs + p) * n * bps)
    with dv.Combiner(fmt, n_pairs=pairs, n_targets=targets) as c, an.Canceller(fmt, n_pairs=pairs) as q:
        for k in range(targets):
            c.set_freq(k, dv.step_from_hz(TARGETS_HZ[k], RATE))
        c.timing(True); q.timing(True)
        for _ in range(2):                                      # warm-up; the second call starts inside a block, as all behind it do
            _combine(c, d_rows, d_out, pairs, n, bps); _combine(q, d_rows, d_out2, pairs, n, bps)
        t_c, t_q = [], []
        for _ in range(reps):
            t_c.append(_combine(c, d_rows, d_out, pairs, n, bps))
            t_q.append(_combine(q, d_rows, d_out2, pairs, n, bps))
        shape, shape_q = c.debug_last_launch(), q.debug_last_launch()
        status = c.get(0, 0)
    for d in (d_rows, d_out, d_out2):
        d.free()
    mc, mq = statistics.median(t_c), statistics.median(t_q)
    div_bytes = pairs * n * (4 * bps + 4 * targets)
    anc_bytes = pairs * n * (4 * bps + 4)
    div_tb, anc_tb = div_bytes / (mc * 1e-3) / 1e12, anc_bytes / (mq * 1e-3) / 1e12
    return {"format": fmt_name, "pairs": pairs, "targets": targets, "samples_per_row": n, "runs_each": reps,
            "div_ms_median": round(mc, 4), "div_ms_min": round(min(t_c), 4), "div_ms_max": round(max(t_c), 4),
            "anc_ms_median": round(mq, 4), "anc_ms_min": round(min(t_q), 4), "anc_ms_max": round(max(t_q), 4),
            "div_GB_two_reads_of_both_rows_one_write_per_target": round(div_bytes / 1e9, 3), "anc_GB_two_reads_of_both_rows_one_write": round(anc_bytes / 1e9, 3),
            "div_TB_per_s": round(div_tb, 3), "anc_TB_per_s": round(anc_tb, 3),
            "div_over_anc_time": round(mc / mq, 3), "by_bytes": round((4 * bps + 4 * targets) / (4 * bps + 4), 3),
            "div_of_streaming": round(div_tb / STREAMING_TB_S, 3), "streaming_TB_per_s": STREAMING_TB_S,
            "div_chunks": shape["chunks"], "div_tiles_per_chunk": shape["tiles_per_chunk"], "anc_chunks": shape_q["chunks"],
            "lead_pair0": status["lead"], "weight_pair0": status["weight"], "coherence_pair0": status["coherence_q14"], "cells_solved_pair0": status["cells_solved"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=252000)
    ap.add_argument("--formats", default="cs16,cu8")
    ap.add_argument("--targets", default="1,4")
    a = ap.parse_args()
    n = a.samples // 8 * 8                                   # every row starts 16-byte aligned in every format
    if nv.device_count() < 1:
        raise SystemExit("tools/div_rate.py needs a GPU: there is no CPU path and nothing to time without one")
    for name in a.formats.split(","):
        for targets in a.targets.split(","):
            print(json.dumps(run(name, a.pairs, n, max(1, a.reps), int(targets))), flush=True)


if __name__ == "__main__":
    main()
