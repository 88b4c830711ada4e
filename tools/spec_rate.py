#!/usr/bin/env python3
"""Rate of the spectrum monitor (include/navtex_amd_spec.h) against the band scan: HIP-event time per call (the line kernel
and the fold per batch of lines, and the carry: nvx_spec_time_stats / nvx_scan_time_stats), after a warm-up, over ten calls of
each, interleaved in one process (monitor with level words, monitor survey only, scan, monitor, ...), median, minimum and
maximum.  The rows go on from call to call as a stream does.  Shape: 4096 rows x 252 000 int16 samples at N = 2048 and at
N = 4096, A = 8; the scan runs on the same rows as 252 kS/s streams (three whole frames of 80 640 samples: 27 transforms of
2048 points per row, on FIR1's output, a quarter of the samples).  The monitor's transforms overlap by half, so it transforms
every sample twice: the comparison is per transformed sample (transforms x N).  Prints one JSON line per N.  DESIGN 3.21
records them.

    python tools/spec_rate.py [--reps 10] [--rows 4096] [--samples 252000] [--sizes 11,12] [--avg 8] [--format cs16]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import navtex_amd as nv               # noqa: E402
import navtex_amd.scan as scan        # noqa: E402
import navtex_amd.spec as sp          # noqa: E402

STREAMING_TB_S = 6.29
FORMATS = {"cs16": sp.CS16, "cu8": sp.CU8, "cs8": sp.CS8, "cf32": sp.CF32}
CARRIERS_HZ = (-13940.0, -14310.0, 3000.0, 21000.0)
RATE = 252000.0


def _timed_spec(h, call):
    call()
    ms, calls = h.time_stats(reset=True)
    assert calls == 1
    return ms


def _timed_scan(call):
    call()
    ms, calls = scan.time_stats(reset=True)
    assert calls == 1
    return ms


def _stats(t):
    return {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}


def run(fmt_name, rows, n, n_log2, avg, reps):
    fmt = FORMATS[fmt_name]
    bps = sp.BYTES_PER_SAMPLE[fmt]
    N = 1 << n_log2
    # four carriers over noise, the same in every row: the time does not depend on the data
    rng = np.random.default_rng(1)
    z = rng.uniform(-1500, 1500, n) + 1j * rng.uniform(-1500, 1500, n)
    for hz in CARRIERS_HZ:
        z = z + 3000 * np.exp(2j * np.pi * ((np.arange(n) * (hz / RATE)) % 1.0))
    x = np.stack([z.real, z.imag], axis=1)
    row = {sp.CS16: lambda: np.rint(x).astype(np.int16), sp.CU8: lambda: np.clip(np.rint(x * 3 / 256 + 127.5), 0, 255).astype(np.uint8),
           sp.CS8: lambda: np.clip(np.rint(x * 3 / 256), -128, 127).astype(np.int8), sp.CF32: lambda: (x / 32768.0).astype(np.float32)}[fmt]()
    d_rows = nv.DeviceBuffer(rows * n * bps)
    for s in range(rows):
        d_rows.upload(row, s * n * bps)
    frames = n // nv.FRAME_IN
    with_scan = fmt == sp.CS16 and frames >= 1
    d_power = nv.DeviceBuffer(rows * scan.FFT * 8)
    with sp.Spectrum(fmt, n_rows=rows, n_log2=n_log2, avg=avg) as a, sp.Spectrum(fmt, n_rows=rows, n_log2=n_log2, avg=avg) as b:
        cap = a.lines_for(n) + 1                                 # a later call of a stream may complete one line more than the first
        d_levels = nv.DeviceBuffer(rows * cap * N * 2)
        a.timing(True); b.timing(True); scan.timing(True)
        levels = lambda: a.resident(d_rows, n, n, d_levels, cap)          # noqa: E731
        survey = lambda: b.resident(d_rows, n, n)                         # noqa: E731
        scanned = lambda: scan.scan_resident_into(d_rows, n, 0, frames, rows, False, 0, d_power)     # noqa: E731
        _timed_spec(a, levels); _timed_spec(b, survey)                    # warm-up
        if with_scan:
            _timed_scan(scanned)
        t_l, t_s, t_q, lines = [], [], [], []
        for _ in range(reps):
            lines.append(a.lines_for(n))
            t_l.append(_timed_spec(a, levels))
            t_s.append(_timed_spec(b, survey))
            if with_scan:
                t_q.append(_timed_scan(scanned))
        shape = a.debug_last_launch()
        total = a.get(0)[3]
        d_levels.free()
    d_rows.free(); d_power.free()
    ml, ms = statistics.median(t_l), statistics.median(t_s)
    per_call = statistics.mean(lines)
    transformed = rows * per_call * avg * N                      # samples that go through a transform per call
    nbytes = rows * (n * bps + per_call * N * 2)                 # the input once (its second reading is the L2's) and the level words
    out = {"format": fmt_name, "rows": rows, "samples_per_row": n, "n_log2": n_log2, "avg": avg, "runs_each": reps, "lines_per_call": per_call,
           "lines_in_survey": total, "batch_lines": shape["batch_lines"], "batches": shape["batches"],
           "levels_ms": _stats(t_l), "survey_only_ms": _stats(t_s),
           "transformed_Gsamples_per_call": round(transformed / 1e9, 3), "levels_Gsamples_transformed_per_s": round(transformed / (ml * 1e-3) / 1e9, 2),
           "survey_Gsamples_transformed_per_s": round(transformed / (ms * 1e-3) / 1e9, 2),
           "fp64_flops_per_transformed_sample": 5 * n_log2 + 14, "levels_fp64_TFLOP_per_s": round(transformed * (5 * n_log2 + 14) / (ml * 1e-3) / 1e12, 2),
           "GB_read_once_and_levels": round(nbytes / 1e9, 3), "levels_TB_per_s": round(nbytes / (ml * 1e-3) / 1e12, 3),
           "levels_of_streaming": round(nbytes / (ml * 1e-3) / 1e12 / STREAMING_TB_S, 3), "streaming_TB_per_s": STREAMING_TB_S}
    if with_scan:
        mq = statistics.median(t_q)
        scan_transformed = rows * frames * 9 * scan.FFT
        out.update({"scan_ms": _stats(t_q), "scan_frames": frames, "scan_Gsamples_transformed_per_s": round(scan_transformed / (mq * 1e-3) / 1e9, 2),
                    "levels_over_scan_time_per_transformed_sample": round((ml / transformed) / (mq / scan_transformed), 3),
                    "survey_over_scan_time_per_transformed_sample": round((ms / transformed) / (mq / scan_transformed), 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=252000)
    ap.add_argument("--sizes", default="11,12")
    ap.add_argument("--avg", type=int, default=sp.AVG_DEFAULT)
    ap.add_argument("--format", default="cs16")
    a = ap.parse_args()
    n = a.samples // 8 * 8                                   # every row starts 16-byte aligned in every format
    if nv.device_count() < 1:
        raise SystemExit("tools/spec_rate.py needs a GPU: there is no CPU path and nothing to time without one")
    for size in a.sizes.split(","):
        print(json.dumps(run(a.format, a.rows, n, int(size), a.avg, max(1, a.reps))), flush=True)


if __name__ == "__main__":
    main()
