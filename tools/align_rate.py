#!/usr/bin/env python3
"""Rate of the row aligner (include/navtex_amd_align.h).

Apply: HIP-event time per call (nvx_align_time_stats / nvx_iqc_time_stats), after a warm-up, over ten calls of the aligner and
of the IQ corrector, interleaved in one process (aligner, corrector, aligner, ...), median, minimum and maximum.  Shape: 2048
pairs x 252 000 samples (1 s at 252 kS/s) as int16 and as unsigned 8-bit, delay 137 + 13/32 samples; the corrector runs on the
same 4096 rows, which lie in one buffer (the main rows, then the sense rows).  The aligner's bytes are counted as one read of
both rows and one write of both (CS16: 16 per pair-sample), the corrector's as two reads and one write per sample (CS16: 12).

Measure: ten calls at one stated shape, 8 pairs x 8192 lags x N = 65 536 (int16), against the issue-rate bound of its
2 n_lags N dot products per pair: one v_dot2_i32_i16 per lane and clock, 64 lanes per CU, 256 CUs at a nominal 2.4 GHz.  The
clock under this load was not measured, so the share of the bound is a lower estimate.

Prints one JSON line per format and one for the measurement, each with the date.  DESIGN 3.17 records them.  Not measured
here: other delays (the time does not depend on the delay but for the alignment of the main row's loads), max_delay above the
default (every call rewrites the carried samples), float32 and int8 input unless asked for, and the measurement at other shapes.

    python tools/align_rate.py [--reps 10] [--pairs 2048] [--samples 252000] [--formats cs16,cu8]"""
import argparse
import datetime
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import navtex_amd as nv               # noqa: E402
import navtex_amd.align as al         # noqa: E402
import navtex_amd.iqc as iq           # noqa: E402

STREAMING_TB_S = 6.29
DOT_LANES_PER_S = 256 * 64 * 2.4e9
FORMATS = {"cs16": al.CS16, "cu8": al.CU8, "cs8": al.CS8, "cf32": al.CF32}
DELAY_Q5 = 137 * 32 + 13


class _At:
    def __init__(self, ptr):
        self.ptr = ptr


def _rows(n, fmt, rng):
    x = rng.uniform(-6000, 6000, (n, 2))
    return {al.CS16: lambda: np.rint(x).astype(np.int16), al.CU8: lambda: np.clip(np.rint(x * 3 / 256 + 127.5), 0, 255).astype(np.uint8),
            al.CS8: lambda: np.clip(np.rint(x * 3 / 256), -128, 127).astype(np.int8), al.CF32: lambda: (x / 32768.0).astype(np.float32)}[fmt]()


def _once(handle, call):
    call()
    ms, calls = handle.time_stats(reset=True)
    assert calls == 1
    return ms


def run_apply(fmt_name, pairs, n, reps):
    fmt = FORMATS[fmt_name]
    bps = al.BYTES_PER_SAMPLE[fmt]
    rng = np.random.default_rng(1)
    d_rows = nv.DeviceBuffer(2 * pairs * n * bps)               # [2 pairs rows][n]: the main rows, then the sense rows
    d_out = nv.DeviceBuffer(2 * pairs * n * 4); d_out2 = nv.DeviceBuffer(2 * pairs * n * 4)
    for k in range(2):
        row = _rows(n, fmt, rng)                                # the same in every pair: the time does not depend on the data
        for s in range(pairs):
            d_rows.upload(row, (k * pairs + s) * n * bps)
    sense, out_sense = _At(d_rows.ptr + pairs * n * bps), _At(d_out.ptr + pairs * n * 4)
    with al.Aligner(fmt, n_pairs=pairs) as c, iq.Corrector(fmt, n_streams=2 * pairs) as q:
        c.timing(True); q.timing(True)
        c.set_delay(DELAY_Q5)
        align = lambda: c.resident(d_rows, n, sense, n, n, d_out, n, out_sense, n)      # noqa: E731
        correct = lambda: q.resident(d_rows, n, n, d_out2, n)                          # noqa: E731
        _once(c, align); _once(q, correct)                       # warm-up
        t_a, t_q = [], []
        for _ in range(reps):
            t_a.append(_once(c, align))
            t_q.append(_once(q, correct))
        shape = c.debug_last_launch()
    for d in (d_rows, d_out, d_out2):
        d.free()
    ma, mq = statistics.median(t_a), statistics.median(t_q)
    a_bytes, q_bytes = pairs * n * (2 * bps + 8), 2 * pairs * n * (2 * bps + 4)
    a_tb, q_tb = a_bytes / (ma * 1e-3) / 1e12, q_bytes / (mq * 1e-3) / 1e12
    return {"what": "apply", "date": datetime.date.today().isoformat(), "format": fmt_name, "pairs": pairs, "samples_per_row": n, "runs_each": reps,
            "delay_q5": DELAY_Q5, "align_ms_median": round(ma, 4), "align_ms_min": round(min(t_a), 4), "align_ms_max": round(max(t_a), 4),
            "iqc_ms_median": round(mq, 4), "iqc_ms_min": round(min(t_q), 4), "iqc_ms_max": round(max(t_q), 4), "iqc_rows": 2 * pairs,
            "align_GB_one_read_one_write_of_both_rows": round(a_bytes / 1e9, 3), "iqc_GB_two_reads_one_write": round(q_bytes / 1e9, 3),
            "align_TB_per_s": round(a_tb, 3), "iqc_TB_per_s": round(q_tb, 3), "align_over_iqc_time": round(ma / mq, 3),
            "by_bytes": round((2 * bps + 8) / (2 * (2 * bps + 4)), 3), "align_of_streaming": round(a_tb / STREAMING_TB_S, 3),
            "streaming_TB_per_s": STREAMING_TB_S, "align_chunks": shape["chunks"], "align_tiles_per_chunk": shape["tiles_per_chunk"]}


def run_measure(reps, pairs=8, n_lags=8192, window=65536):
    n_in = window + n_lags - 1
    n_row = (n_in + 7) // 8 * 8
    rng = np.random.default_rng(2)
    d_rows = nv.DeviceBuffer(2 * pairs * n_row * 4)
    for k in range(2):
        row = _rows(n_row, al.CS16, rng)
        for s in range(pairs):
            d_rows.upload(row, (k * pairs + s) * n_row * 4)
    sense = _At(d_rows.ptr + pairs * n_row * 4)
    with al.Aligner(al.CS16, n_pairs=pairs) as c:
        assert al.window(n_in, -n_lags // 2, n_lags) == window
        c.timing(True)
        call = lambda: c.measure_resident(d_rows, n_row, sense, n_row, n_in, -n_lags // 2, n_lags)      # noqa: E731
        _once(c, call)
        t = [_once(c, call) for _ in range(reps)]
    d_rows.free()
    m = statistics.median(t)
    dots = 2 * n_lags * window * pairs
    bound_ms = dots / DOT_LANES_PER_S * 1e3
    return {"what": "measure", "date": datetime.date.today().isoformat(), "format": "cs16", "pairs": pairs, "n_lags": n_lags, "window": window,
            "runs": reps, "ms_median": round(m, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "dot_products": dots,
            "issue_rate_bound_ms_at_2.4_GHz": round(bound_ms, 4), "share_of_the_bound": round(bound_ms / m, 3), "T_dot_products_per_s": round(dots / (m * 1e-3) / 1e12, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=252000)
    ap.add_argument("--formats", default="cs16,cu8")
    a = ap.parse_args()
    n = a.samples // 8 * 8                                   # every row starts 16-byte aligned in every format
    if nv.device_count() < 1:
        raise SystemExit("tools/align_rate.py needs a GPU: there is no CPU path and nothing to time without one")
    for name in a.formats.split(","):
        print(json.dumps(run_apply(name, a.pairs, n, max(1, a.reps))), flush=True)
    print(json.dumps(run_measure(max(1, a.reps))), flush=True)


if __name__ == "__main__":
    main()
