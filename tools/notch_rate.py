#!/usr/bin/env python3
"""Rate of the tone notch (include/navtex_amd_notch.h) against the IQ corrector: HIP-event time per call (the three kernels,
and the zeroing of the block records where a call starts inside a block: nvx_notch_time_stats / nvx_iqc_time_stats), after a
warm-up, over ten calls of each, interleaved in one process (notch, corrector, notch, ...), median, minimum and maximum.  The
rows go on from call to call as a stream does: 252 000 samples are 984 blocks and 96 samples, so every call but each eighth
starts inside a block.  Shape: 4096 rows x 252 000 samples (1 s at 252 kS/s) as int16 and as unsigned 8-bit, with K = 1 and
K = 4 notches enabled per row; the corrector runs on the same rows into an output of its own.  Both read their input twice and
write 4 bytes per sample (CS16: 12 bytes per sample); the notch adds 2 K table reads per sample from the LDS.  Prints one JSON
line per format and K.  DESIGN 3.15 records them.

With --first-hz the first notch sits at the given frequencies, one run each: a lane reads the table at its own phase, so the
LDS bank conflicts depend on the step (0 Hz: every lane the same word; 492.1875 Hz: a lane's four samples 32 words from the
next lane's, every lane on one bank).

    python tools/notch_rate.py [--reps 10] [--rows 4096] [--samples 252000] [--formats cs16,cu8] [--notches 1,4] [--width-log2 5]
                               [--first-hz 0,492.1875,-13939]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import navtex_amd as nv               # noqa: E402
import navtex_amd.iqc as iq           # noqa: E402
import navtex_amd.notch as nt         # noqa: E402

STREAMING_TB_S = 6.29
FORMATS = {"cs16": nt.CS16, "cu8": nt.CU8, "cs8": nt.CS8, "cf32": nt.CF32}
CARRIERS_HZ = (-13940.0, -14310.0, 3000.0, 21000.0)
RATE = 252000.0


def _timed(h, call):
    call()
    ms, calls = h.time_stats(reset=True)
    assert calls == 1
    return ms


def run(fmt_name, rows, n, k, width_log2, reps, first_hz=None):
    fmt = FORMATS[fmt_name]
    bps = nt.BYTES_PER_SAMPLE[fmt]
    # four carriers over noise, the same in every row: the time does not depend on the data, but the table reads depend on the steps
    rng = np.random.default_rng(1)
    z = rng.uniform(-1500, 1500, n) + 1j * rng.uniform(-1500, 1500, n)
    for hz in CARRIERS_HZ:
        z = z + 3000 * np.exp(2j * np.pi * ((np.arange(n) * (hz / RATE)) % 1.0))
    x = np.stack([z.real, z.imag], axis=1)
    row = {nt.CS16: lambda: np.rint(x).astype(np.int16), nt.CU8: lambda: np.clip(np.rint(x * 3 / 256 + 127.5), 0, 255).astype(np.uint8),
           nt.CS8: lambda: np.clip(np.rint(x * 3 / 256), -128, 127).astype(np.int8), nt.CF32: lambda: (x / 32768.0).astype(np.float32)}[fmt]()
    d_rows = nv.DeviceBuffer(rows * n * bps)
    d_out = nv.DeviceBuffer(rows * n * 4); d_out2 = nv.DeviceBuffer(rows * n * 4)
    for s in range(rows):
        d_rows.upload(row, s * n * bps)
    with nt.Notch(fmt, n_rows=rows, n_notches=k, width_log2=width_log2) as c, iq.Corrector(fmt, n_streams=rows) as q:
        for j in range(k):
            c.set_freq(j, nt.step_from_hz(CARRIERS_HZ[j] + 1.0 if j or first_hz is None else first_hz, RATE)); c.enable(j)
        c.timing(True); q.timing(True)
        notch = lambda: c.resident(d_rows, n, n, d_out, n)          # noqa: E731
        correct = lambda: q.resident(d_rows, n, n, d_out2, n)       # noqa: E731
        _timed(c, notch); _timed(q, correct)                        # warm-up
        t_c, t_q = [], []
        for _ in range(reps):
            t_c.append(_timed(c, notch))
            t_q.append(_timed(q, correct))
        shape, shape_q = c.debug_last_launch(), q.debug_last_launch()
        status = c.get(0)
    for d in (d_rows, d_out, d_out2):
        d.free()
    mc, mq = statistics.median(t_c), statistics.median(t_q)
    nbytes = rows * n * (2 * bps + 4)
    return {"format": fmt_name, "notch0_hz": CARRIERS_HZ[0] + 1.0 if first_hz is None else first_hz, "rows": rows, "samples_per_row": n, "notches": k, "width_log2": width_log2, "runs_each": reps,
            "notch_ms_median": round(mc, 4), "notch_ms_min": round(min(t_c), 4), "notch_ms_max": round(max(t_c), 4),
            "iqc_ms_median": round(mq, 4), "iqc_ms_min": round(min(t_q), 4), "iqc_ms_max": round(max(t_q), 4),
            "GB_two_reads_one_write": round(nbytes / 1e9, 3),
            "notch_TB_per_s": round(nbytes / (mc * 1e-3) / 1e12, 3), "iqc_TB_per_s": round(nbytes / (mq * 1e-3) / 1e12, 3),
            "notch_over_iqc_time": round(mc / mq, 3), "notch_of_streaming": round(nbytes / (mc * 1e-3) / 1e12 / STREAMING_TB_S, 3),
            "streaming_TB_per_s": STREAMING_TB_S, "notch_chunks": shape["chunks"], "notch_tiles_per_chunk": shape["tiles_per_chunk"],
            "notch_records": shape["records"], "iqc_chunks": shape_q["chunks"], "pairs_notch0": status["pairs"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=252000)
    ap.add_argument("--formats", default="cs16,cu8")
    ap.add_argument("--notches", default="1,4")
    ap.add_argument("--width-log2", type=int, default=nt.WIDTH_LOG2_DEFAULT)
    ap.add_argument("--first-hz", default="", help="comma-separated frequencies of notch 0, one run each: the table reads' bank conflicts depend on the step")
    a = ap.parse_args()
    n = a.samples // 8 * 8                                   # every row starts 16-byte aligned in every format
    if nv.device_count() < 1:
        raise SystemExit("tools/notch_rate.py needs a GPU: there is no CPU path and nothing to time without one")
    for name in a.formats.split(","):
        for k in a.notches.split(","):
            for hz in ([float(v) for v in a.first_hz.split(",")] if a.first_hz else [None]):
                print(json.dumps(run(name, a.rows, n, int(k), a.width_log2, max(1, a.reps), hz)), flush=True)


if __name__ == "__main__":
    main()
