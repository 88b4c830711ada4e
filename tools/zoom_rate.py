#!/usr/bin/env python3
"""Rate of the zoom bank (include/navtex_amd_zoom.h) against the down-converter bank: HIP-event time per call
(nvx_zoom_time_stats / nvx_ddc_time_stats), after a warm-up, over ten calls of each, interleaved in one process (zoom, bank,
zoom, ...), median, minimum and maximum.  The inputs go on from call to call as a stream does.  Shape: 256 inputs x 2 016 000
samples at k = 5 (8.064 MS/s x 0.25 s -> 252 kS/s) as int16 and as unsigned 8-bit, with one zoom and with four; the bank runs
on as many input bytes: the same rows taken as 2.4 MS/s, with as many slices as the zoom has zooms.  Prints one JSON line per
format and number of zooms: ms, input GB/s, the share of the 8 TB/s peak.  DESIGN 3.16 records them.

    python tools/zoom_rate.py [--reps 10] [--inputs 256] [--samples 2016000] [--log2-decim 5] [--formats cs16,cu8] [--zooms 1,4]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import navtex_amd as nv               # noqa: E402
import navtex_amd.ddc as dd           # noqa: E402
import navtex_amd.zoom as zm          # noqa: E402

PEAK_TB_S = 8.0
BANK_RATE = 2400000
FORMATS = {"cs16": zm.CS16, "cu8": zm.CU8, "cs8": zm.CS8, "cf32": zm.CF32}
STEPS = (-1219, 1422, 37, -500, 2047, -2048, 512, 1)
BANK_HZ = (-300000.0, 350000.0, 21000.0, -700000.0, 1000000.0, -1000000.0, 500000.0, 600.0)


def _timed(h, call):
    call()
    ms, calls = h.time_stats(reset=True)
    assert calls == 1
    return ms


def run(fmt_name, inputs, n, k, zooms, reps):
    fmt = FORMATS[fmt_name]
    bps = zm.BYTES_PER_SAMPLE[fmt]
    # a few tones over noise, the same in every input: the time does not depend on the data
    rng = np.random.default_rng(1)
    t = np.arange(n)
    z = rng.uniform(-1500, 1500, n) + 1j * rng.uniform(-1500, 1500, n) + 6000 * np.exp(2j * np.pi * ((t * 0.2977) % 1.0)) + 3000 * np.exp(-2j * np.pi * ((t * 0.0713) % 1.0))
    x = np.stack([z.real, z.imag], axis=1)
    row = {zm.CS16: lambda: np.rint(x).astype(np.int16), zm.CU8: lambda: np.clip(np.rint(x * 3 / 256 + 127.5), 0, 255).astype(np.uint8),
           zm.CS8: lambda: np.clip(np.rint(x * 3 / 256), -128, 127).astype(np.int8), zm.CF32: lambda: (x / 32768.0).astype(np.float32)}[fmt]()
    d_rows = nv.DeviceBuffer(inputs * n * bps)
    for s in range(inputs):
        d_rows.upload(row, s * n * bps)
    outs = n >> k
    with zm.Zoom(k, fmt, n_inputs=inputs, n_zooms=zooms) as c, dd.Ddc(BANK_RATE, fmt, n_inputs=inputs, n_slices=zooms) as q:
        bank_outs = -((-n * q.L) // q.M) + 1
        d_out = nv.DeviceBuffer(inputs * zooms * outs * 4); d_out2 = nv.DeviceBuffer(inputs * zooms * bank_outs * 4)
        for j in range(zooms):
            c.set_step(j, STEPS[j]); q.set_shift(j, BANK_HZ[j])
        c.timing(True); q.timing(True)
        zoom = lambda: c.resident(d_rows, n, n, d_out, outs)                # noqa: E731
        bank = lambda: q.resident(d_rows, n, n, d_out2, bank_outs)          # noqa: E731
        _timed(c, zoom); _timed(q, bank)                                    # warm-up
        t_c, t_q = [], []
        for _ in range(reps):
            t_c.append(_timed(c, zoom))
            t_q.append(_timed(q, bank))
        shape = c.debug_last_launch()
        for d in (d_out, d_out2):
            d.free()
    d_rows.free()
    mc, mq = statistics.median(t_c), statistics.median(t_q)
    in_bytes = inputs * n * bps
    return {"format": fmt_name, "inputs": inputs, "samples_per_input": n, "log2_decim": k, "zooms": zooms, "runs_each": reps,
            "zoom_ms_median": round(mc, 4), "zoom_ms_min": round(min(t_c), 4), "zoom_ms_max": round(max(t_c), 4),
            "bank_ms_median": round(mq, 4), "bank_ms_min": round(min(t_q), 4), "bank_ms_max": round(max(t_q), 4),
            "input_GB": round(in_bytes / 1e9, 3), "zoom_input_GB_per_s": round(in_bytes / (mc * 1e-3) / 1e9, 1),
            "bank_input_GB_per_s": round(in_bytes / (mq * 1e-3) / 1e9, 1),
            "zoom_share_of_peak": round(in_bytes / (mc * 1e-3) / 1e12 / PEAK_TB_S, 4), "bank_share_of_peak": round(in_bytes / (mq * 1e-3) / 1e12 / PEAK_TB_S, 4),
            "zoom_Gsamples_per_s_and_zoom": round(inputs * n / (mc * 1e-3) / 1e9, 2), "peak_TB_per_s": PEAK_TB_S, "bank_rate": BANK_RATE,
            "zoom_chunks": shape["chunks"], "zoom_tiles_per_chunk": shape["tiles_per_chunk"], "zoom_warm_tiles": shape["warm_tiles"],
            "zoom_lds_bytes": shape["lds_bytes"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inputs", type=int, default=256)
    ap.add_argument("--samples", type=int, default=2016000)
    ap.add_argument("--log2-decim", type=int, default=5)
    ap.add_argument("--formats", default="cs16,cu8")
    ap.add_argument("--zooms", default="1,4")
    a = ap.parse_args()
    n = a.samples // 64 * 64                                 # a multiple of every D, and every row starts 16-byte aligned in every format
    if nv.device_count() < 1:
        raise SystemExit("tools/zoom_rate.py needs a GPU: there is no CPU path and nothing to time without one")
    for name in a.formats.split(","):
        for z in a.zooms.split(","):
            print(json.dumps(run(name, a.inputs, n, a.log2_decim, int(z), max(1, a.reps))), flush=True)


if __name__ == "__main__":
    main()
