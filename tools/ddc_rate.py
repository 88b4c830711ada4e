#!/usr/bin/env python3
"""Rate of the down-converter bank (include/navtex_amd_ddc.h) against the resampler it is built on: HIP-event kernel time
per launch (nvx_ddc_time_stats / nvx_resample_time_stats), after a warm-up, over ten launches of each, interleaved in one
process (bank, resampler, bank, ...), median and minimum.  Shapes: 256 inputs x 16 slices x 1 966 080 samples at 2.4 MS/s as
unsigned 8-bit and as int16, and 4096 inputs x 1 slice of the same length; the yardstick is nvx_resample_resident with as
many streams as the bank has output rows (4096), same rate, format and length, reading the same device buffer.  Prints one
JSON line per shape: both times and their ratio, the bytes read plus written per second against the algorithmic bytes (the
input once plus the output rows), and the instructions of the staging step per group of 8 samples counted in the generated
code (the constants below, re-counted from the ISA when the kernel changes).  DESIGN 3.8 and profiles/TUNING.md record them.

    python tools/ddc_rate.py [--reps 10] [--rows 4096] [--samples 1966080] [--formats cu8,cs16]"""
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
import navtex_amd.resample as rs      # noqa: E402

RATE = 2400000
STREAMING_TB_S = 6.29
# instructions of nvx_ddc_bank<format, true> per staged group of 8 samples, counted in the ISA as (VALU, LDS + vector memory):
# the k = 0 branch (the resampler's staging) and the mixing branch (8 table reads, 16 dot products, shifts, clamps, packing)
STAGE_K0 = {dd.CS16: (13.5, 4), dd.CU8: (17.5, 3)}
STAGE_MIX = {dd.CS16: (189.5, 12), dd.CU8: (205.5, 11)}
FORMATS = {"cu8": dd.CU8, "cs16": dd.CS16}


def _one(obj, d_in, pitch, n_in, d_out, n_out):
    obj.reset()
    obj.resident(d_in, pitch, n_in, d_out, n_out)
    ms, launches = obj.time_stats(reset=True)
    assert launches == 1
    return ms


def run(fmt_name, rows, n_in, reps):
    fmt = FORMATS[fmt_name]
    bps = dd.BYTES_PER_SAMPLE[fmt]
    n_out = rs.out_count(RATE, 0, n_in)
    d_in = nv.DeviceBuffer(rows * n_in * bps)
    d_out = nv.DeviceBuffer(rows * n_out * 4)
    row = np.random.default_rng(1).integers(0, 256, size=n_in * bps, dtype=np.uint8)
    for s in range(rows):                            # the same noise in every row: the time does not depend on the data
        d_in.upload(row, s * n_in * bps)
    kmax = (dd.GRID * (RATE - 2 * dd.GUARD_HZ)) // (2 * RATE)
    out = []
    with rs.Resampler(RATE, fmt, n_streams=rows) as r:
        r.timing(True)
        for n_inputs, n_slices in ((rows // 16, 16), (rows, 1)):
            with dd.Ddc(RATE, fmt, n_inputs=n_inputs, n_slices=n_slices) as d:
                # slices spread over the band, none at k = 0: every row pays the mixer
                for s in range(n_slices):
                    d.set_shift(s, ((2 * s + 1) * kmax // (2 * n_slices) * (1 if s % 2 else -1)) * RATE / dd.GRID)
                d.timing(True)
                _one(d, d_in, n_in, n_in, d_out, n_out); _one(r, d_in, n_in, n_in, d_out, n_out)      # warm-up
                t_d, t_r = [], []
                for _ in range(reps):
                    t_d.append(_one(d, d_in, n_in, n_in, d_out, n_out))
                    t_r.append(_one(r, d_in, n_in, n_in, d_out, n_out))
                shape = d.debug_last_launch()
            md, mr = statistics.median(t_d), statistics.median(t_r)
            algo = n_inputs * n_in * bps + rows * n_out * 4              # the input once, every output row
            touched = rows * (n_in * bps + n_out * 4)                    # what the workgroups load and store
            out.append({"rate": RATE, "format": fmt_name, "inputs": n_inputs, "slices": n_slices, "samples_per_input": n_in,
                        "launches_each": reps, "ddc_ms_median": round(md, 4), "ddc_ms_min": round(min(t_d), 4),
                        "resample_ms_median": round(mr, 4), "resample_ms_min": round(min(t_r), 4), "ddc_over_resample": round(md / mr, 3),
                        "algorithmic_GB": round(algo / 1e9, 3), "algorithmic_TB_per_s": round(algo / (md * 1e-3) / 1e12, 3),
                        "loaded_plus_stored_TB_per_s": round(touched / (md * 1e-3) / 1e12, 3),
                        "resample_TB_per_s": round(touched / (mr * 1e-3) / 1e12, 3), "streaming_TB_per_s": STREAMING_TB_S,
                        "chunks": shape["chunks"], "tiles_per_chunk": shape["tiles_per_chunk"], "lds_bytes": shape["lds_bytes"],
                        "stage_k0_per_group": STAGE_K0[fmt], "stage_mix_per_group": STAGE_MIX[fmt]})
    d_in.free(); d_out.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=1966080)
    ap.add_argument("--formats", default="cu8,cs16")
    a = ap.parse_args()
    for name in a.formats.split(","):
        for line in run(name, a.rows, a.samples // 8 * 8, max(1, a.reps)):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
