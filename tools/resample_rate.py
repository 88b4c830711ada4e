#!/usr/bin/env python3
"""Rate of the resampler (include/navtex_amd_resample.h): HIP-event kernel time of nvx_resample_resident per launch
(nvx_resample_time_stats), after a warm-up, over at least ten launches, at the headline batch (4096 streams x 0.96 s at
2.048 MS/s, int16 and unsigned 8-bit), the same duration at 250 kS/s int16 and at 3.2 MS/s float32, and 64 streams at
2.048 MS/s.  Prints one JSON line per shape: the bytes read plus written over the time, against the 6.29 TB/s streaming
figure of the chip and the 5.1 TB/s (read plus write) of nvx_channelise, and the vector instructions per input sample
counted in the generated code (per 8 tap slots of the FIR loop, per output, per staged group of 8 samples: the constants
below, re-counted from the ISA when the kernel changes).  profiles/TUNING.md records them.

    python tools/resample_rate.py [--reps 10] [--form 0] [--streams 4096] [--seconds 0.96]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import navtex_amd as nv               # noqa: E402
import navtex_amd.resample as rs      # noqa: E402

STREAMING_TB_S = 6.29
CHANNELISE_TB_S = 5.1
# instructions of nvx_resample<format, true>, counted in the ISA as (VALU, LDS + vector memory):
LOOP_PER_8_SLOTS = (10, 6)            # 8 v_dot2c_i32_i16 + 2 address adds; 6 ds_read_b64
PER_OUTPUT = (31, 1)                  # window and tap-row addresses, rounding shift, clamp, pack, the (q, r) step; the store
PER_GROUP = {rs.CS16: (13.5, 4), rs.CU8: (17.5, 3), rs.CS8: (17.5, 3), rs.CF32: (116.5, 6)}    # per 8 staged samples: conversion
#                                       and loop share; the 16-byte loads and two ds_write_b128


def instructions_per_input_sample(fmt, L, M, T):
    """(VALU, all vector instructions) per input sample."""
    tp = (T + 6) // 4 * 4
    out = []
    for k in (0, 1):
        per_output = PER_OUTPUT[k] + LOOP_PER_8_SLOTS[k] * tp / 8.0
        out.append(per_output * L / M + PER_GROUP[fmt][k] / 8.0)
    return out[0], out[0] + out[1]


def run(fi, fmt, n_streams, seconds, reps, form):
    n_in = int(round(fi * seconds)) // 8 * 8
    bps = rs.BYTES_PER_SAMPLE[fmt]
    n_out = rs.out_count(fi, 0, n_in)
    d_in = nv.DeviceBuffer(n_streams * n_in * bps)
    d_out = nv.DeviceBuffer(n_streams * n_out * 4)
    rng = np.random.default_rng(1)
    row = (rng.uniform(-1, 1, size=(n_in, 2)).astype(np.float32) if fmt == rs.CF32 else
           rng.integers(0, 256, size=n_in * bps, dtype=np.uint8))
    for s in range(n_streams):                       # the same noise in every stream: the time does not depend on the data
        d_in.upload(row, s * n_in * bps)
    with rs.Resampler(fi, fmt, n_streams=n_streams) as r:
        r.set_form(form)
        r.timing(True)
        r.resident(d_in, n_in, n_in, d_out, n_out)   # warm-up
        r.time_stats(reset=True)
        for _ in range(reps):
            r.reset()
            r.resident(d_in, n_in, n_in, d_out, n_out)
        ms, launches = r.time_stats(reset=True)
        L, M, T = r.L, r.M, r.T
    d_in.free(); d_out.free()
    assert launches == reps
    t = ms / launches * 1e-3
    nbytes = n_streams * (n_in * bps + n_out * 4)
    return {"rate": fi, "format": ("cs16", "cu8", "cs8", "cf32")[fmt], "streams": n_streams, "samples_per_stream": n_in, "form": form,
            "launches": launches, "ms_per_launch": round(t * 1e3, 4), "read_plus_written_GB": round(nbytes / 1e9, 3),
            "TB_per_s": round(nbytes / t / 1e12, 3), "of_streaming_6.29": round(nbytes / t / 1e12 / STREAMING_TB_S, 3),
            "of_channelise_5.1": round(nbytes / t / 1e12 / CHANNELISE_TB_S, 3),
            "input_GS_per_s": round(n_streams * n_in / t / 1e9, 2), "L": L, "M": M, "T": T,
            "valu_per_input_sample": round(instructions_per_input_sample(fmt, L, M, T)[0], 2),
            "vector_instructions_per_input_sample": round(instructions_per_input_sample(fmt, L, M, T)[1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--form", type=int, default=0)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=0.96)
    a = ap.parse_args()
    shapes = ((2048000, rs.CS16, a.streams), (2048000, rs.CU8, a.streams), (250000, rs.CS16, a.streams), (3200000, rs.CF32, a.streams),
              (2048000, rs.CS16, 64))
    for fi, fmt, n in shapes:
        print(json.dumps(run(fi, fmt, n, a.seconds, max(10, a.reps), a.form)), flush=True)


if __name__ == "__main__":
    main()
