#!/usr/bin/env python3
"""Rate of the band scan (include/navtex_amd_scan.h): HIP-event kernel time of nvx_scan_resident per launch
(nvx_scan_time_stats), after a warm-up, over at least ten launches, at the headline batch (4096 raw-rate streams x 12
frames, generated on the device), two smaller raw-rate batches and the 252 kS/s batch.  Prints one JSON line per shape:
the algorithmic bytes (4 B x the samples a slot needs) and the fp64 operations of the header's arithmetic over the time,
against 8 TB/s and 39.3 T op/s (the no-FMA issue rate), and the bound that binds.  profiles/TUNING.md records them.

    python tools/scan_rate.py [--reps 10] [--frames 12] [--form 0]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import navtex_amd as nv          # noqa: E402
import navtex_amd.scan as sc     # noqa: E402
import signals                   # noqa: E402

HBM_BYTES_PER_S = 8.0e12
FP64_OPS_PER_S = 39.3e12
SLOT_SAMPLES_IN = 8256                       # 64 lead-in + 4 * 2048 samples at 252 kS/s
# per slot: FIR1 2048 outputs x 37 taps x 2 components x (product + sum); window 2 + 2 x 2048; transform 1024 butterflies x
# 11 stages x 10; power 3 x 2048 + the slot sum 2048
SLOT_OPS = 2048 * 37 * 2 * 2 + 2048 * 4 + 1024 * 11 * 10 + 2048 * 4


def run(raw, n, frames, reps, form):
    rate = nv.RATE_RAW if raw else nv.RATE_IN
    pitch = frames * (nv.FRAME_RAW if raw else nv.FRAME_IN)
    streams = [signals.stream_params(nv, s, rate, freq_hz=(s * 37) % 48001 - 24000)[0] for s in range(n)]
    buf = nv.DeviceBuffer(n * pitch * 4)
    nv.synth_device(streams, rate, pitch, buf, pitch)
    out = nv.DeviceBuffer(n * sc.FFT * 8)
    sc.set_form(form)
    sc.timing(True)
    sc.scan_resident_into(buf, pitch, 0, frames, n, raw, 1, out)          # warm-up
    sc.time_stats(reset=True)
    for _ in range(reps):
        sc.scan_resident_into(buf, pitch, 0, frames, n, raw, 1, out)
    ms, launches = sc.time_stats(reset=True)
    sc.timing(False)
    buf.free(); out.free()
    assert launches == reps
    t = ms / launches * 1e-3
    slots = n * frames * sc.SLOTS_PER_FRAME
    nbytes = slots * SLOT_SAMPLES_IN * (8 if raw else 1) * 4
    ops = slots * SLOT_OPS
    t_hbm, t_ops = nbytes / HBM_BYTES_PER_S, ops / FP64_OPS_PER_S
    return {"input": "raw" if raw else "252k", "streams": n, "frames": frames, "form": form, "launches": launches,
            "ms_per_launch": round(t * 1e3, 4), "algorithmic_GB": round(nbytes / 1e9, 3), "TB_per_s": round(nbytes / t / 1e12, 3),
            "fp64_Top_per_s": round(ops / t / 1e12, 3), "of_hbm_bound": round(t_hbm / t, 3), "of_fp64_bound": round(t_ops / t, 3),
            "binding_bound": "HBM read" if t_hbm >= t_ops else "fp64 issue"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--form", type=int, default=0)
    a = ap.parse_args()
    for raw, n in ((True, 4096), (True, 512), (True, 64), (False, 4096)):
        print(json.dumps(run(raw, n, a.frames, max(10, a.reps), a.form)), flush=True)


if __name__ == "__main__":
    main()
