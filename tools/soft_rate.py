#!/usr/bin/env python3
"""Cost of soft decoding (include/navtex_amd_soft.h): HIP-event time of nvx_demod_fsm per launch and the whole step, with
the mode off and with NVX_SOFT_DECODE, at the headline shape (4096 raw-rate streams x 12 frames, one chain).  Ten
launches after a warm-up, off and on interleaved twice.  In the steady state the demodulator of launch k runs beside the
cascade of launch k + 1, so the step shows what of the kernel's extra time is NOT hidden there plus the device-to-host
copy of 4 bytes per bit.  Prints one JSON line; profiles/TUNING.md records it.

    python tools/soft_rate.py [--reps 10] [--streams 4096] [--frames 12] [--charlayer]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import navtex_amd as nv      # noqa: E402
import signals               # noqa: E402


def run(mode, n, frames, reps, buf, pitch, charlayer):
    with nv.Pipeline(n_streams=n, raw_rate=True, chain_mask=nv.CHAIN_518, max_frames=frames, char_layer=charlayer) as p:
        if mode:
            p.enable_soft(mode)
        p.enable_timing(True)
        for _ in range(2):                                             # warm-up
            p.process_resident(buf, pitch, 0, frames)
        p.fetch()
        p.kernel_time_stats(0, reset=True)
        t0 = time.perf_counter()
        for _ in range(reps):
            p.process_resident(buf, pitch, 0, frames)
        p.fetch()                                                       # waits for the last launch's bits (and values)
        step = (time.perf_counter() - t0) / reps * 1e3
        fsm, launches = p.kernel_time_stats(3)
        front_fsm, _ = p.kernel_time_stats(1)
        casc, _ = p.kernel_time_stats(0)
        bits = sum(p.bit_count(s, 0) for s in range(n))
        values = sum(p.soft_count(s, 0) for s in range(n))
        return {"step_ms": step, "fsm_ms": fsm / launches, "demod_ms": front_fsm / launches, "cascade_ms": casc / launches,
                "bits_per_launch": bits // (reps + 2), "values_per_launch": values // (reps + 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--charlayer", action="store_true", help="with the host character layers (hard, and soft when on)")
    a = ap.parse_args()
    if nv.device_count() < 1:
        raise SystemExit("soft_rate.py needs a GPU")
    pitch = a.frames * nv.FRAME_RAW
    streams = [signals.stream_params(nv, s, nv.RATE_RAW)[0] for s in range(a.streams)]
    buf = nv.DeviceBuffer(a.streams * pitch * 4)
    nv.synth_device(streams, nv.RATE_RAW, pitch, buf, pitch)
    res = {"off": [], "on": []}
    for _ in range(2):
        for key, mode in (("off", 0), ("on", nv.SOFT_DECODE)):
            res[key].append(run(mode, a.streams, a.frames, a.reps, buf, pitch, a.charlayer))
    buf.free()
    best = {k: {f: min(r[f] for r in v) for f in v[0]} for k, v in res.items()}
    print(json.dumps({"streams": a.streams, "frames": a.frames, "reps": a.reps, "charlayer": a.charlayer, "runs": res,
                      "fsm_ms_off": round(best["off"]["fsm_ms"], 4), "fsm_ms_on": round(best["on"]["fsm_ms"], 4),
                      "step_ms_off": round(best["off"]["step_ms"], 3), "step_ms_on": round(best["on"]["step_ms"], 3),
                      "d2h_bytes_per_launch_on": 4 * best["on"]["values_per_launch"]}), flush=True)


if __name__ == "__main__":
    main()
