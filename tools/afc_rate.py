#!/usr/bin/env python3
"""What automatic frequency control (include/navtex_amd_afc.h) costs a step at the headline shape: 4096 raw-rate streams x 12
frames, one chain each, the launches bench.py times (resident input generated on the device, K launches queued, one fetch).
One handle, one process, three settings taken in turn -- tracking off, tracking on for every chain, tracking on for one
chain -- `rounds` times each, interleaved (off, all, one, off, ...), after a warm-up; a setting's figure is the median over
its rounds of (wall time of K steps) / K.  Tracking on is reported as its delta against tracking off in the same process,
with the run-to-run spread of the off figure (max - min over its rounds) beside it, and the update kernel's own HIP-event
time per launch (nvx_kernel_time_stats, which = 4) from a timed pass of its own behind the untimed ones.  Prints one JSON
line.  DESIGN 3.1.2 records it.

    python tools/afc_rate.py [--streams 4096] [--frames 12] [--steps 10] [--warmup 3] [--rounds 5]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import navtex_amd as nv               # noqa: E402
import signals                        # noqa: E402

SETTINGS = ("off", "all", "one")


def setting(pipe, name, streams, was):
    """Tracking as `name` says, from what `was` left."""
    if was == "all":
        for s in range(streams):
            pipe.afc_disable(s, 0)
    elif was == "one":
        pipe.afc_disable(0, 0)
    if name == "all":
        for s in range(streams):
            pipe.afc_enable(s, 0)
    elif name == "one":
        pipe.afc_enable(0, 0)


def steps_ms(pipe, buf, pitch, frames, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        pipe.process_resident(buf, pitch, 0, frames)
    pipe.fetch()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    S, F = a.streams, a.frames
    pitch = F * nv.FRAME_RAW
    buf = nv.DeviceBuffer(S * pitch * 4)
    nv.synth_device([signals.stream_params(nv, s, nv.RATE_RAW)[0] for s in range(S)], nv.RATE_RAW, pitch, buf, pitch)
    ms = {name: [] for name in SETTINGS}
    kernel_ms = {}
    with nv.Pipeline(n_streams=S, raw_rate=True, chain_mask=nv.CHAIN_518, max_frames=F, bit_history=65536) as pipe:
        was = "off"
        for _ in range(a.warmup):
            pipe.process_resident(buf, pitch, 0, F)
        pipe.fetch()
        for _ in range(max(1, a.rounds)):
            for name in SETTINGS:
                setting(pipe, name, S, was); was = name
                pipe.process_resident(buf, pitch, 0, F); pipe.fetch()          # the setting's first launch is not timed
                ms[name].append(steps_ms(pipe, buf, pitch, F, a.steps))
        pipe.enable_timing(True)
        for name in ("all", "one"):                                            # the update kernel's own time, events on
            setting(pipe, name, S, was); was = name
            pipe.fetch(); pipe.kernel_time_stats(0, reset=True)
            for _ in range(a.steps):
                pipe.process_resident(buf, pitch, 0, F)
            pipe.fetch()
            total, launches = pipe.kernel_time_stats(4)
            kernel_ms[name] = total / max(1, launches)
            if name == "all":                                                   # of 64 chains across the handle: their gates passed
                moved = sum(pipe.afc_status(s, 0)["updates"] > 0 for s in range(0, S, max(1, S // 64)))
    buf.free()
    med = {name: statistics.median(v) for name, v in ms.items()}
    out = {"streams": S, "frames": F, "steps": a.steps, "rounds": len(ms["off"]),
           "off_ms": round(med["off"], 4), "off_spread_ms": round(max(ms["off"]) - min(ms["off"]), 4),
           "all_ms": round(med["all"], 4), "all_minus_off_ms": round(med["all"] - med["off"], 4),
           "one_ms": round(med["one"], 4), "one_minus_off_ms": round(med["one"] - med["off"], 4),
           "update_kernel_ms_all": round(kernel_ms["all"], 5), "update_kernel_ms_one": round(kernel_ms["one"], 5),
           "note_bytes_per_launch": 8 * 2 * S, "sampled_chains_whose_gate_passed_of_64": moved,
           "off_ms_rounds": [round(v, 4) for v in ms["off"]], "all_ms_rounds": [round(v, 4) for v in ms["all"]],
           "one_ms_rounds": [round(v, 4) for v in ms["one"]]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
