#!/usr/bin/env python3
"""Cost of carrier tuning (include/navtex_amd_tune.h) in the cascade kernel: HIP-event time of nvx_fir_cascade per launch,
no chain tuned against every chain tuned (random k), one chain and two chains, at the headline shape (4096 raw-rate
streams x 12 frames) and the 252 kS/s shape.  Prints one JSON line per configuration; profiles/TUNING.md records them.

    python tools/tune_rate.py [--reps 5] [--streams 4096] [--frames 12]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import numpy as np           # noqa: E402
import navtex_amd as nv      # noqa: E402
import signals               # noqa: E402


def run(raw, mask, tuned, n, frames, reps, buf, pitch):
    with nv.Pipeline(n_streams=n, raw_rate=raw, chain_mask=mask, max_frames=frames, char_layer=False) as p:
        if tuned:
            rng = np.random.default_rng(1)
            for s in range(n):
                for c in range(2):
                    if (mask >> c) & 1:
                        p.set_carrier(s, c, float(rng.integers(-8000, 8001)) * 3.125)
        p.enable_timing(True)
        p.process_resident(buf, pitch, 0, frames); p.fetch()          # warm-up
        p.kernel_time_stats(0, reset=True)
        for _ in range(reps):
            p.process_resident(buf, pitch, 0, frames)
        p.fetch()
        ms, launches = p.kernel_time_stats(0)
        return ms / max(1, launches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=12)
    a = ap.parse_args()
    for raw in (True, False):
        rate = nv.RATE_RAW if raw else nv.RATE_IN
        n = a.streams if raw else a.streams // 4                        # the 252 kS/s shape: a quarter of the streams
        frame = nv.FRAME_RAW if raw else nv.FRAME_IN
        pitch = a.frames * frame
        streams = [signals.stream_params(nv, s, rate)[0] for s in range(n)]
        buf = nv.DeviceBuffer(n * pitch * 4)
        nv.synth_device(streams, rate, pitch, buf, pitch)
        for mask in (nv.CHAIN_518, 3):
            # interleaved: nominal, tuned, nominal, tuned
            res = {"nominal": [], "tuned": []}
            for _ in range(2):
                for tuned in (False, True):
                    res["tuned" if tuned else "nominal"].append(run(raw, mask, tuned, n, a.frames, a.reps, buf, pitch))
            nom, tun = min(res["nominal"]), min(res["tuned"])
            print(json.dumps({"input": "raw" if raw else "252k", "streams": n, "frames": a.frames, "chains": 1 if mask == 1 else 2,
                              "cascade_ms_nominal": res["nominal"], "cascade_ms_tuned": res["tuned"],
                              "tuned_over_nominal": round(tun / nom, 4)}), flush=True)
        buf.free()


if __name__ == "__main__":
    main()
