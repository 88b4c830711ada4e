#!/usr/bin/env python3
"""Rate of the channel tap (include/navtex_amd_tap.h): HIP-event time per call (nvx_tap_time_stats), after a warm-up, over ten
calls, median and minimum.  Shapes: 4096 inputs x 2 taps x 1 s of 252 kS/s IQ to 12 kS/s IQ, 48 kS/s IQ and 8 kS/s audio, and
64 inputs x 2 taps to 12 kS/s IQ.  Per output the kernel issues R int16 dot products per component and half (R = T + 3 rounded
up to 8; two components, two halves of the split taps): 2 R v_dot2.  The paper bound printed beside the time is the larger of
that count at full issue rate (256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz, one v_dot2 per lane and clock) and the bytes -- every
input sample read once per tile row (the taps of an input share it through the caches), every output written once -- at the
streaming figure.  Every shape runs in a process of its own under a time limit, and the first that fails ends the run.
Prints one JSON line per shape.  DESIGN 3.13 records them.

    python tools/tap_rate.py [--reps 10] [--seconds 1.0] [--limit 180]"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
STREAMING_TB_S = 6.29
DOT2_PER_S = 256 * 4 * 16 * 2.4e9
# name: (inputs, taps, rate, kind)
SHAPES = {"12k_iq": (4096, 2, 12000, "iq"), "48k_iq": (4096, 2, 48000, "iq"), "8k_real": (4096, 2, 8000, "real"), "12k_iq_64": (64, 2, 12000, "iq")}


def run(name, reps, seconds):
    import numpy as np
    sys.path.insert(0, str(ROOT))
    import navtex_amd as nv
    import navtex_amd.tap as tp
    inputs, taps, rate, kind_name = SHAPES[name]
    kind = {"iq": tp.IQ, "real": tp.REAL}[kind_name]
    n_in = int(tp.INPUT_RATE * seconds)
    rng = np.random.default_rng(1)
    k = np.arange(n_in)
    z = 9000 * np.exp(2j * np.pi * 0.055 * k) + 4000 * np.exp(-2j * np.pi * 0.0556 * k)      # the time does not depend on the data
    row = np.rint(np.stack([z.real, z.imag], axis=1) + rng.uniform(-3000, 3000, size=(n_in, 2))).astype(np.int16)
    d_in = nv.DeviceBuffer(inputs * n_in * 4)
    for s in range(inputs):
        d_in.upload(row, s * n_in * 4)
    with tp.Tap(rate, kind, n_inputs=inputs, n_taps=taps) as c:
        n_out = tp.out_count(c.L, c.M, 0, n_in)
        d_out = nv.DeviceBuffer(inputs * taps * n_out * tp.OUT_BYTES[kind])
        for t, hz in enumerate((14000.0, -14000.0)[:taps]):
            c.set_shift(t, hz)
        c.timing(True)

        def call():
            c.reset()
            assert c.resident(d_in, n_in, n_in, d_out, n_out) == n_out
            ms, calls = c.time_stats(reset=True)
            assert calls == 1
            return ms

        call()                                              # warm-up
        times = [call() for _ in range(reps)]
        shape = c.debug_last_launch()
        out = {"shape": name, "inputs": inputs, "taps": taps, "rate": rate, "kind": kind_name, "L": c.L, "M": c.M, "T": c.T,
               "samples_per_input": n_in, "outputs_per_row": n_out, "runs": reps}
    med = statistics.median(times)
    R = (out["T"] + 3 + 7) // 8 * 8
    outputs = inputs * taps * n_out
    dot2 = outputs * 2 * R
    nbytes = inputs * n_in * 4 + outputs * tp.OUT_BYTES[kind]
    bound_ms = max(dot2 / DOT2_PER_S, nbytes / (STREAMING_TB_S * 1e12)) * 1e3
    out.update({"ms_median": round(med, 4), "ms_min": round(min(times), 4), "G_outputs_per_s": round(outputs / (med * 1e-3) / 1e9, 3),
                "G_dot2": round(dot2 / 1e9, 2), "GB_read_once_plus_write": round(nbytes / 1e9, 3), "paper_bound_ms": round(bound_ms, 4),
                "time_over_paper_bound": round(med / bound_ms, 2), "tile_out": shape["tile_out"], "tiles": shape["tiles"], "form": shape["form"],
                "lds_bytes": shape["lds_bytes"]})
    d_in.free(); d_out.free()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--limit", type=int, default=180, help="seconds a shape may take")
    ap.add_argument("--shape", default=None, help="run this shape in this process")
    a = ap.parse_args()
    if a.shape:
        return run(a.shape, max(1, a.reps), a.seconds)
    for name in SHAPES:                                     # a process and a time limit each; nothing more runs after a failure
        done = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), "--shape", name,
                               "--reps", str(a.reps), "--seconds", str(a.seconds)])
        if done.returncode != 0:
            print(json.dumps({"shape": name, "failed": done.returncode}), flush=True)
            return done.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
