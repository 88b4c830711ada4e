#!/usr/bin/env python3
"""Rate of the multi-tap noise canceller (include/navtex_amd_wanc.h) against the single-weight canceller on the same rows:
HIP-event time per call (all kernels and the zeroing of the block records: nvx_wanc_time_stats / nvx_anc_time_stats), after a
warm-up, over ten calls of each, interleaved in one process (K = 4, K = 8, K = 16, single weight, K = 4, ...), median, minimum
and maximum.  The rows go on from call to call as a stream does, so after the warm-up calls the windows are full and every
block start is solved.  Shape: 2048 pairs x 252 000 samples (1 s at 252 kS/s) as int16 and as unsigned 8-bit.  Both libraries'
bytes are two reads of both rows and one write per pair-sample (CS16: 20, CU8: 12).  Prints one JSON line per format.  DESIGN
3.18 records them.

    python tools/wanc_rate.py [--reps 10] [--pairs 2048] [--samples 252000] [--formats cs16,cu8] [--taps 4,8,16]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import navtex_amd as nv               # noqa: E402
import navtex_amd.anc as an           # noqa: E402
import navtex_amd.wanc as wn          # noqa: E402

STREAMING_TB_S = 6.29
FORMATS = {"cs16": wn.CS16, "cu8": wn.CU8, "cs8": wn.CS8, "cf32": wn.CF32}


class _At:
    def __init__(self, ptr):
        self.ptr = ptr


def _cancel(c, d_rows, d_out, pairs, n, bps):
    c.resident(d_rows, n, _At(d_rows.ptr + pairs * n * bps), n, n, d_out, n)
    ms, calls = c.time_stats(reset=True)
    assert calls == 1
    return ms


def run(fmt_name, pairs, n, reps, taps):
    fmt = FORMATS[fmt_name]
    bps = wn.BYTES_PER_SAMPLE[fmt]
    # common noise over an echo on the main row and at 0.8 e^{j 2.1} on the sense row, over a little own noise, the same in every
    # pair: the time does not depend on the data
    rng = np.random.default_rng(1)
    loc = rng.uniform(-6000, 6000, n) + 1j * rng.uniform(-6000, 6000, n)
    echo = loc.copy()
    echo[1:] += 0.5j * loc[:-1]
    rows = [echo + rng.uniform(-150, 150, n) + 1j * rng.uniform(-150, 150, n), 0.8 * np.exp(2.1j) * loc + rng.uniform(-150, 150, n) + 1j * rng.uniform(-150, 150, n)]

    def to_format(z):
        x = np.stack([z.real, z.imag], axis=1)
        return {wn.CS16: lambda: np.rint(x).astype(np.int16), wn.CU8: lambda: np.clip(np.rint(x * 3 / 256 + 127.5), 0, 255).astype(np.uint8),
                wn.CS8: lambda: np.clip(np.rint(x * 3 / 256), -128, 127).astype(np.int8), wn.CF32: lambda: (x / 32768.0).astype(np.float32)}[fmt]()

    d_rows = nv.DeviceBuffer(2 * pairs * n * bps)               # [2 pairs rows][n]: the main rows, then the sense rows
    d_out = nv.DeviceBuffer(pairs * n * 4)
    for k, z in enumerate(rows):
        row = to_format(z)
        for s in range(pairs):
            d_rows.upload(row, (k * pairs + s) * n * bps)
    names = [f"wanc_k{k}" for k in taps] + ["anc"]
    plans = [wn.Canceller(fmt, n_pairs=pairs, n_taps=k) for k in taps] + [an.Canceller(fmt, n_pairs=pairs)]
    times = {name: [] for name in names}
    try:
        for c in plans:
            c.timing(True)
        for _ in range(2):                                       # warm-up: five blocks, the windows are full behind them
            for c in plans:
                _cancel(c, d_rows, d_out, pairs, n, bps)
        for _ in range(reps):
            for name, c in zip(names, plans):
                times[name].append(_cancel(c, d_rows, d_out, pairs, n, bps))
        shape = plans[0].debug_last_launch()
        solved = {name: c.get(0)["blocks_solved"] for name, c in zip(names, plans)}
    finally:
        for c in plans:
            c.close()
        d_rows.free(); d_out.free()
    total = pairs * n * (4 * bps + 4)
    out = {"format": fmt_name, "pairs": pairs, "samples_per_row": n, "runs_each": reps, "GB_two_reads_of_both_rows_one_write": round(total / 1e9, 3),
           "streaming_TB_per_s": STREAMING_TB_S, "chunks": shape["chunks"], "tiles_per_chunk": shape["tiles_per_chunk"], "records": shape["records"]}
    med_anc = statistics.median(times["anc"])
    for name in names:
        t = times[name]
        med = statistics.median(t)
        out[name] = {"ms_median": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "TB_per_s": round(total / (med * 1e-3) / 1e12, 3),
                     "of_streaming": round(total / (med * 1e-3) / 1e12 / STREAMING_TB_S, 3), "over_anc": round(med / med_anc, 2),
                     "blocks_solved_pair0": solved[name]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=252000)
    ap.add_argument("--formats", default="cs16,cu8")
    ap.add_argument("--taps", default="4,8,16")
    a = ap.parse_args()
    n = a.samples // 8 * 8                                   # every row starts 16-byte aligned in every format
    if nv.device_count() < 1:
        raise SystemExit("tools/wanc_rate.py needs a GPU: there is no CPU path and nothing to time without one")
    for name in a.formats.split(","):
        print(json.dumps(run(name, a.pairs, n, max(1, a.reps), [int(k) for k in a.taps.split(",")])), flush=True)


if __name__ == "__main__":
    main()
