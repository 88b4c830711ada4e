#!/usr/bin/env python3
"""Rate of the impulse noise blanker (include/navtex_amd_blank.h) against the channeliser: HIP-event kernel time per launch
(nvx_blank_time_stats / nvx_channelise_time_stats), after a warm-up, over ten launches of each, interleaved in one process
(blanker, channeliser, blanker, ...), median and minimum.  Shapes: 4096 streams x 1 966 080 samples as int16 and as unsigned
8-bit (one workgroup per stream), and 64 streams of the same length (a stream spread over workgroups, each behind a pre-roll).
The yardstick is nvx_channelise_resident on the same device buffers in the same run: like the blanker as int16 it reads
every byte once and writes as many (DESIGN 3 quotes it at 5.1 TB/s read plus write); the chip's streaming figure is the other
reference.  Prints one JSON line per shape: both times, the bytes read plus written per second of both and their ratio.
DESIGN 3.9 and profiles/TUNING.md record them.

    python tools/blank_rate.py [--reps 10] [--streams 4096,64] [--samples 1966080] [--formats cs16,cu8]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import navtex_amd as nv               # noqa: E402
import navtex_amd.blank as bl         # noqa: E402

STREAMING_TB_S = 6.29
FORMATS = {"cs16": bl.CS16, "cu8": bl.CU8, "cs8": bl.CS8, "cf32": bl.CF32}


def _blank(b, d_in, d_out, n):
    b.reset()
    b.resident(d_in, n, n, d_out, n)
    ms, launches = b.time_stats(reset=True)
    assert launches == 1
    return ms


def _channelise(d_in, d_out, streams, n):
    nv.channelise(d_in, n, 0, streams, n // 8, d_out, n // 8)
    ms, launches = nv.channelise_time_stats(reset=True)
    assert launches == 1
    return ms


def run(fmt_name, streams, n, reps, d_in, d_out):
    fmt = FORMATS[fmt_name]
    bps = bl.BYTES_PER_SAMPLE[fmt]
    # uniform noise with a burst every 25 000 samples, the same in every row: the time does not depend on the data
    rng = np.random.default_rng(1)
    x = rng.integers(-1500, 1501, size=(n, 2))
    for s in range(5000, n - 300, 25000):
        x[s:s + 200] = rng.integers(-30000, 30001, size=(200, 2))
    row = {bl.CS16: lambda: x.astype(np.int16), bl.CU8: lambda: np.clip(x // 256 + 128, 0, 255).astype(np.uint8),
           bl.CS8: lambda: np.clip(x // 256, -128, 127).astype(np.int8), bl.CF32: lambda: (x / 32768.0).astype(np.float32)}[fmt]()
    for s in range(streams):
        d_in.upload(row, s * n * bps)
    with bl.Blanker(fmt, n_streams=streams) as b:
        b.timing(True)
        _blank(b, d_in, d_out, n); _channelise(d_in, d_out, streams, n)            # warm-up
        t_b, t_c = [], []
        for _ in range(reps):
            t_b.append(_blank(b, d_in, d_out, n))
            t_c.append(_channelise(d_in, d_out, streams, n))
        shape = b.debug_last_launch()
        _, detections, blanked = b.stats(0)
    mb, mc = statistics.median(t_b), statistics.median(t_c)
    blank_bytes = streams * n * (bps + 4)
    chan_bytes = streams * n * 8                             # the channeliser reads the buffer as int16 whatever it holds
    blank_tb, chan_tb = blank_bytes / (mb * 1e-3) / 1e12, chan_bytes / (mc * 1e-3) / 1e12
    return {"format": fmt_name, "streams": streams, "samples_per_stream": n, "launches_each": reps,
            "blank_ms_median": round(mb, 4), "blank_ms_min": round(min(t_b), 4), "channelise_ms_median": round(mc, 4),
            "channelise_ms_min": round(min(t_c), 4), "blank_GB": round(blank_bytes / 1e9, 3), "blank_TB_per_s": round(blank_tb, 3),
            "channelise_TB_per_s": round(chan_tb, 3), "blank_over_channelise_bytes_per_s": round(blank_tb / chan_tb, 3),
            "of_streaming": round(blank_tb / STREAMING_TB_S, 3), "streaming_TB_per_s": STREAMING_TB_S,
            "chunks": shape["chunks"], "blocks_per_chunk": shape["blocks_per_chunk"], "preroll_blocks": shape["preroll_blocks"],
            "blanked_fraction_stream0": round(blanked / ((reps + 1) * n), 5), "detections_stream0_per_launch": detections // (reps + 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--streams", default="4096,64")
    ap.add_argument("--samples", type=int, default=1966080)
    ap.add_argument("--formats", default="cs16,cu8")
    a = ap.parse_args()
    n = a.samples // 512 * 512                               # the channeliser takes multiples of 64 outputs
    counts = [int(s) for s in a.streams.split(",")]
    nv.lib.nvx_channelise_timing(1)
    widest = max(4, *(bl.BYTES_PER_SAMPLE[FORMATS[name]] for name in a.formats.split(",")))        # the channeliser reads 4 bytes a sample
    d_in = nv.DeviceBuffer(max(counts) * n * widest); d_out = nv.DeviceBuffer(max(counts) * n * 4)
    for streams in counts:
        for name in a.formats.split(","):
            print(json.dumps(run(name, streams, n, max(1, a.reps), d_in, d_out)), flush=True)
    d_in.free(); d_out.free()


if __name__ == "__main__":
    main()
