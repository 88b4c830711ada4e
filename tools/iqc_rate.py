#!/usr/bin/env python3
"""Rate of the IQ corrector (include/navtex_amd_iqc.h) against the channeliser: HIP-event time per call (both kernels and the
zeroing of the block records: nvx_iqc_time_stats / nvx_channelise_time_stats), after a warm-up, over ten calls of each,
interleaved in one process (corrector, channeliser, corrector, ...), median and minimum.  Shapes: 4096 streams x 1 966 080
samples as int16 and as unsigned 8-bit (one workgroup per stream), and 64 streams of the same length (a stream spread over
workgroups); with --samples-per-call the same rows go through in calls that short, which is how to see whether the second
read of a small call comes from the 256 MB infinity cache.  The yardstick is nvx_channelise_resident on the same device
buffers in the same run (it reads every byte once and writes as many; DESIGN 3 quotes it at 5.1 TB/s read plus write); the
chip's streaming figure is the other reference.  The corrector's bytes are counted as two reads and one write of every sample.
Prints one JSON line per shape.  DESIGN 3.10 and profiles/TUNING.md record them.

    python tools/iqc_rate.py [--reps 10] [--streams 4096,64] [--samples 1966080] [--formats cs16,cu8] [--samples-per-call 0]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import navtex_amd as nv               # noqa: E402
import navtex_amd.iqc as iq           # noqa: E402

STREAMING_TB_S = 6.29
FORMATS = {"cs16": iq.CS16, "cu8": iq.CU8, "cs8": iq.CS8, "cf32": iq.CF32}


class _At:
    def __init__(self, ptr):
        self.ptr = ptr


def _correct(c, d_in, d_out, n, per_call, bps):
    c.reset()
    for at in range(0, n, per_call):
        k = min(per_call, n - at)
        c.resident(_At(d_in.ptr + at * bps), n, k, d_out, n, at)
    ms, calls = c.time_stats(reset=True)
    assert calls == (n + per_call - 1) // per_call
    return ms


def _channelise(d_in, d_out, streams, n):
    nv.channelise(d_in, n, 0, streams, n // 8, d_out, n // 8)
    ms, launches = nv.channelise_time_stats(reset=True)
    assert launches == 1
    return ms


def run(fmt_name, streams, n, reps, per_call, d_in, d_out):
    fmt = FORMATS[fmt_name]
    bps = iq.BYTES_PER_SAMPLE[fmt]
    # uniform noise through a gain and phase error with an offset, the same in every row: the time does not depend on the data
    rng = np.random.default_rng(1)
    x = rng.integers(-6000, 6001, size=(n, 2)).astype(np.float64)
    x = np.stack([x[:, 0] + 300, 1.05 * (x[:, 1] * np.cos(np.deg2rad(3)) + x[:, 0] * np.sin(np.deg2rad(3))) - 200], axis=1)
    row = {iq.CS16: lambda: np.rint(x).astype(np.int16), iq.CU8: lambda: np.clip(np.rint(x * 3 / 256 + 127.5), 0, 255).astype(np.uint8),
           iq.CS8: lambda: np.clip(np.rint(x * 3 / 256), -128, 127).astype(np.int8), iq.CF32: lambda: (x / 32768.0).astype(np.float32)}[fmt]()
    for s in range(streams):
        d_in.upload(row, s * n * bps)
    per_call = per_call or n
    with iq.Corrector(fmt, n_streams=streams) as c:
        c.timing(True)
        _correct(c, d_in, d_out, n, per_call, bps); _channelise(d_in, d_out, streams, n)            # warm-up
        t_q, t_c = [], []
        for _ in range(reps):
            t_q.append(_correct(c, d_in, d_out, n, per_call, bps))
            t_c.append(_channelise(d_in, d_out, streams, n))
        shape = c.debug_last_launch()
        status = c.get(0)
    mq, mc = statistics.median(t_q), statistics.median(t_c)
    iqc_bytes = streams * n * (2 * bps + 4)
    chan_bytes = streams * n * 8                             # the channeliser reads the buffer as int16 whatever it holds
    iqc_tb, chan_tb = iqc_bytes / (mq * 1e-3) / 1e12, chan_bytes / (mc * 1e-3) / 1e12
    return {"format": fmt_name, "streams": streams, "samples_per_stream": n, "samples_per_call": per_call, "runs_each": reps,
            "iqc_ms_median": round(mq, 4), "iqc_ms_min": round(min(t_q), 4), "channelise_ms_median": round(mc, 4),
            "channelise_ms_min": round(min(t_c), 4), "iqc_GB_two_reads_one_write": round(iqc_bytes / 1e9, 3), "iqc_TB_per_s": round(iqc_tb, 3),
            "channelise_TB_per_s": round(chan_tb, 3), "iqc_over_channelise_bytes_per_s": round(iqc_tb / chan_tb, 3),
            "of_streaming": round(iqc_tb / STREAMING_TB_S, 3), "streaming_TB_per_s": STREAMING_TB_S,
            "of_streaming_if_the_second_read_is_cached": round(streams * n * (bps + 4) / (mq * 1e-3) / 1e12 / STREAMING_TB_S, 3),
            "chunks": shape["chunks"], "tiles_per_chunk": shape["tiles_per_chunk"], "records": shape["records"],
            "coefficients_stream0": status["coefficients"], "blocks_solved_stream0": status["blocks_solved"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--streams", default="4096,64")
    ap.add_argument("--samples", type=int, default=1966080)
    ap.add_argument("--formats", default="cs16,cu8")
    ap.add_argument("--samples-per-call", type=int, default=0)
    a = ap.parse_args()
    n = a.samples // 512 * 512                               # the channeliser takes multiples of 64 outputs
    per_call = a.samples_per_call // 8 * 8                   # every call's rows start 16-byte aligned
    counts = [int(s) for s in a.streams.split(",")]
    nv.lib.nvx_channelise_timing(1)
    widest = max(4, *(iq.BYTES_PER_SAMPLE[FORMATS[name]] for name in a.formats.split(",")))        # the channeliser reads 4 bytes a sample
    d_in = nv.DeviceBuffer(max(counts) * n * widest); d_out = nv.DeviceBuffer(max(counts) * n * 4)
    for streams in counts:
        for name in a.formats.split(","):
            print(json.dumps(run(name, streams, n, max(1, a.reps), per_call, d_in, d_out)), flush=True)
    d_in.free(); d_out.free()


if __name__ == "__main__":
    main()
