#!/usr/bin/env python3
"""Rate of the real-input converter (include/navtex_amd_real.h) against the channeliser: HIP-event time per call
(nvx_real_time_stats / nvx_channelise_time_stats), after a warm-up, over ten calls of each, interleaved in one process
(converter, channeliser, converter, ...), median and minimum.  Shapes: 4096 streams x 3 932 160 real samples (1 966 080
outputs) as int16 and as unsigned 8-bit (one workgroup per stream), and 64 streams of the same length (a stream spread over
workgroups).  The yardstick is nvx_channelise_resident in the same run (it reads every byte of its input once and writes as
many; DESIGN 3 quotes it at 5.1 TB/s read plus write); the chip's streaming figure is the other reference.  The converter's
bytes are one read of every sample and one 4-byte word per output.  Prints one JSON line per shape.  DESIGN 3.11 records them.

    python tools/real_rate.py [--reps 10] [--streams 4096,64] [--outputs 1966080] [--formats s16,u8]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import navtex_amd as nv               # noqa: E402
import navtex_amd.real as rl          # noqa: E402

STREAMING_TB_S = 6.29
FORMATS = {"s16": rl.S16, "u8": rl.U8, "s8": rl.S8, "f32": rl.F32}


def _convert(c, d_in, d_out, n_in):
    c.reset()
    c.resident(d_in, n_in, n_in, d_out, n_in // 2)
    ms, calls = c.time_stats(reset=True)
    assert calls == 1
    return ms


def _channelise(d_chan, d_out, streams, n):
    nv.channelise(d_chan, n, 0, streams, n // 8, d_out, n // 8)
    ms, launches = nv.channelise_time_stats(reset=True)
    assert launches == 1
    return ms


def run(fmt_name, streams, n_out, reps, d_in, d_out, d_chan):
    fmt = FORMATS[fmt_name]
    bps = rl.BYTES_PER_SAMPLE[fmt]
    n_in = 2 * n_out
    # a few tones over noise, the same in every row: the time does not depend on the data
    rng = np.random.default_rng(1)
    k = np.arange(n_in)
    x = 9000 * np.cos(2 * np.pi * 0.27 * k) + 4000 * np.cos(2 * np.pi * 0.113 * k) + rng.uniform(-3000, 3000, size=n_in)
    row = {rl.S16: lambda: np.rint(x).astype(np.int16), rl.U8: lambda: np.clip(np.rint(x / 256 + 127.5), 0, 255).astype(np.uint8),
           rl.S8: lambda: np.clip(np.rint(x / 256), -128, 127).astype(np.int8), rl.F32: lambda: (x / 32768.0).astype(np.float32)}[fmt]()
    for s in range(streams):
        d_in.upload(row, s * n_in * bps)
    with rl.Converter(fmt, n_streams=streams) as c:
        c.timing(True)
        _convert(c, d_in, d_out, n_in); _channelise(d_chan, d_out, streams, n_out)                # warm-up
        t_r, t_c = [], []
        for _ in range(reps):
            t_r.append(_convert(c, d_in, d_out, n_in))
            t_c.append(_channelise(d_chan, d_out, streams, n_out))
        shape = c.debug_last_launch()
    mr, mc = statistics.median(t_r), statistics.median(t_c)
    real_bytes = streams * n_out * (2 * bps + 4)
    chan_bytes = streams * n_out * 8
    real_tb, chan_tb = real_bytes / (mr * 1e-3) / 1e12, chan_bytes / (mc * 1e-3) / 1e12
    return {"format": fmt_name, "streams": streams, "samples_per_stream": n_in, "outputs_per_stream": n_out, "runs_each": reps,
            "real_ms_median": round(mr, 4), "real_ms_min": round(min(t_r), 4), "channelise_ms_median": round(mc, 4),
            "channelise_ms_min": round(min(t_c), 4), "real_GB_read_plus_write": round(real_bytes / 1e9, 3), "real_TB_per_s": round(real_tb, 3),
            "channelise_TB_per_s": round(chan_tb, 3), "real_over_channelise_bytes_per_s": round(real_tb / chan_tb, 3),
            "of_streaming": round(real_tb / STREAMING_TB_S, 3), "streaming_TB_per_s": STREAMING_TB_S,
            "G_outputs_per_s": round(streams * n_out / (mr * 1e-3) / 1e9, 1), "chunks": shape["chunks"], "tiles_per_chunk": shape["tiles_per_chunk"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--streams", default="4096,64")
    ap.add_argument("--outputs", type=int, default=1966080)
    ap.add_argument("--formats", default="s16,u8")
    a = ap.parse_args()
    n_out = a.outputs // 512 * 512                           # the channeliser takes multiples of 64 outputs
    counts = [int(s) for s in a.streams.split(",")]
    nv.lib.nvx_channelise_timing(1)
    widest = max(rl.BYTES_PER_SAMPLE[FORMATS[name]] for name in a.formats.split(","))
    d_in = nv.DeviceBuffer(max(counts) * 2 * n_out * widest)
    d_out = nv.DeviceBuffer(max(counts) * n_out * 4)
    d_chan = nv.DeviceBuffer(max(counts) * n_out * 4)        # the channeliser's input: as many int16 IQ samples as outputs
    for streams in counts:
        for name in a.formats.split(","):
            print(json.dumps(run(name, streams, n_out, max(1, a.reps), d_in, d_out, d_chan)), flush=True)
    d_in.free(); d_out.free(); d_chan.free()


if __name__ == "__main__":
    main()
