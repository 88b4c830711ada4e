#!/usr/bin/env python3
"""Rate of the narrowband interpolator (include/navtex_amd_narrow.h): HIP-event time per call (nvx_nb_time_stats), after a
warm-up, over ten calls, median and minimum.  Shapes: 4096 streams x 1 s at 12 kS/s CS16, 8 kS/s REAL S16, 48 kS/s CS16 and
11.025 kS/s CU8 (one workgroup per stream), and 64 streams x 1 s at 12 kS/s (a stream spread over workgroups).  The yardstick
is the existing resampler at 96 kS/s CS16 beside the new kernel at 96 kS/s CS16, interleaved in one process: both have T = 12,
the same output count and the same bytes.  The bytes are one read of every input sample and one 4-byte word per output.  Per
output the kernel issues T' = 8 ceil(T / 8) int16 dot products per component (two components for IQ, one for REAL) and reads
16 ceil(T / 8) bytes of taps from the LDS; both are printed.  Every shape runs in a process of its own under a time limit, and
the first that fails ends the run.  Prints one JSON line per shape.  DESIGN 3.12 records them.

    python tools/narrow_rate.py [--reps 10] [--seconds 1.0] [--limit 120]"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
STREAMING_TB_S = 6.29
# name: (streams, rate, format, kind)
SHAPES = {"12k_cs16": (4096, 12000, "s16", "iq"), "8k_real_s16": (4096, 8000, "s16", "real"), "48k_cs16": (4096, 48000, "s16", "iq"),
          "11k025_cu8": (4096, 11025, "u8", "iq"), "12k_cs16_64": (64, 12000, "s16", "iq"), "96k_cs16_yardstick": (4096, 96000, "s16", "iq")}


def _row(np, nb, rate, fmt, kind, n):
    """A few tones over noise, the same in every row: the time does not depend on the data."""
    rng = np.random.default_rng(1)
    k = np.arange(n)
    z = 9000 * np.exp(2j * np.pi * 0.07 * k) + 4000 * np.exp(-2j * np.pi * 0.113 * k)
    a = np.stack([z.real, z.imag], axis=1) + rng.uniform(-3000, 3000, size=(n, 2))
    if fmt == nb.U8:
        out = np.clip(np.rint(a / 256 + 127.5), 0, 255).astype(np.uint8)
    else:
        out = np.rint(a).astype(np.int16)
    return out if kind == nb.IQ else np.ascontiguousarray(out[:, 0])


def run(name, reps, seconds):
    import numpy as np
    sys.path.insert(0, str(ROOT))
    import navtex_amd as nv
    import navtex_amd.narrow as nb
    streams, rate, fmt_name, kind_name = SHAPES[name]
    fmt, kind = {"s16": nb.S16, "u8": nb.U8}[fmt_name], {"iq": nb.IQ, "real": nb.REAL}[kind_name]
    n_in = int(rate * seconds) // 16 * 16
    bps = nb.BYTES_PER_SAMPLE[kind][fmt]
    row = _row(np, nb, rate, fmt, kind, n_in)
    d_in = nv.DeviceBuffer(streams * n_in * bps)
    for s in range(streams):
        d_in.upload(row, s * n_in * bps)
    with nb.Interpolator(rate, format=fmt, kind=kind, n_streams=streams) as c:
        n_out = nb.out_count(c.L, c.M, 0, n_in)
        d_out = nv.DeviceBuffer(streams * n_out * 4)
        c.timing(True)

        def narrow():
            c.reset()
            assert c.resident(d_in, n_in, n_in, d_out, n_out) == n_out
            ms, calls = c.time_stats(reset=True)
            assert calls == 1
            return ms

        other = None
        if name.endswith("yardstick"):
            import navtex_amd.resample as rs
            r = rs.Resampler(rate, rs.CS16, n_streams=streams)
            r.timing(True)

            def other():
                r.reset()
                assert r.resident(d_in, n_in, n_in, d_out, n_out) == n_out
                ms, launches = r.time_stats(reset=True)
                assert launches == 1
                return ms

        narrow()                                            # warm-up
        if other:
            other()
        t_n, t_o = [], []
        for _ in range(reps):
            t_n.append(narrow())
            if other:
                t_o.append(other())
        shape = c.debug_last_launch()
        tq = (c.T + 7) // 8
        out = {"shape": name, "streams": streams, "rate": rate, "format": fmt_name, "kind": kind_name, "L": c.L, "M": c.M, "T": c.T,
               "samples_per_stream": n_in, "outputs_per_stream": n_out, "runs": reps}
    mn = statistics.median(t_n)
    nbytes = streams * (n_in * bps + n_out * 4)
    out.update({"narrow_ms_median": round(mn, 4), "narrow_ms_min": round(min(t_n), 4), "GB_read_plus_write": round(nbytes / 1e9, 3),
                "narrow_TB_per_s": round(nbytes / (mn * 1e-3) / 1e12, 3), "of_streaming": round(nbytes / (mn * 1e-3) / 1e12 / STREAMING_TB_S, 3),
                "G_outputs_per_s": round(streams * n_out / (mn * 1e-3) / 1e9, 2),
                "dot2_per_output": 8 * tq * (2 if kind == nb.IQ else 1), "lds_tap_bytes_per_output": 16 * tq,
                "chunks": shape["chunks"], "tiles_per_chunk": shape["tiles_per_chunk"], "windows": shape["windows"], "lds_bytes": shape["lds_bytes"]})
    if other:
        mo = statistics.median(t_o)
        out.update({"resampler_ms_median": round(mo, 4), "resampler_ms_min": round(min(t_o), 4),
                    "resampler_TB_per_s": round(nbytes / (mo * 1e-3) / 1e12, 3), "narrow_over_resampler_time": round(mn / mo, 3)})
        r.close()
    d_in.free(); d_out.free()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--limit", type=int, default=120, help="seconds a shape may take")
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
