"""The narrowband interpolator's cases, shared by tests/test_narrow.py (CPU), tests/test_gpu_narrow.py and
tests/test_gpu_narrow_edges.py: the rates whose design is held to the two bars, rows of tones and noise and full-scale random
rows in every format and kind, rows at the rails matched to a phase's taps, and the end-to-end cases -- audio and low-rate IQ
sources, the path each takes and where its chain is tuned.  Nothing is kept: a test that wants several rows at once holds
them itself for as long as it runs.  Behind them what the two GPU files share: the rates whose tap row is three 16-byte words
(or an exact or a six-zero row) and which format and kind runs at each, and the resident call under sentinels (_run_resident,
_same, _first_difference)."""
from __future__ import annotations

import numpy as np

import narrow_ref as nr
import real_cases
import real_ref as rf
import resample_ref as rr
import signals

# (rate_num, rate_den) whose taps are held to the bars
DESIGN_RATES = ((2000, 1), (4000, 1), (11025, 2), (6000, 1), (8000, 1), (11025, 1), (12000, 1), (16000, 1), (22050, 1), (24000, 1),
                (32000, 1), (44100, 1), (48000, 1), (50000, 1), (64000, 1), (88200, 1), (96000, 1), (12500, 1), (7350, 1),
                (72000, 1), (67200, 1), (75600, 1), (70000, 1), (73332, 1), (84000, 1), (64800, 1))
T_OF_RATE = {(64000, 1): 28, (88200, 1): 14, (96000, 1): 12,       # 30 everywhere else
             (72000, 1): 20, (67200, 1): 24, (75600, 1): 18, (70000, 1): 22, (73332, 1): 18, (84000, 1): 16, (64800, 1): 26}

# End to end: amplitude 8000 over noise 1500, signals.stream_text(seed), 40 phasing characters.
#   source: "real" (audio: the I column of the generator) or "iq";  rate: of the source;  station: its centre in the source;
#   path: "converter" (real_ref, then the IQ kind with rate_den 2), "iq" or "real" (the REAL kind);  tuned: the chain's carrier
#   (None: the untuned 518 chain, k = 4480)
E2E = {17: dict(source="real", rate=8000, station=1000.0, path="converter", tuned=-1000.0),
       19: dict(source="real", rate=11025, station=1700.0, path="converter", tuned=-1056.25),
       20: dict(source="iq", rate=12000, station=-1000.0, path="iq", tuned=-1000.0),
       21: dict(source="iq", rate=48000, station=14000.0, path="iq", tuned=None),
       22: dict(source="real", rate=44100, station=1000.0, path="real", tuned=1000.0),
       25: dict(source="real", rate=48000, station=500.0, path="real", tuned=500.0)}
AMPLITUDE, NOISE, PHASING = 8000, 1500, 40


def source(nv, seed: int, station: float | None = None, text: str | None = None) -> np.ndarray:
    """The source row of case `seed`: int16 [n] (real) or [n, 2] (IQ) at the case's rate."""
    case = E2E[seed]
    bits = nv.sitor_encode(text or signals.stream_text(seed), PHASING)
    n = (len(bits) + 300) * case["rate"] // 100
    iq = rr.cpfsk(bits, case["rate"], n, freq_hz=case["station"] if station is None else station, amplitude=AMPLITUDE, noise_amp=NOISE, seed=seed)
    return np.ascontiguousarray(iq[:, 0]) if case["source"] == "real" else iq


def plan_of(seed: int):
    """(rate_num, rate_den, kind) of the interpolator of case `seed`."""
    case = E2E[seed]
    return (case["rate"], 2, nr.IQ) if case["path"] == "converter" else (case["rate"], 1, nr.REAL if case["path"] == "real" else nr.IQ)


def interpolator_input(seed: int, src: np.ndarray) -> np.ndarray:
    """What the interpolator of case `seed` is fed: the converter's output for the first path, the source itself otherwise."""
    if E2E[seed]["path"] == "converter":
        return rf.convert_all(src[:len(src) // 2 * 2])[0]
    return src


# ----------------------------------------------------------------------------------------------------------------- rows
def signal(fmt: int, kind: int, n: int, seed: int) -> np.ndarray:
    """A few tones and noise in format fmt: [n, 2] (IQ) or [n] (REAL)."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    z = 9000 * np.exp(2j * np.pi * (0.07 * k + seed / 7)) + 4000 * np.exp(-2j * np.pi * 0.113 * k) + 2500 * np.exp(2j * np.pi * 0.31 * k)
    a = np.stack([z.real, z.imag], axis=1) + rng.uniform(-3000, 3000, size=(n, 2))
    a16 = np.rint(a).astype(np.int16)
    if fmt == nr.U8:
        out = np.clip(np.rint(a16 / 128.0 + 127.5), 0, 255).astype(np.uint8)
    elif fmt == nr.S8:
        out = np.clip(np.rint(a16 / 128.0), -128, 127).astype(np.int8)
    elif fmt == nr.F32:
        out = (a16 / 32768.0).astype(np.float32)
    else:
        out = a16
    return out if kind == nr.IQ else np.ascontiguousarray(out[:, 0])


def full_scale(fmt: int, kind: int, n: int, seed: int) -> np.ndarray:
    """Full-scale random samples; float32 with the specials of the F32 rule (NaN, +-inf, denormals, exact ties)."""
    flat = real_cases.full_scale(fmt, n * (2 if kind == nr.IQ else 1), seed)
    return flat.reshape(n, 2) if kind == nr.IQ else flat


def rails(taps: np.ndarray, fmt: int, kind: int, windows: int, gap: int = 1) -> np.ndarray:
    """`windows` windows of T samples, `gap` samples of silence between them, each matched in sign to the phase with the
    largest sum of |h|: +full scale where that phase's tap is positive and -full scale where it is negative, every second
    window negated, and Q the negative of I.  Where an output of that phase stands on a window's last sample the sum is
    +-(sum |h|) * full scale."""
    T = taps.shape[1]
    r = int(np.abs(taps.astype(np.int64)).sum(axis=1).argmax())
    sign = np.where(taps[r, ::-1] >= 0, 1, -1)              # sample q - t meets h[r][t]: the window ascends, the taps descend
    dt = nr.DTYPES[fmt]
    lo, hi = (np.float32(-1.0), np.float32(32767.0 / 32768.0)) if fmt == nr.F32 else (np.iinfo(dt).min, np.iinfo(dt).max)
    zero = 128 if fmt == nr.U8 else 0
    rows = []
    for w in range(windows):
        s = sign if w % 2 == 0 else -sign
        i = np.where(s > 0, hi, lo).astype(dt)
        q = np.where(s > 0, lo, hi).astype(dt)
        rows.append(np.stack([i, q], axis=1))
        rows.append(np.full((gap, 2), zero, dtype=dt))
    out = np.concatenate(rows)
    return out if kind == nr.IQ else np.ascontiguousarray(out[:, 0])


# ------------------------------------------------------------------------------------------- the three-word rows (GPU edges)
# (L, M, T) of the rates whose tap row the existing cases never reach: T = 18 .. 24 is three 16-byte words (TQ = 3: T = 24 fills
# the row, the others have Tp - T zero taps in front), T = 16 an exact two-word row, T = 26 a four-word row behind six zeros
EDGE_PLANS = {(72000, 1): (7, 2, 20), (67200, 1): (15, 4, 24), (75600, 1): (10, 3, 18), (70000, 1): (18, 5, 22), (73332, 1): (1000, 291, 18),
              (144000, 2): (7, 2, 20), (84000, 1): (3, 1, 16), (64800, 1): (35, 9, 26)}
_ALL = tuple((fmt, kind) for fmt in (nr.S16, nr.U8, nr.S8, nr.F32) for kind in (nr.IQ, nr.REAL))
# (format, kind) run at each rate: all eight at 72 000 and 67 200, and each of the eight once more at one of the other three
# TQ = 3 rates (two of the issue's six places would leave two kernels at two rates), so that every (format, kind) has three
# rates with a three-word row; 144 000 / 2 is the plan of 72 000 once more
EDGE_RUNS = {(72000, 1): _ALL, (67200, 1): _ALL,
             (75600, 1): ((nr.S16, nr.IQ), (nr.S8, nr.REAL), (nr.F32, nr.IQ)),
             (70000, 1): ((nr.S16, nr.REAL), (nr.U8, nr.IQ), (nr.F32, nr.REAL)),
             (73332, 1): ((nr.U8, nr.REAL), (nr.S8, nr.IQ)),
             (144000, 2): ((nr.S16, nr.IQ),),
             (84000, 1): ((nr.S16, nr.IQ), (nr.F32, nr.REAL)), (64800, 1): ((nr.S16, nr.IQ), (nr.F32, nr.REAL))}
EDGE_STREAMS, EDGE_SAMPLES = 3, 3 * 256 + 37


def edge_rows(rate, fmt: int, kind: int) -> list:
    """The rows of the three-tiles-and-a-ragged-fourth case at `rate`: EDGE_STREAMS x EDGE_SAMPLES samples, a seed each."""
    return [signal(fmt, kind, EDGE_SAMPLES, 100 * fmt + 10 * kind + s + rate[0]) for s in range(EDGE_STREAMS)]


# ------------------------------------------------------------------------------------------------ the resident call (GPU)
SENTINEL = 0x5a5a1234


def _run_resident(nv, c, rows, cuts, pitch_extra=0, out_first=0):
    """The rows (all of one length, in the plan's format and kind) through nvx_nb_resident in calls of `cuts` samples; every
    call's input is uploaded to the start of the input rows as whole rows: behind a call's n_in samples the row is full scale up
    to the pitch, so a read behind n_in changes the output.  Sentinels around every output row.  Returns int16 [streams, outputs, 2]."""
    ns, n = len(rows), len(rows[0])
    assert sum(cuts) == n and ns == c.n_streams
    dt = rows[0].dtype
    comps = 2 if c.kind == nr.IQ else 1
    start = c.position(0)
    n_out = nr.outputs_after(start[0] + n, c.L, c.M) - start[1]
    pitch_out = out_first + n_out + pitch_extra
    pitch_in = (max(max(cuts), 1) + 15) // 16 * 16 + 16 * pitch_extra
    d_in = nv.DeviceBuffer(ns * pitch_in * comps * dt.itemsize)
    d_out = nv.DeviceBuffer(ns * pitch_out * 4)
    d_out.upload(np.full(ns * pitch_out, SENTINEL, dtype=np.uint32))
    block = np.empty((ns, pitch_in * comps), dtype=dt)
    pos = made = 0
    for cut in cuts:
        block[:, cut * comps:] = 1.0 if dt == np.float32 else np.iinfo(dt).max
        for s in range(ns):
            block[s, :cut * comps] = rows[s][pos:pos + cut].reshape(-1)
        d_in.upload(block)
        got = c.resident(d_in, pitch_in, cut, d_out, pitch_out, out_first + made)
        assert got == nr.outputs_after(start[0] + pos + cut, c.L, c.M) - nr.outputs_after(start[0] + pos, c.L, c.M), (pos, cut)
        pos += cut; made += got
    assert made == n_out and c.position(ns - 1) == (start[0] + n, start[1] + n_out)
    words = d_out.download(ns * pitch_out * 4, dtype=np.uint32).reshape(ns, pitch_out)
    d_in.free(); d_out.free()
    assert np.all(words[:, :out_first] == SENTINEL) and np.all(words[:, out_first + n_out:] == SENTINEL), "words outside the span were written"
    return np.ascontiguousarray(words[:, out_first:out_first + n_out]).view(np.int16).reshape(ns, n_out, 2)


def _first_difference(got, want):
    return int(np.argmax(np.any(got != want, axis=1)))


def _same(got, want, what):
    for s in range(len(want)):
        assert got[s].shape == want[s].shape and np.array_equal(got[s], want[s]), (what, s, _first_difference(got[s], want[s]))
