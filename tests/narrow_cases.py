"""The narrowband interpolator's cases, shared by tests/test_narrow.py (CPU) and tests/test_gpu_narrow.py: the rates whose
design is held to the two bars, rows of tones and noise and full-scale random rows in every format and kind, rows at the
rails matched to a phase's taps, and the end-to-end cases -- audio and low-rate IQ sources, the path each takes and where its
chain is tuned.  Nothing is kept: a test that wants several rows at once holds them itself for as long as it runs."""
from __future__ import annotations

import numpy as np

import narrow_ref as nr
import real_cases
import real_ref as rf
import resample_ref as rr
import signals

# (rate_num, rate_den) whose taps are held to the bars
DESIGN_RATES = ((2000, 1), (4000, 1), (11025, 2), (6000, 1), (8000, 1), (11025, 1), (12000, 1), (16000, 1), (22050, 1), (24000, 1),
                (32000, 1), (44100, 1), (48000, 1), (50000, 1), (64000, 1), (88200, 1), (96000, 1), (12500, 1), (7350, 1))
T_OF_RATE = {(64000, 1): 28, (88200, 1): 14, (96000, 1): 12}       # 30 everywhere else

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
