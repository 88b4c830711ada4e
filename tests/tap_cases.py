"""The channel tap's cases, shared by tests/test_tap.py (CPU) and tests/test_gpu_tap.py: the rates whose design is held to the
two bars, rows of tones and noise and full-scale random rows, rows at the rails matched to a phase's taps, and the end-to-end
cases -- a 252 kS/s row with stations, the taps that take them out, the way back through the interpolator and where the chain
is tuned.  Nothing is kept: a test that wants several rows at once holds them itself for as long as it runs."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import resample_ref as rr
import signals
import tap_ref as tp

IQ_RATES = (2000, 6250, 8000, 11025, 12000, 24000, 48000, 96000)
REAL_RATES = (8000, 11025, 12000, 44100, 48000)
DESIGNS = tuple((fo, tp.IQ) for fo in IQ_RATES) + tuple((fo, tp.REAL) for fo in REAL_RATES)
# recorded from the C design: (L, M, T)
PLAN_OF = {(2000, tp.IQ): (1, 126, 3602), (6250, tp.IQ): (25, 1008, 1154), (8000, tp.IQ): (2, 63, 902), (11025, tp.IQ): (7, 160, 654),
           (12000, tp.IQ): (1, 21, 602), (24000, tp.IQ): (2, 21, 302), (48000, tp.IQ): (4, 21, 152), (96000, tp.IQ): (8, 21, 32),
           (8000, tp.REAL): (2, 63, 3602), (11025, tp.REAL): (7, 160, 3602), (12000, tp.REAL): (1, 21, 3602), (44100, tp.REAL): (7, 40, 3602),
           (48000, tp.REAL): (4, 21, 3602)}

# End to end: stations of amplitude 8000 over noise 1500 in a 252 kS/s row, signals.stream_text(seed), 40 phasing characters.
#   stations: {seed: centre in the row};  rate, kind: of the tap;  back: how the tap's output returns to 252 kS/s --
#   "iq" (narrow_ref's IQ kind), "real" (its REAL kind) or "converter" (real_ref, then the IQ kind with rate_den 2)
E2E = {"i": dict(stations={31: 14000.0, 32: -14000.0}, rate=12000, kind=tp.IQ, back="iq"),
       "ii": dict(stations={33: 14000.0, 34: -14000.0}, rate=48000, kind=tp.IQ, back="iq"),
       "iii": dict(stations={35: 14000.0}, rate=8000, kind=tp.REAL, back="real"),
       "iv": dict(stations={36: 14000.0}, rate=11025, kind=tp.REAL, back="converter"),
       "v": dict(stations={37: 9371.0}, rate=12000, kind=tp.IQ, back="iq")}
AMPLITUDE, NOISE, PHASING = 8000, 1500, 40


def text(seed: int, short: bool = False) -> str:
    """The station's message: signals.stream_text(seed), or a message of one short line (the device tests: a fifth of the row)."""
    if not short:
        return signals.stream_text(seed)
    return f"ZCZC {chr(ord('A') + seed % 26)}{chr(ord('A') + (seed // 26) % 26)}{seed % 100:02d}\nTAP {seed}\nNNNN\n"


def row(nv, case: str, short: bool = False) -> np.ndarray:
    """The 252 kS/s row of the case: int16 [n, 2], its stations summed, noise once."""
    c = E2E[case]
    bits = {seed: nv.sitor_encode(text(seed, short), PHASING) for seed in c["stations"]}
    n = (max(len(b) for b in bits.values()) + 300) * 2520
    total = np.zeros((n, 2), dtype=np.int32)
    for i, (seed, hz) in enumerate(c["stations"].items()):
        total += rr.cpfsk(bits[seed], tp.INPUT_RATE, n, freq_hz=hz, amplitude=AMPLITUDE, noise_amp=NOISE if i == 0 else 0, seed=seed, bit_offset=777 * i)
    return np.clip(total, -32768, 32767).astype(np.int16)


def tuned_hz(case: str, hz: float, k: int, kp: int | None = None) -> float:
    """Where the chain behind the way back is tuned for a station at `hz` taken by a tap at grid step k (and pitch step kp): the
    shift's residue; for audio on top of the applied pitch; through the converter a quarter of the audio rate lower."""
    c = E2E[case]
    residue = Fraction(hz) - Fraction(k * tp.INPUT_RATE, tp.N)
    if c["kind"] == tp.REAL:
        residue += Fraction(kp * c["rate"], tp.N)
        if c["back"] == "converter":
            residue -= Fraction(c["rate"], 4)
    return float(residue)


# ----------------------------------------------------------------------------------------------------------------- rows
def signal(n: int, seed: int) -> np.ndarray:
    """A few tones and noise: int16 [n, 2]."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    z = 9000 * np.exp(2j * np.pi * (0.0007 * k + seed / 7)) + 4000 * np.exp(-2j * np.pi * 0.0113 * k) + 2500 * np.exp(2j * np.pi * 0.31 * k)
    a = np.stack([z.real, z.imag], axis=1) + rng.uniform(-3000, 3000, size=(n, 2))
    return np.rint(a).astype(np.int16)


def full_scale(n: int, seed: int) -> np.ndarray:
    """Full-scale random samples, -32768 among them: int16 [n, 2]."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-32768, 32768, size=(n, 2)).astype(np.int16)
    a[rng.integers(0, n, size=n // 16)] = (-32768, 32767)
    return a


def rails(taps: np.ndarray, L: int, M: int, windows: int) -> np.ndarray:
    """`windows` windows of T samples with silence between them, each matched in sign to the phase r with the largest sum of
    |h|: +full scale where that phase's tap is positive and -full scale where it is negative, every second window negated,
    and Q the negative of I.  A decimator stands on few samples: every window ends on the q of an output of phase r, so
    that output's sum is +-(sum |h|) * full scale (through a tap with k = 0: the mixer would turn the signs away)."""
    T = taps.shape[1]
    r = int(np.abs(taps.astype(np.int64)).sum(axis=1).argmax())
    sign = np.where(taps[r, ::-1] >= 0, 1, -1)              # sample q - t meets h[r][t]: the window ascends, the taps descend
    ends, n, free = [], 0, T - 1
    while len(ends) < windows:
        if (n * M) % L == r and (n * M) // L >= free:
            ends.append((n * M) // L)
            free = ends[-1] + T + 1
        n += 1
    out = np.zeros((ends[-1] + 3, 2), dtype=np.int16)
    for w, q in enumerate(ends):
        s = sign if w % 2 == 0 else -sign
        out[q - T + 1:q + 1, 0] = np.where(s > 0, 32767, -32768)
        out[q - T + 1:q + 1, 1] = np.where(s > 0, -32768, 32767)
    return out
