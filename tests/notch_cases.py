"""The tone notch's cases, shared by tests/test_notch.py (CPU) and tests/test_gpu_notch.py: a weak 490 station at -14 kHz of a
252 kS/s row with two carriers inside its chain's passband (the acceptance case), pure tones over nothing, white noise, and the
rows for the restatement's edges: the rails and full-scale random input in every format (the canceller's rows).  Nothing is
kept: a row is 24 MB."""
from __future__ import annotations

import numpy as np

import anc_cases as ac
import notch_ref as nr
import resample_ref as rr

SEEDS = ac.SEEDS
RATE = 252000
CENTRE = -14000.0                           # of the 490 chain in the row
AMP_490, NOISE = 300, 1500
CARRIERS = ((CENTRE + 60.0, 3000.0), (CENTRE - 310.0, 6000.0))      # (hertz, amplitude): between the two tones, and below both
B = nr.BLOCK


def text():
    return ac.text()


def _quantise(z: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(np.stack([z.real, z.imag], axis=1)), -32768, 32767).astype(np.int16)


def carrier(n: int, hz: float, amp: float, rate: float = RATE, phase: float = 0.0) -> np.ndarray:
    """complex [n]: the phase in turns is kept small, so a row of minutes stays exact to the last bits of a double."""
    turns = (np.arange(n, dtype=np.float64) * (hz / rate)) % 1.0
    return amp * np.exp(2j * np.pi * (turns + phase))


def tone(n: int, hz: float, amp: float = 8000.0, rate: float = RATE) -> np.ndarray:
    """A pure tone as int16 [n, 2]."""
    return _quantise(carrier(n, hz, amp, rate))


def white(n: int, amp: float = 6000.0, seed: int = 3) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return _quantise(rng.uniform(-amp, amp, n) + 1j * rng.uniform(-amp, amp, n))


def acceptance_row(nv, seed: int) -> np.ndarray:
    """int16 [n, 2], n whole frames: the 490 station at amplitude 300, the two carriers (each at a phase the seed draws), noise of
    +-1500 per component.  The generator draws the two phases, then the noise's re, then its im."""
    s = ac.station(nv, seed, AMP_490)
    n = len(s)
    rng = np.random.default_rng(3000 + seed)
    phases = rng.uniform(0, 1, len(CARRIERS))
    z = s + rng.uniform(-NOISE, NOISE, n) + 1j * rng.uniform(-NOISE, NOISE, n)
    for (hz, amp), ph in zip(CARRIERS, phases):
        z = z + carrier(n, hz, amp, phase=ph)
    return _quantise(z)


def steps(off_hz: float = 0.0):
    """The steps of two notches set off_hz above the carriers' true frequencies."""
    return [nr.step_from_hz(hz + off_hz, RATE) for hz, _ in CARRIERS]


def delivered(oracle, iq252: np.ndarray, frame_in: int):
    return ac.delivered(oracle, iq252, frame_in)


def power_db(out: np.ndarray, against: np.ndarray) -> float:
    return ac.power_db(out, against)


def busy_row(n: int, seed: int, fmt: int = nr.CS16, k: int = 4):
    """(a row in format fmt, the steps of k notches for it).  Three carriers of 5000 .. 9000 at frequencies the seed draws
    within +-20 kHz over noise of +-2000; the notches sit 3 Hz above the first carrier, 25 Hz below the second, on the third, and
    the fourth where the seed puts it.  Every notch near a carrier has a large, turning amplitude, so a word computed from
    the wrong block or phase shows."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(-2000, 2000, n) + 1j * rng.uniform(-2000, 2000, n)
    hz = rng.uniform(-20000, 20000, 4)
    for f, amp, ph in zip(hz[:3], rng.uniform(5000, 9000, 3), rng.uniform(0, 1, 3)):
        z = z + carrier(n, f, amp, phase=ph)
    at = [hz[0] + 3.0, hz[1] - 25.0, hz[2], hz[3]]
    return rr.to_format(_quantise(z), fmt), [nr.step_from_hz(f, RATE) for f in at[:k]]


def rails(fmt: int, n: int) -> np.ndarray:
    """Every component at the format's lowest value."""
    return ac.extremes(fmt, n, 1)[0][0]


def full_scale(fmt: int, n: int, seed: int) -> np.ndarray:
    """Full-scale random input (float32: the specials of the conversion among it)."""
    return ac.extremes(fmt, n, seed)[2][0]
