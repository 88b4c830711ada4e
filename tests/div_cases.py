"""The diversity combiner's cases, shared by tests/test_div.py (CPU) and tests/test_gpu_div.py: a 490 station at -14 kHz of a
252 kS/s row that fades on two antennas in quadrature (the acceptance case), a static pair whose weight is known, and the rows
for the restatement's edges: a tone whose stronger branch changes, silence, rails and full-scale random input in every format
(the canceller's, tests/anc_cases.py).  Nothing is kept: a row is 24 MB."""
from __future__ import annotations

import numpy as np

import anc_cases as ac
import div_ref as dr
import resample_ref as rr

SEEDS = ac.SEEDS
RATE = ac.RATE
AMP_490 = 300
NOISE = 1500
FADE_S = 8.0
PHASE_A, PHASE_B = 0.7, 2.1
STEP_490 = dr.step_from_hz(-14000, RATE)
STATIC_GAIN = 0.5 * np.exp(1.0j)            # the station on the second antenna against the main antenna
STATIC_WEIGHT = (2213, -3447)               # rint(8192 * conj(STATIC_GAIN)): what turns the second row onto the main row, in Q13
C = dr.CELL

text, delivered, extremes = ac.text, ac.delivered, ac.extremes


def fading_pair(nv, seed: int, noise: float = NOISE, period_s: float = FADE_S):
    """(main, second) as int16 [n, 2], n whole frames: main = cos(2 pi t / period) e^{j 0.7} s + e1, second = sin(2 pi t / period)
    e^{j 2.1} s + e2, with s the 490 station at amplitude 300 and e1, e2 each receiver's own noise (+-noise per component).  The
    generator draws the re and im of e1, then of e2."""
    s = ac.station(nv, seed, AMP_490)
    n = len(s)
    t = np.arange(n) / RATE
    rng = np.random.default_rng(2000 + seed)
    e1 = rng.uniform(-noise, noise, n) + 1j * rng.uniform(-noise, noise, n)
    e2 = rng.uniform(-noise, noise, n) + 1j * rng.uniform(-noise, noise, n)
    a = np.cos(2 * np.pi * t / period_s) * np.exp(1j * PHASE_A) * s + e1
    b = np.sin(2 * np.pi * t / period_s) * np.exp(1j * PHASE_B) * s + e2
    return ac._quantise(a), ac._quantise(b)


def static_pair(nv, seed: int, amp: float = 3000, noise: float = 300):
    """The station at gain 1 on the main row and 0.5 e^{j 1.0} on the second, over own noise of +-noise."""
    s = ac.station(nv, seed, amp)[:6 * C]
    n = len(s)
    rng = np.random.default_rng(3000 + seed)
    e1 = rng.uniform(-noise, noise, n) + 1j * rng.uniform(-noise, noise, n)
    e2 = rng.uniform(-noise, noise, n) + 1j * rng.uniform(-noise, noise, n)
    return ac._quantise(s + e1), ac._quantise(STATIC_GAIN * s + e2)


# ------------------------------------------------------------------------------------------ rows for the restatement's edges
def tones_pair(n: int, seed: int, steps, amp: float = 5000, noise: float = 400, flip_every: int = 50000):
    """A tone at each of `steps` (phase steps per sample) whose two paths change every flip_every samples (gains 0.1 .. 1, any
    phase, drawn per tone and row), over own noise: every window solves to another weight, the stronger branch changes from
    window to window, and a sample given the wrong cell's weight shows in the output."""
    rng = np.random.default_rng(seed)
    k = n // flip_every + 1
    idx = np.arange(n)
    a = rng.uniform(-noise, noise, n) + 1j * rng.uniform(-noise, noise, n)
    b = rng.uniform(-noise, noise, n) + 1j * rng.uniform(-noise, noise, n)
    for step in steps:
        signed = step - (1 << 32) if step >= 1 << 31 else step
        tone = amp / max(len(steps), 1) * np.exp(2j * np.pi * ((signed * idx) % (1 << 32)) / 4294967296.0)
        ga = (rng.uniform(0.1, 1.0, size=k) * np.exp(1j * rng.uniform(0, 2 * np.pi, size=k)))[idx // flip_every]
        gb = (rng.uniform(0.1, 1.0, size=k) * np.exp(1j * rng.uniform(0, 2 * np.pi, size=k)))[idx // flip_every]
        a += ga * tone
        b += gb * tone
    return ac._quantise(a), ac._quantise(b)


def formatted_tones(n: int, seed: int, steps, fmt: int):
    """tones_pair requantised to the format a radio of that kind delivers (three times the level for the 8-bit formats)."""
    a, b = tones_pair(n, seed, steps)
    gain = 3.0 if fmt in (rr.CU8, rr.CS8) else 1.0
    return rr.to_format(a, fmt, gain=gain), rr.to_format(b, fmt, gain=gain)


def silence_then_tone(n: int, seed: int, step: int, silent: int):
    """Both rows all zero for `silent` samples (reason 1 for the windows inside), then tones_pair."""
    a, b = tones_pair(n, seed, [step])
    a[:silent] = 0
    b[:silent] = 0
    return a, b
