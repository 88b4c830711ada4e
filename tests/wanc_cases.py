"""The multi-tap canceller's cases, shared by tests/test_wanc.py (CPU) and tests/test_gpu_wanc.py: the canceller's acceptance
case (tests/anc_cases.py: a weak 490 station at -14 kHz under local broadband noise that a sense antenna hears too) with the
noise reaching the main antenna over three echoes and the sense antenna over one, the pure-noise rows of the null depth over
the same two paths, and the rows for the restatement's edges: a path that changes, rejection reasons, rails.  Nothing is kept:
a row is 24 MB."""
from __future__ import annotations

import numpy as np

import anc_cases as ac
import resample_ref as rr
import wanc_ref as wr

SEEDS = ac.SEEDS
B = wr.BLOCK
OMEGA = -2 * np.pi * 14000 / ac.RATE
MAIN_PATH = (1.0, 0.7 * np.exp(1j * (OMEGA + 0.5)), 0.5 * np.exp(1j * (2 * OMEGA + 0.5)), 0.3 * np.exp(1j * (3 * OMEGA + 0.5)))
SENSE_PATH = (1.0, 0.15 * np.exp(0.5j))


def through(path, loc: np.ndarray) -> np.ndarray:
    """sum_i path[i] L[n - i], L = 0 in front of the row."""
    out = np.zeros(len(loc), dtype=np.complex128)
    for i, h in enumerate(path):
        out[i:] += h * loc[:len(loc) - i]
    return out


def pair(nv, seed: int, amp: float = ac.AMP_490, noise: float = ac.NOISE, own: float = ac.OWN):
    """anc_cases.pair's signals and draw order (the re and im of L, then of e1, then of e2); the common noise reaches the main
    row over MAIN_PATH and the sense row as NOISE_GAIN times L over SENSE_PATH."""
    s = ac.station(nv, seed, amp)
    n = len(s)
    rng = np.random.default_rng(1000 + seed)
    loc = rng.uniform(-noise, noise, n) + 1j * rng.uniform(-noise, noise, n)
    e1 = rng.uniform(-own, own, n) + 1j * rng.uniform(-own, own, n)
    e2 = rng.uniform(-own, own, n) + 1j * rng.uniform(-own, own, n)
    return ac._quantise(s + through(MAIN_PATH, loc) + e1), ac._quantise(ac.STATION_GAIN * s + ac.NOISE_GAIN * through(SENSE_PATH, loc) + e2)


def noise_pair(n: int, own: float, seed: int = 5, amp: float = ac.NOISE, echoes: bool = True):
    """Pure common noise over the two paths (or, without echoes, anc_cases.noise_pair's), no station, own noise +-own."""
    rng = np.random.default_rng(seed)
    loc = rng.uniform(-amp, amp, n) + 1j * rng.uniform(-amp, amp, n)
    e1 = rng.uniform(-own, own, n) + 1j * rng.uniform(-own, own, n) if own else 0
    e2 = rng.uniform(-own, own, n) + 1j * rng.uniform(-own, own, n) if own else 0
    if not echoes:
        return ac._quantise(loc + e1), ac._quantise(ac.NOISE_GAIN * loc + e2)
    return ac._quantise(through(MAIN_PATH, loc) + e1), ac._quantise(ac.NOISE_GAIN * through(SENSE_PATH, loc) + e2)


def band_db(out: np.ndarray, against: np.ndarray, freq_hz: float, half_width_hz: float = 500.0) -> float:
    """The power of `out` against that of `against` inside freq_hz +- half_width_hz of a 252 kS/s row, in dB (Hann-windowed
    segments of 65536 samples, averaged)."""
    def spectrum(x):
        z = (x.astype(np.float64) @ (1, 1j))[:len(x) // B * B].reshape(-1, B) * np.hanning(B)
        return (np.abs(np.fft.fft(z, axis=1)) ** 2).sum(axis=0)
    f = np.fft.fftfreq(B, 1.0 / ac.RATE)
    sel = np.abs(f - freq_hz) <= half_width_hz
    return 10 * np.log10(max(spectrum(out)[sel].sum(), 1e-9) / spectrum(against)[sel].sum())


def delayed(a: np.ndarray, G: int) -> np.ndarray:
    """The main row as the canceller's output carries it: G samples late, zeros in front."""
    return np.concatenate([np.zeros((G, 2), dtype=a.dtype), a])[:len(a)]


# ------------------------------------------------------------------------------------------ rows for the restatement's edges
def drifting_pair(n: int, seed: int, amp: int = 5000):
    """Common noise over paths of three echoes that change every 50 000 samples, over own noise of +-200: every window solves to
    other weights, so a sample given the wrong block's weights shows in the output."""
    rng = np.random.default_rng(seed)
    k = n // 50000 + 1
    loc = rng.uniform(-amp, amp, n) + 1j * rng.uniform(-amp, amp, n)
    seg = np.arange(n) // 50000
    main = np.zeros(n, dtype=np.complex128)
    for i in range(3):
        h = (rng.uniform(0.2, 0.7, size=k) * np.exp(1j * rng.uniform(0, 2 * np.pi, size=k)))[seg]
        main[i:] += h[i:] * loc[:n - i]
    g = (rng.uniform(0.5, 1.2, size=k) * np.exp(1j * rng.uniform(0, 2 * np.pi, size=k)))[seg]
    e1 = rng.uniform(-200, 200, n) + 1j * rng.uniform(-200, 200, n)
    e2 = rng.uniform(-200, 200, n) + 1j * rng.uniform(-200, 200, n)
    return ac._quantise(main + e1), ac._quantise(g * loc + e2)


def formatted_pair(n: int, seed: int, fmt: int):
    """drifting_pair requantised to the format a radio of that kind delivers (three times the level for the 8-bit formats)."""
    a, b = drifting_pair(n, seed)
    gain = 3.0 if fmt in (rr.CU8, rr.CS8) else 1.0
    return rr.to_format(a, fmt, gain=gain), rr.to_format(b, fmt, gain=gain)


def silent_sense(n: int):
    """Reason 1: the main row at the rails, the sense row all zero."""
    return ac.rails(n), np.zeros((n, 2), dtype=np.int16)


def edge_sense(n: int):
    """Reason 2 at the start of block 6 (W = 4): a faint sense row (3, 3) with one strong sample (3000, 0) at the first sample
    of block 2 and a full-scale one (32767, 0) in front of it, outside the window of blocks 2 .. 5.  Their product is in
    r[1] and the full-scale sample's power is not in r[0]: |r[1]| > r[0] + lambda, no autocorrelation, and the second pivot is
    negative.  The windows of blocks 0 .. 3 and 1 .. 4 hold both samples: their matrices are sound, and against a main row at
    the rails they want weights beyond the bounds (reason 3)."""
    b = np.full((n, 2), 3, dtype=np.int16)
    b[2 * B - 1] = (32767, 0)
    b[2 * B] = (3000, 0)
    return ac.rails(n), b


def weak_white_sense(n: int, seed: int = 9):
    """Reason 3: white noise of +-600 on the sense row and sixteen times it, one sample late, on the main row: w_1 wants 16.0."""
    rng = np.random.default_rng(seed)
    b = rng.integers(-600, 601, size=(n, 2)).astype(np.int16)
    a = np.zeros((n, 2), dtype=np.int16)
    a[1:] = 16 * b[:-1]
    return a, b
