"""The row aligner's cases, shared by tests/test_align.py (CPU) and tests/test_gpu_align.py: common noise confined to a share
of the band with the sense row delayed by any number of samples (the estimator's trials), the canceller's acceptance case
(tests/anc_cases.py) with that noise and a sense row that starts 137.4 samples late, and the rows for the restatement's
edges.  Nothing is kept."""
from __future__ import annotations

import numpy as np

import anc_cases as ac
import resample_ref as rr

SEEDS = ac.SEEDS
BAND = 0.8                                  # the share of the band the common noise fills
DELAY = 137.4                               # samples by which the acceptance case's sense row lags
LAG_FIRST, N_LAGS, MEASURE_N = 0, 256, 65536 + 255     # the acceptance case's measurement: lags 0 .. 255 over N = 65 536


def delayed(z: np.ndarray, delay: float) -> np.ndarray:
    """z delayed by `delay` samples (any real number), circularly: a phase ramp over its spectrum."""
    f = np.fft.fftfreq(len(z))
    return np.fft.ifft(np.fft.fft(z) * np.exp(-2j * np.pi * f * delay))


def band_noise(n: int, amp: float, band: float, rng) -> np.ndarray:
    """Uniform noise of +-amp per component with everything outside |f| <= band / 2 of the rate removed."""
    z = rng.uniform(-amp, amp, n) + 1j * rng.uniform(-amp, amp, n)
    if band >= 1.0:
        return z
    spec = np.fft.fft(z)
    spec[np.abs(np.fft.fftfreq(n)) > band / 2] = 0
    return np.fft.ifft(spec)


def noise_pair(n: int, delay: float, seed: int, band: float = BAND, amp: float = 6000, own: float = 150, gain: complex = ac.NOISE_GAIN):
    """(main, sense) as int16 [n, 2]: main = L + e1, sense = gain * L delayed by `delay` + e2."""
    rng = np.random.default_rng(seed)
    loc = band_noise(n, amp, band, rng)
    e1 = rng.uniform(-own, own, n) + 1j * rng.uniform(-own, own, n)
    e2 = rng.uniform(-own, own, n) + 1j * rng.uniform(-own, own, n)
    return ac._quantise(loc + e1), ac._quantise(gain * delayed(loc, delay) + e2)


def pair(nv, seed: int, delay: float = DELAY, noise: float = ac.NOISE, band: float = BAND):
    """The canceller's acceptance pair (anc_cases.pair: the same station, gains, own noise and generator order) with the
    common noise confined to `band` of the band and everything the sense antenna receives `delay` samples late."""
    s = ac.station(nv, seed)
    n = len(s)
    rng = np.random.default_rng(1000 + seed)
    loc = band_noise(n, noise, band, rng)
    e1 = rng.uniform(-ac.OWN, ac.OWN, n) + 1j * rng.uniform(-ac.OWN, ac.OWN, n)
    e2 = rng.uniform(-ac.OWN, ac.OWN, n) + 1j * rng.uniform(-ac.OWN, ac.OWN, n)
    return ac._quantise(s + loc + e1), ac._quantise(delayed(ac.STATION_GAIN * s + ac.NOISE_GAIN * loc, delay) + e2)


def carrier_pair(n: int, delay: int, seed: int):
    """Reason 3: what the rows share is a carrier; each row has noise of its own."""
    rng = np.random.default_rng(seed)
    c = 8000 * np.exp(2j * np.pi * 0.0731 * np.arange(n + delay))
    e1 = rng.uniform(-2000, 2000, n) + 1j * rng.uniform(-2000, 2000, n)
    e2 = rng.uniform(-2000, 2000, n) + 1j * rng.uniform(-2000, 2000, n)
    return ac._quantise(c[delay:] + e1), ac._quantise(0.7 * c[:n] + e2)


def random_rows(fmt: int, n: int, seed: int):
    """Full-scale random rows in format fmt (float32: the specials of the conversion among them)."""
    return ac.extremes(fmt, n, seed)[2]


def rails(n: int, value: int = -32768) -> np.ndarray:
    return np.full((n, 2), value, dtype=np.int16)


def alternating(n: int):
    """Full-scale input that drives the clamp.  The sense row's I follows the signs of the half-sample phase's taps, sixteen
    samples as they are and sixteen negated, so that once in thirty-two outputs all sixteen products add up (sum |h| * 32768:
    nearly twice full scale) and once they add up the other way; its Q and the main row alternate from sample to sample."""
    import align_ref
    a = np.full((n, 2), -32768, dtype=np.int16)
    a[1::2] = 32767
    b = a.copy()
    signs = np.sign(align_ref.taps()[16][::-1])                # sample m of a run meets tap 15 - m at the run's last output
    run = np.concatenate([signs, -signs])
    b[:, 0] = np.where(np.tile(run, n // 32 + 1)[:n] > 0, 32767, -32768)
    return a, b


def to_format(iq16: np.ndarray, fmt: int) -> np.ndarray:
    return rr.to_format(iq16, fmt, gain=3.0 if fmt in (rr.CU8, rr.CS8) else 1.0)
