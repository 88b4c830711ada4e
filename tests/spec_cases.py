"""The spectrum monitor's cases, shared by tests/test_spec.py (CPU) and tests/test_gpu_spec.py: busy rows in every format
(noise and turning carriers: a word from the wrong sample, bin or segment shows), tones on and between bins, the rails and
full-scale random input (the canceller's rows), and the notch's acceptance row, whose two carriers the finder is not told."""
from __future__ import annotations

import numpy as np

import notch_cases as nc
import spec_ref as sr

RATE = nc.RATE
SEEDS = nc.SEEDS
CARRIERS = nc.CARRIERS


def busy(n: int, seed: int, fmt: int = sr.CS16) -> np.ndarray:
    """Three carriers of 5000 .. 9000 over noise of +-2000, in format fmt (the notch's busy row)."""
    return nc.busy_row(n, seed, fmt)[0]


def tone(n: int, n_log2: int, bins: float, amp: float = 8000.0, noise: float = 0.0, seed: int = 1) -> np.ndarray:
    """int16 [n, 2]: a tone `bins` bins of 2^n_log2 above the centre (negative: below), over noise of +-noise."""
    z = nc.carrier(n, bins / (1 << n_log2), amp, rate=1.0)
    if noise:
        rng = np.random.default_rng(seed)
        z = z + rng.uniform(-noise, noise, n) + 1j * rng.uniform(-noise, noise, n)
    return nc._quantise(z)


def rails(fmt: int, n: int) -> np.ndarray:
    return nc.rails(fmt, n)


def full_scale(fmt: int, n: int, seed: int) -> np.ndarray:
    return nc.full_scale(fmt, n, seed)


def zeros(fmt: int, n: int) -> np.ndarray:
    """Silence in format fmt: what converts to (0, 0).  CU8 has no such value: its quietest input, 127.5 +- 0.5, is not silence,
    so the row is CS16-silent for the other three only."""
    assert fmt != sr.CU8
    return np.zeros((n, 2), dtype={sr.CS16: np.int16, sr.CS8: np.int8, sr.CF32: np.float32}[fmt])


def acceptance_row(nv, seed: int) -> np.ndarray:
    return nc.acceptance_row(nv, seed)


def hits_hz(hits):
    """The frequencies of the finder's hits, in hertz of the acceptance row."""
    return [h["cycles_per_sample"] * RATE for h in hits]
