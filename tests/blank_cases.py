"""The blanker's acceptance case, shared by tests/test_blank.py (CPU) and tests/test_gpu_blank.py: a weak message at
+14 kHz under impulsive interference, at 252 kS/s (twelve seeds) and at 768 kS/s in front of the resampler (one seed).  Nothing
is kept: a row is 24 MB, and a test that wants the twelve at once holds them itself for as long as it runs."""
from __future__ import annotations

import numpy as np

import resample_ref as rr
import signals

SEEDS = tuple(range(11, 23))
TEXT_ID = 7
RATE = 252000
CHAIN_RATE, CHAIN_SEED, CHAIN_HOLD = 768000, 12, 96


def text() -> str:
    return signals.stream_text(TEXT_ID)


def bursts(n: int, rate: int, seed: int, shortest: int, longest: int) -> np.ndarray:
    """40 bursts a second of `shortest` .. `longest` samples of uniform +-30000, as float64 [n, 2] to add to a row."""
    rng = np.random.default_rng(1000 + seed)
    k = rng.poisson(40 * n / rate)
    z = np.zeros((n, 2))
    for s in rng.integers(0, n - shortest * 3, k):
        L = rng.integers(shortest, longest + 1)
        z[s:s + L] += rng.uniform(-30000, 30000, size=(L, 2))
    return z


def _add(x: np.ndarray, z: np.ndarray) -> np.ndarray:
    """clip(rint(x + z)) as int16, in z's own memory."""
    z += x
    np.rint(z, out=z)
    np.clip(z, -32768, 32767, out=z)
    return z.astype(np.int16)


def rows(nv_frame_in: int, bits: str, seed: int):
    """(clean x, with bursts y) as int16 [n, 2] at 252 kS/s, n whole frames."""
    n = (len(bits) + 300) * 2520 // nv_frame_in * nv_frame_in
    x = rr.cpfsk(bits, RATE, n, freq_hz=14000, amplitude=300, noise_amp=1500, seed=seed)
    y = _add(x, bursts(n, RATE, seed, 100, 300))
    return x, y


def chain_rows(bits: str, seed: int = CHAIN_SEED):
    """(clean, with bursts of 300 .. 900 samples) as int16 [n, 2] at 768 kS/s, n a whole number of 252 kS/s frames' worth."""
    per_frame = CHAIN_RATE * 8 // 25
    n = (len(bits) + 300) * (CHAIN_RATE // 100) // per_frame * per_frame
    x = rr.cpfsk(bits, CHAIN_RATE, n, freq_hz=14000, amplitude=300, noise_amp=1500, seed=seed)
    y = _add(x, bursts(n, CHAIN_RATE, seed, 300, 900))
    return x, y


def delivered(oracle, iq252: np.ndarray, frame_in: int):
    """The messages the oracle decodes from a row at 252 kS/s, and its bits."""
    ref = oracle.Pipe(chain_mask=1)
    ref.push(iq252[:len(iq252) // frame_in * frame_in])
    return [m[2] for m in ref.messages], ref.bits(0)
