"""The noise canceller's cases, shared by tests/test_anc.py (CPU) and tests/test_gpu_anc.py: a weak 490 station at -14 kHz of
a 252 kS/s row under local broadband noise that a sense antenna hears too (the acceptance case), the two pure-noise rows of
the null depth, the known limit (b) -- a strong station on both rows and nothing else --, and the rows for the
restatement's edges: rejection reasons, rails, full-scale random input in every format.  Nothing is kept: a row is 24 MB."""
from __future__ import annotations

import numpy as np

import anc_ref as ar
import resample_ref as rr
import signals

SEEDS = tuple(range(11, 23))
RATE = 252000
TEXT_490 = 7
AMP_490, NOISE, OWN = 300, 6000, 150
BIT_OFFSET_490 = 1234
STATION_GAIN = 0.3 * np.exp(0.7j)           # the station on the sense antenna against the main antenna
NOISE_GAIN = 0.8 * np.exp(2.1j)             # the local noise likewise
WEIGHT = (-5170, -8839)                     # rint(8192 / NOISE_GAIN): what cancels the noise exactly, in Q13
LIMIT_AMP, LIMIT_OWN, LIMIT_GAIN = 8000, 1500, 0.9 * np.exp(0.7j)
B = ar.BLOCK


def text():
    return signals.stream_text(TEXT_490)


def _quantise(z: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(np.stack([z.real, z.imag], axis=1)), -32768, 32767).astype(np.int16)


def station(nv, seed: int, amp: float = AMP_490) -> np.ndarray:
    """The 490 station alone as the main antenna receives it, complex [n], n whole frames."""
    bits = nv.sitor_encode(text(), 40)
    n = (len(bits) + 300) * 2520 // nv.FRAME_IN * nv.FRAME_IN
    s = rr.cpfsk(bits, RATE, n, freq_hz=-14000, amplitude=amp, noise_amp=0, seed=seed, bit_offset=BIT_OFFSET_490).astype(np.float64)
    return s[:, 0] + 1j * s[:, 1]


def pair(nv, seed: int, amp: float = AMP_490, noise: float = NOISE, own: float = OWN, station_gain: complex = STATION_GAIN):
    """(main, sense) as int16 [n, 2], n whole frames: main = s + L + e1, sense = station_gain s + NOISE_GAIN L + e2, with s the
    490 station, L the common noise (+-noise per component) and e1, e2 each receiver's own (+-own).  The generator draws the
    re and im of L, then of e1, then of e2."""
    s = station(nv, seed, amp)
    n = len(s)
    rng = np.random.default_rng(1000 + seed)
    loc = rng.uniform(-noise, noise, n) + 1j * rng.uniform(-noise, noise, n)
    e1 = rng.uniform(-own, own, n) + 1j * rng.uniform(-own, own, n)
    e2 = rng.uniform(-own, own, n) + 1j * rng.uniform(-own, own, n)
    return _quantise(s + loc + e1), _quantise(station_gain * s + NOISE_GAIN * loc + e2)


def limit_pair(nv, seed: int):
    """Known limit (b): the station at amplitude 8000 on both rows (sense gain 0.9 e^{j 0.7}), own noise +-1500, no common noise."""
    return pair(nv, seed, amp=LIMIT_AMP, noise=0, own=LIMIT_OWN, station_gain=LIMIT_GAIN)


def noise_pair(n: int, amp: float, seed: int = 5):
    """Pure common noise: main = L, sense = NOISE_GAIN L, no station and no own noise."""
    rng = np.random.default_rng(seed)
    loc = rng.uniform(-amp, amp, n) + 1j * rng.uniform(-amp, amp, n)
    return _quantise(loc), _quantise(NOISE_GAIN * loc)


def power_db(out: np.ndarray, against: np.ndarray) -> float:
    p = lambda x: float((x.astype(np.float64) ** 2).sum())      # noqa: E731
    return 10 * np.log10(max(p(out), 1e-9) / p(against))


def delivered(oracle, iq252: np.ndarray, frame_in: int):
    """(the texts the oracle's 490 chain decodes from a row at 252 kS/s, (bits of 518, bits of 490))."""
    ref = oracle.Pipe(chain_mask=3)
    ref.push(iq252[:len(iq252) // frame_in * frame_in])
    return [m[2] for m in ref.messages if m[0] == 490], (ref.bits(0), ref.bits(1))


# ------------------------------------------------------------------------------------------ rows for the restatement's edges
def drifting_pair(n: int, seed: int, amp: int = 6000):
    """Common noise whose path to the sense antenna changes every 50 000 samples (gain 0.5 .. 1.2, any phase), over own noise
    of +-200: every window solves to another weight, so a sample given the wrong block's weight shows in the output."""
    rng = np.random.default_rng(seed)
    k = n // 50000 + 1
    h = (rng.uniform(0.5, 1.2, size=k) * np.exp(1j * rng.uniform(0, 2 * np.pi, size=k)))[np.arange(n) // 50000]
    loc = rng.uniform(-amp, amp, n) + 1j * rng.uniform(-amp, amp, n)
    e1 = rng.uniform(-200, 200, n) + 1j * rng.uniform(-200, 200, n)
    e2 = rng.uniform(-200, 200, n) + 1j * rng.uniform(-200, 200, n)
    return _quantise(loc + e1), _quantise(h * loc + e2)


def formatted_pair(n: int, seed: int, fmt: int):
    """drifting_pair requantised to the format a radio of that kind delivers (three times the level for the 8-bit formats)."""
    a, b = drifting_pair(n, seed)
    gain = 3.0 if fmt in (rr.CU8, rr.CS8) else 1.0
    return rr.to_format(a, fmt, gain=gain), rr.to_format(b, fmt, gain=gain)


def rails(n: int) -> np.ndarray:
    return np.full((n, 2), -32768, dtype=np.int16)


def silent_sense(n: int):
    """Reason 1: the main row at the rails, the sense row all zero."""
    return rails(n), np.zeros((n, 2), dtype=np.int16)


def faint_sense(n: int):
    """Reason 2: the main row at the rails, the sense row (4, 4): TBB = 32 N passes step 1, tbb = 8 fails step 3."""
    return rails(n), np.full((n, 2), 4, dtype=np.int16)


def quarter_sense(n: int):
    """Reason 3: the sense row at a quarter of the main row wants the weight 4.0 = 32768 in Q13."""
    return rails(n), np.full((n, 2), -8192, dtype=np.int16)


def half_sense(n: int):
    """The sense row at half the main row: the weight 2.0 = (16384, 0), and nothing is left."""
    return rails(n), np.full((n, 2), -16384, dtype=np.int16)


def extremes(fmt: int, n: int, seed: int):
    """Three pairs in format fmt: both rows at the lowest value, the rails alternating in sign (differently in the two rows),
    and full-scale random input (float32: the specials of the conversion among it)."""
    dt = rr.DTYPES[fmt]
    rng = np.random.default_rng(seed)

    def random_row():
        if fmt != ar.CF32:
            return rng.integers(int(lo), int(hi) + 1, size=(n, 2)).astype(dt)
        rnd = rng.uniform(-1.3, 1.3, size=(n, 2)).astype(np.float32)
        special = np.array([np.nan, np.inf, -np.inf, 1e-42, -1e-42, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768,
                            32766.5 / 32768, 32767.5 / 32768, -32768.5 / 32768, 1.0, -1.0, 3e38, -3e38, 0.0, -0.0, 123.5 / 32768], dtype=np.float32)
        at = rng.integers(0, n, size=(400, 2))
        rnd[at[:, 0], at[:, 1] % 2] = special[rng.integers(0, len(special), size=400)]
        rnd[:len(special), 0] = special
        return rnd

    if fmt == ar.CF32:
        lo, hi = np.float32(-1.0), np.float32(32767.0 / 32768.0)
    else:
        lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
    low = np.full((n, 2), lo, dtype=dt)
    alt_a, alt_b = low.copy(), low.copy()
    alt_a[1::2, 0] = hi
    alt_a[(np.arange(n) // 3) % 2 == 1, 1] = hi
    alt_b[(np.arange(n) // 5) % 2 == 1, 0] = hi
    alt_b[2::3, 1] = hi
    return [(low, low.copy()), (alt_a, alt_b), (random_row(), random_row())]
