"""The IQ corrector's cases, shared by tests/test_iqc.py (CPU) and tests/test_gpu_iqc.py: two stations at mirrored
frequencies of one 252 kS/s stream -- 518 strong at +14 kHz, 490 weak under noise at -14 kHz -- the impairment of a zero-IF
radio (gain, phase, DC offset), and a noise-free tone on an FFT bin.  Nothing is kept: a row is 24 MB, and a test that wants
several at once holds them itself for as long as it runs."""
from __future__ import annotations

import numpy as np

import resample_ref as rr
import signals

SEEDS = tuple(range(11, 23))
RATE = 252000
TEXT_518, TEXT_490 = 3, 7
AMP_518, AMP_490, NOISE = 8000, 300, 1500
BIT_OFFSET_490 = 1234
GAIN, PHASE_DEG, DC_I, DC_Q = 1.05, 3.0, 300, -200
TONE_BIN, TONE_AMP = 3641, 8000


def texts():
    return signals.stream_text(TEXT_518), signals.stream_text(TEXT_490)


def rows(nv, seed: int, amp_490: float = AMP_490, noise: float = NOISE) -> np.ndarray:
    """The clean row as int16 [n, 2], n whole frames: the two stations and uniform noise."""
    bits = [nv.sitor_encode(t, 40) for t in texts()]
    n = (max(len(b) for b in bits) + 300) * 2520 // nv.FRAME_IN * nv.FRAME_IN
    a = rr.cpfsk(bits[0], RATE, n, freq_hz=14000, amplitude=AMP_518, noise_amp=0, seed=seed).astype(np.int32)
    a += rr.cpfsk(bits[1], RATE, n, freq_hz=-14000, amplitude=amp_490, noise_amp=noise, seed=seed, bit_offset=BIT_OFFSET_490)
    return np.clip(a, -32768, 32767).astype(np.int16)


def impair(x: np.ndarray) -> np.ndarray:
    """I' = I + 300, Q' = 1.05 (Q cos 3 deg + I sin 3 deg) - 200, rounded and clipped."""
    ph = np.deg2rad(PHASE_DEG)
    i, q = x[:, 0].astype(np.float64), x[:, 1].astype(np.float64)
    y = np.stack([i + DC_I, GAIN * (q * np.cos(ph) + i * np.sin(ph)) + DC_Q], axis=1)
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)


def tone(n: int) -> np.ndarray:
    """A noise-free tone on bin TONE_BIN of a 65 536-point FFT, as int16 [n, 2]."""
    ph = 2 * np.pi * ((TONE_BIN * np.arange(n, dtype=np.int64)) % 65536) / 65536.0
    return np.rint(TONE_AMP * np.stack([np.cos(ph), np.sin(ph)], axis=1)).astype(np.int16)


def image_dbc(block: np.ndarray) -> float:
    """The image of the tone in a block of 65 536 samples (Hann window), in dB against the tone."""
    z = (block[:, 0].astype(np.float64) + 1j * block[:, 1].astype(np.float64)) * np.hanning(65536)
    f = np.abs(np.fft.fft(z))
    peak = lambda k: f[[(k - 1) % 65536, k, (k + 1) % 65536]].max()      # noqa: E731
    return float(20 * np.log10(max(peak(65536 - TONE_BIN), 1e-9) / peak(TONE_BIN)))


def delivered(oracle, iq252: np.ndarray, frame_in: int):
    """({518: [texts], 490: [texts]} the oracle's two chains decode from a row at 252 kS/s, and (bits of 518, bits of 490)."""
    ref = oracle.Pipe(chain_mask=3)
    ref.push(iq252[:len(iq252) // frame_in * frame_in])
    return {f: [m[2] for m in ref.messages if m[0] == f] for f in (518, 490)}, (ref.bits(0), ref.bits(1))


# ------------------------------------------------------------------------------------------ rows for the restatement's edges
def impaired_noise(n: int, seed: int, amp: int = 6000) -> np.ndarray:
    """Uniform noise whose level changes every 50 000 samples, through impair(): every window solves to other coefficients."""
    rng = np.random.default_rng(seed)
    level = rng.uniform(0.3, 1.0, size=n // 50000 + 1)[np.arange(n) // 50000]
    x = rng.uniform(-amp, amp, size=(n, 2)) * level[:, None]
    return impair(np.rint(x).astype(np.int16))


def silence_with_dc(n: int) -> np.ndarray:
    """(300, -200) throughout: reason 1, with the offset removed all the same."""
    return np.tile(np.array([[DC_I, DC_Q]], dtype=np.int16), (n, 1))


def q_equals_i(n: int, seed: int) -> np.ndarray:
    """Q = I: the coherence is 1, reason 2."""
    i = np.random.default_rng(seed).integers(-5000, 5001, size=n).astype(np.int16)
    return np.stack([i, i], axis=1)


def q_three_i_rotated(n: int, seed: int) -> np.ndarray:
    """Q at three times the level of I and all but independent of it: step 7 passes (|a| is about 0.15), step 9 finds g near
    1/3: reason 4."""
    rng = np.random.default_rng(seed)
    i, j = rng.integers(-3000, 3001, size=n), rng.integers(-3000, 3001, size=n)
    return np.stack([i, np.rint(3 * (0.05 * i + j))], axis=1).astype(np.int16)


def rails(n: int, alternating: bool) -> np.ndarray:
    """Every sample at (-32768, -32768), or the rails alternating in sign: I every sample, Q every third."""
    x = np.full((n, 2), -32768, dtype=np.int16)
    if alternating:
        x[1::2, 0] = 32767
        x[(np.arange(n) // 3) % 2 == 1, 1] = 32767
    return x
