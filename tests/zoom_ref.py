"""Restatement of the zoom bank (include/navtex_amd_zoom.h), written from the header's contract, not from the kernel: the
conversion (the resampler's), the mixer (the bank's, ddc_ref.mix, with the table ddc_ref builds from decimals), k half-band
stages of the fourteen taps as a 55-tap low-pass in int64 numpy -- and one stage output at a time in Python integers
(stage_int), which the tests hold the numpy against --, the carried state of an input cut into calls anywhere, the retune
rule, the samples a push holds back, and the response computed from the taps."""
from __future__ import annotations

import numpy as np

import ddc_ref as dr
import resample_ref as rr

N, KZ_MIN, KZ_MAX = 4096, -2048, 2047
TAPS = (10376, 3314, 1825, 1144, 745, 486, 310, 191, 111, 60, 30, 13, 4, 1)
REACH, DELAY, SHIFT = 53, 26, 15
ABS_SUM = (1 << 14) + 2 * sum(TAPS)                          # 53604
ACC_MAX = ABS_SUM * 32768
CS16, CU8, CS8, CF32 = rr.CS16, rr.CU8, rr.CS8, rr.CF32
DTYPES = rr.DTYPES


def history(k: int) -> int:
    return REACH * ((1 << k) - 1)


def delay(k: int) -> int:
    return DELAY * ((1 << k) - 1)


def lowpass() -> np.ndarray:
    """h[0 .. 54] at scale 2^15: h[t] multiplies u[2m + 1 - t]; centre 2^14 at t = 27, odd taps (-1)^j A[j] at t = 27 +- (2j + 1)."""
    h = np.zeros(55, dtype=np.int64)
    h[27] = 1 << 14
    for j, a in enumerate(TAPS):
        h[27 - (2 * j + 1)] = h[27 + (2 * j + 1)] = (-1) ** j * a
    return h


def grid(rate_hz: float, hz: float):
    """kz = rint(hz N / rate), ties to even, in exact rationals; None where it leaves the range or hz is not finite."""
    from fractions import Fraction
    if not np.isfinite(hz) or not np.isfinite(rate_hz) or rate_hz <= 0:
        return None
    q = Fraction(hz) * N / Fraction(rate_hz)
    k = q.numerator // q.denominator
    r = q - k
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and k % 2):
        k += 1
    return k if KZ_MIN <= k <= KZ_MAX else None


def clamp16(v):
    return np.clip(v, -32768, 32767)


def stage_int(u, m: int):
    """Output m of a stage whose input since the reset is u[0 ...] (one component), in Python integers: (value, acc)."""
    x = lambda i: int(u[i]) if 0 <= i < len(u) else 0       # noqa: E731
    assert 2 * m + 1 < len(u)
    acc = (1 << 14) * x(2 * m - 26) + sum((-1) ** j * TAPS[j] * (x(2 * m - 27 - 2 * j) + x(2 * m - 25 + 2 * j)) for j in range(14))
    assert abs(acc) <= ACC_MAX and acc + (1 << 14) < 1 << 31
    return max(-32768, min(32767, (acc + (1 << 14)) >> SHIFT)), acc


def stage(front: np.ndarray, u: np.ndarray, track=None) -> np.ndarray:
    """One stage over a call: u [n, 2] (n even) behind `front` [53, 2], the stage's input in front of the call -> [n / 2, 2]."""
    assert len(front) == REACH and len(u) % 2 == 0
    a = np.concatenate([front, u])                           # sample i of the call at REACH + i
    n = len(u) // 2
    planes = (np.ascontiguousarray(a[0::2]), np.ascontiguousarray(a[1::2]))
    at = lambda c: planes[(REACH + c) % 2][(REACH + c) // 2:(REACH + c) // 2 + n]      # noqa: E731  a[REACH + 2 m + c] for m = 0 .. n - 1
    acc = at(-26) << 14
    for j, t in enumerate(TAPS):
        pair = at(-27 - 2 * j) + at(-25 + 2 * j)
        pair *= (-1) ** j * t
        acc += pair
    if n:
        assert np.abs(acc).max() <= ACC_MAX
        if track is not None:
            track[0], track[1] = min(track[0], int(acc.min())), max(track[1], int(acc.max()))
    return clamp16((acc + (1 << 14)) >> SHIFT)


def pack(iq16: np.ndarray) -> np.ndarray:
    """int16 [n, 2] -> the uint32 words the kernel writes."""
    a = iq16.astype(np.int64)
    return ((a[:, 0] & 0xffff) | ((a[:, 1] & 0xffff) << 16)).astype(np.uint32)


class Zoom:
    """One input with its zooms, fed in calls of any length."""

    def __init__(self, k: int, kzs=(0,), fmt: int = CS16, position: int = 0):
        assert 1 <= k <= 6 and 1 <= len(kzs) <= 8
        self.k, self.D, self.H, self.fmt = k, 1 << k, history(k), fmt
        self.kz = [int(v) for v in kzs]
        self.acc = [0, 0]                                   # the smallest and the largest stage sum seen
        self.reset(position)

    def reset(self, position: int = 0) -> None:
        """Sample `position` (a multiple of D), silence in front of it, no sample held; the shifts stay."""
        assert position % self.D == 0
        self.taken = position                               # samples the stages have seen
        self.hist = np.zeros((self.H, 2), dtype=np.int64)   # the last H converted, unmixed samples
        self.held = np.zeros((0, 2), dtype=np.int64)

    def set_shift(self, zoom: int, kz: int) -> None:
        assert KZ_MIN <= kz <= KZ_MAX
        self.kz[zoom] = int(kz)

    @property
    def consumed(self) -> int:
        return self.taken + len(self.held)

    @property
    def produced(self) -> int:
        return self.taken // self.D

    def push(self, samples: np.ndarray) -> np.ndarray:
        """Any number of samples -> int16 [zooms, outputs, 2]; up to D - 1 trailing samples wait for the next call."""
        c = np.concatenate([self.held, rr.convert(samples, self.fmt)])
        n = len(c) // self.D * self.D
        self.held = c[n:]
        out = np.zeros((len(self.kz), n // self.D, 2), dtype=np.int16)
        if n == 0:
            return out
        x = np.concatenate([self.hist, c[:n]])              # sample i of the call at H + i
        first = self.taken - self.H                         # its position: negative positions hold zeros, and zero mixes to zero
        for z, kz in enumerate(self.kz):
            u = dr.mix(x, kz, first % N) if kz else x       # only the position mod N enters the phase
            for s in range(1, self.k + 1):
                # the stage takes its own 53 off the front: what it leaves in front of the call is the next stage's history
                u = stage(u[:REACH], u[REACH:], self.acc)
            assert len(u) == n // self.D
            out[z] = u
        self.hist = x[-self.H:]
        self.taken += n
        return out


def zoom_all(samples: np.ndarray, k: int, kzs=(0,), fmt: int = CS16, position: int = 0):
    """One shot: (int16 [zooms, n // D, 2], the Zoom behind it)."""
    ref = Zoom(k, kzs, fmt, position)
    return ref.push(samples), ref


def naive(samples: np.ndarray, k: int, kz: int, fmt: int = CS16) -> np.ndarray:
    """The same shift, then every 2^k-th mixed sample with no filter: int16 [n // D, 2].  Everything D - 1 output bands away
    folds onto the row."""
    x = rr.convert(samples, fmt)
    return dr.mix(x, kz, 0)[:len(x) // (1 << k) * (1 << k):1 << k].astype(np.int16)


# ------------------------------------------------------------------------------------------------------------ the response
def stage_response(f) -> np.ndarray:
    """The stage's amplitude response at f cycles per sample of its input: the 55 taps are symmetric about t = 27."""
    f = np.asarray(f, dtype=np.float64)
    h = lowpass().astype(np.float64) / (1 << 15)
    t = np.arange(55) - 27
    return (h[None, :] * np.cos(2 * np.pi * f[:, None] * t[None, :])).sum(axis=1)


def response(k: int, f_in) -> np.ndarray:
    """The k stages' amplitude response at f_in cycles per input sample: stage s sees the frequency 2^(s-1) f_in."""
    f_in = np.asarray(f_in, dtype=np.float64)
    g = np.ones_like(f_in)
    for s in range(k):
        g = g * stage_response(f_in * (1 << s))
    return g


def ripple_and_folding_db(k: int, points: int = 2001):
    """(lowest and highest in-band gain in dB over |f| <= 0.4 of the output rate, the highest gain in dB of any input
    frequency that folds onto that band: f + a / D for a = 1 .. D - 1)."""
    D = 1 << k
    f = np.linspace(-0.4, 0.4, points) / D
    band = 20 * np.log10(np.abs(response(k, f)))
    fold = max(np.abs(response(k, f + a / D)).max() for a in range(1, D))
    return float(band.min()), float(band.max()), float(20 * np.log10(fold))
