"""Restatement of the tone notch (include/navtex_amd_notch.h), written from the header's contract, not from the kernels: the
conversion (the resampler's), the NCO on the bank's table (tests/ddc_ref.py builds it from series, not from the header), the
block sums, the smoothing, the interpolation, the amplitude, the mix up and the offset readout in numpy int64 with every bound
of the header asserted, and the carried state of a row cut into calls anywhere."""
from __future__ import annotations

import math

import numpy as np

import ddc_ref
import resample_ref as rr

BLOCK = 256
MAX_NOTCHES = 4
WIDTH_LOG2_DEFAULT = 5
MAX_PAIRS = 4096
CS16, CU8, CS8, CF32 = rr.CS16, rr.CU8, rr.CS8, rr.CF32
M32 = (1 << 32) - 1


def step_from_hz(hz: float, rate: float) -> int:
    turns = hz / rate
    return int(np.rint((turns - math.floor(turns)) * 4294967296.0)) & M32


def hz_from_step(step: int, rate: float) -> float:
    return (step - (1 << 32) if step >= 1 << 31 else step) * rate / 4294967296.0


def nco(step: int, first: int, n: int):
    """(c, s) of samples first .. first + n - 1 as int64 arrays."""
    w = ddc_ref.table()
    idx = (np.uint64(first & M32) + np.arange(n, dtype=np.uint64)) & np.uint64(M32)        # below 2^32: the product stays inside 64 bits
    ph = (np.uint64(step) * idx) & np.uint64(M32)
    j = (ph >> np.uint64(20)).astype(np.int64)
    return w[j, 0], w[j, 1]


def pack(iq16: np.ndarray) -> np.ndarray:
    """int16 [n, 2] -> the uint32 words the kernel writes."""
    a = iq16.astype(np.int64)
    return ((a[:, 0] & 0xffff) | ((a[:, 1] & 0xffff) << 16)).astype(np.uint32)


class _Tone:
    """One notch of a row: its step and flag, and what it carries."""

    def __init__(self, hist: int):
        self.step, self.enabled = 0, False
        self.hist = hist
        self.restart(0)

    def restart(self, position: int) -> None:
        self.sums = np.zeros((self.hist, 2), dtype=np.int64)       # the last `hist` complete blocks, oldest first
        self.partial = np.zeros(2, dtype=np.int64)
        self.measure(position)

    def measure(self, position: int) -> None:
        self.x = [0, 0]
        self.pairs = 0
        self.first = -(-position // BLOCK)                         # the first block wholly behind the restart


class Notch:
    """One row, fed in calls of any length."""

    def __init__(self, fmt: int = CS16, n_notches: int = 1, width_log2: int = WIDTH_LOG2_DEFAULT, position: int = 0):
        assert 1 <= n_notches <= MAX_NOTCHES and 2 <= width_log2 <= 6
        self.fmt, self.r, self.R = fmt, width_log2, 1 << width_log2
        self.D = (self.R + 1) * BLOCK
        self.H = 2 * self.R + 2
        self.tones = [_Tone(self.H) for _ in range(n_notches)]
        self.tri = np.array([self.R - abs(k) for k in range(-(self.R - 1), self.R)], dtype=np.int64)
        self.samples = 0
        self.reset(position)

    def delay(self) -> int:
        return self.D

    def reset(self, position: int = 0) -> None:
        """Position `position`, nothing in front; the steps, the flags and the sample counter stay."""
        self.position = self.start = position
        self.line = np.zeros((self.D, 2), dtype=np.int64)
        for t in self.tones:
            t.restart(position)

    def set_freq(self, notch: int, step: int) -> None:
        self.tones[notch].step = step & M32
        self.tones[notch].restart(self.position)

    def enable(self, notch: int, enable: bool = True) -> None:
        self.tones[notch].enabled = bool(enable)

    def measure(self, notch: int) -> None:
        self.tones[notch].measure(self.position)

    def refine(self, notch: int) -> int:
        t = self.tones[notch]
        if t.x != [0, 0]:
            arg = math.atan2(float(t.x[1]), float(t.x[0]))
            self.set_freq(notch, t.step + int(np.rint(arg * 4294967296.0 / (2.0 * math.pi * BLOCK))))
        return t.step

    def offset_hz(self, notch: int, rate: float) -> float:
        t = self.tones[notch]
        return math.atan2(float(t.x[1]), float(t.x[0])) * rate / (2 * math.pi * BLOCK)

    def get(self, notch: int = 0) -> dict:
        t = self.tones[notch]
        return {"x": (int(t.x[0]), int(t.x[1])), "pairs": t.pairs, "step": t.step, "enabled": t.enabled, "samples": self.samples}

    def push(self, samples: np.ndarray) -> np.ndarray:
        x = rr.convert(samples, self.fmt)
        n = len(x)
        if n == 0:
            return np.empty((0, 2), dtype=np.int16)
        P, D, R, r, H = self.position, self.D, self.R, self.r, self.H
        off0 = P % BLOCK
        blocks = (off0 + n - 1) // BLOCK + 1
        done = (off0 + n) // BLOCK
        b0 = P // BLOCK
        i = np.arange(n, dtype=np.int64)
        both = np.concatenate([self.line, x])                      # word i of the call subtracts from both[i] = x[P + i - D]
        # word i interpolates at g = (P + i - D) - 128, in blocks counted from the call's first
        g = off0 - D - BLOCK // 2 + i
        lo, f = g >> 8, g & 255
        E = np.zeros((n, 2), dtype=np.int64)
        bounds = np.concatenate([[0], np.arange(1, blocks, dtype=np.int64) * BLOCK - off0])
        for t in self.tones:
            c, s = nco(t.step, P, n)
            u = np.stack([x[:, 0] * c + x[:, 1] * s, x[:, 1] * c - x[:, 0] * s], axis=1)
            assert np.abs(u).max() < 1 << 31
            rec = np.add.reduceat(u, bounds, axis=0)
            rec[0] += t.partial
            B = np.concatenate([t.sums, rec])                      # B[H + j] is block j of the call
            assert np.abs(B).max() <= 1 << 39
            # M of block j (from the call's first) = sum_k tri[k] B[H + j + k - (R - 1)]: `valid` convolution, M[j] at j + H - (R - 1)
            Bz = np.concatenate([B, np.zeros((2 * R, 2), dtype=np.int64)])
            M = np.stack([np.convolve(Bz[:, k], self.tri, mode="valid") for k in range(2)], axis=1)
            assert np.abs(M).max() <= 1 << (39 + 2 * r)
            at = lambda j: j + H - (R - 1)                         # noqa: E731
            # the offset readout, as the call's blocks end
            first = max(0, t.first - b0 + 2 * R - 1)
            for cb in range(first, done):
                if t.pairs >= MAX_PAIRS:
                    break
                b = cb - (R - 1)
                cur = [int(v) >> (2 * r + 15) for v in M[at(b)]]
                prev = [int(v) >> (2 * r + 15) for v in M[at(b - 1)]]
                assert max(abs(v) for v in cur + prev) <= 1 << 24
                t.x[0] += cur[0] * prev[0] + cur[1] * prev[1]
                t.x[1] += cur[1] * prev[0] - cur[0] * prev[1]
                assert abs(t.x[0]) < 1 << 63 and abs(t.x[1]) < 1 << 63
                t.pairs += 1
            if t.enabled:
                assert lo.min() + at(0) >= 0 and lo.max() + 1 + at(0) < len(M)
                m = M[lo + at(0)] * (256 - f)[:, None] + M[lo + 1 + at(0)] * f[:, None]
                assert np.abs(m).max() <= 1 << (47 + 2 * r)
                sh = 27 + 2 * r
                a = (m + (1 << (sh - 1))) >> sh
                assert np.abs(a).max() <= 1 << 20
                co, so = nco(t.step, P - D, n)
                e = np.stack([a[:, 0] * co - a[:, 1] * so, a[:, 0] * so + a[:, 1] * co], axis=1)
                assert np.abs(e).max() <= 1 << 36
                E += (e + (1 << 18)) >> 19
            # what the notch carries on
            t.sums = B[done:done + H].copy()
            t.partial = B[H + done].copy() if (off0 + n) % BLOCK else np.zeros(2, dtype=np.int64)
        y = np.clip(both[:n] - E, -32768, 32767)
        y[P + i - D < self.start] = 0
        self.line = both[n:].copy()
        self.position += n
        self.samples += n
        return y.astype(np.int16)


def notch(samples: np.ndarray, steps, fmt: int = CS16, width_log2: int = WIDTH_LOG2_DEFAULT, position: int = 0):
    """One shot with len(steps) notches, enabled where the step is not None: (int16 [n, 2], the Notch behind it)."""
    ref = Notch(fmt, len(steps), width_log2, position)
    for k, step in enumerate(steps):
        if step is not None:
            ref.set_freq(k, step)
            ref.enable(k)
    return ref.push(samples), ref
