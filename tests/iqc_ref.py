"""Restatement of the IQ corrector (include/navtex_amd_iqc.h), written from the header's contract, not from the kernels:
the conversion (the resampler's), the five block sums, the window, the ten steps of the solve in Python integers, the
apply, and the carried state of a stream cut into calls anywhere."""
from __future__ import annotations

from math import isqrt

import numpy as np

import resample_ref as rr

BLOCK = 65536
WINDOW_LOG2_DEFAULT = 4
TRACK, HOLD = 0, 1
CS16, CU8, CS8, CF32 = rr.CS16, rr.CU8, rr.CS8, rr.CF32
IDENTITY = (0, 0, 0, 16384)
CQ_MIN, CQ_MAX, CI_MAX = 12288, 21845, 5462


def solve(t, window_log2: int):
    """Steps 1 .. 10 on the window's sums (TI, TQ, TII, TQQ, TIQ): ((dI, dQ, c_i, c_q), reason)."""
    TI, TQ, TII, TQQ, TIQ = (int(v) for v in t)
    ln = 16 + window_log2
    N = 1 << ln
    dI, dQ = (TI + N // 2) >> ln, (TQ + N // 2) >> ln
    CII = TII - 2 * dI * TI + N * dI * dI
    CQQ = TQQ - 2 * dQ * TQ + N * dQ * dQ
    CIQ = TIQ - dI * TQ - dQ * TI + N * dI * dQ
    assert all(abs(v) < 1 << 63 for v in (2 * dI * TI, N * dI * dI, N * dI * dQ, CII, CQQ, CIQ))
    if CII < 16 * N or CQQ < 16 * N:
        return (dI, dQ, 0, 16384), 1
    s = max(0, max(CII, CQQ).bit_length() - 30)
    cii, cqq, ciq = CII >> s, CQQ >> s, CIQ >> s
    a = (-ciq * 32768 + cii) // (2 * cii)
    if abs(a) > 4096:
        return (dI, dQ, 0, 16384), 2
    v = cqq + ((2 * a * ciq) >> 14) + ((a * a * cii) >> 28)
    if v <= 0:
        return (dI, dQ, 0, 16384), 3
    g = isqrt((cii << 28) // v)
    if g < CQ_MIN or g > CQ_MAX:
        return (dI, dQ, 0, 16384), 4
    return (dI, dQ, (a * g + 8192) >> 14, g), 0


def block_sums(c: np.ndarray) -> np.ndarray:
    """The five sums of converted samples (int64 [n, 2]) as int64 [5]."""
    i, q = c[:, 0], c[:, 1]
    return np.array([i.sum(), q.sum(), (i * i).sum(), (q * q).sum(), (i * q).sum()], dtype=np.int64)


def apply(c: np.ndarray, coef) -> np.ndarray:
    """int64 [n, 2] converted samples -> int16 [n, 2]."""
    dI, dQ, c_i, c_q = coef
    i, q = c[:, 0] - dI, c[:, 1] - dQ
    acc = c_q * q + c_i * i + 8192
    assert len(c) == 0 or np.abs(acc).max() < 1 << 31
    return np.stack([np.clip(i, -32768, 32767), np.clip(acc >> 14, -32768, 32767)], axis=1).astype(np.int16)


def pack(iq16: np.ndarray) -> np.ndarray:
    """int16 [n, 2] -> the uint32 words the kernel writes."""
    a = iq16.astype(np.int64)
    return ((a[:, 0] & 0xffff) | ((a[:, 1] & 0xffff) << 16)).astype(np.uint32)


class Corrector:
    """One stream, fed in calls of any length."""

    def __init__(self, fmt: int = CS16, window_log2: int = WINDOW_LOG2_DEFAULT, position: int = 0):
        assert window_log2 in (2, 4, 6)
        self.fmt, self.window_log2, self.W = fmt, window_log2, 1 << window_log2
        self.mode = TRACK
        self.samples = self.solved = self.rejected = 0
        self.reset(position)

    def reset(self, position: int = 0) -> None:
        """Position `position`, no block complete, the identity; the mode and the counters stay."""
        self.position = position
        self.ring = np.zeros((self.W, 5), dtype=np.int64)      # block b in slot b mod W
        self.partial = np.zeros(5, dtype=np.int64)
        self.complete = 0
        self.coef = IDENTITY
        self.reason = 0
        self.history = []                                      # (block, coefficients, reason) of every block start solved

    def set(self, dI: int, dQ: int, c_i: int, c_q: int) -> None:
        assert -32768 <= dI <= 32767 and -32768 <= dQ <= 32767 and abs(c_i) <= CI_MAX and CQ_MIN <= c_q <= CQ_MAX
        self.coef = (dI, dQ, c_i, c_q)

    def set_mode(self, mode: int) -> None:
        assert mode in (TRACK, HOLD)
        self.mode = mode

    def sums(self):
        """TI, TQ, TII, TQQ, TIQ over the complete blocks of the window, as Python integers."""
        return tuple(int(v) for v in self.ring.sum(axis=0))

    def push(self, x: np.ndarray) -> np.ndarray:
        c = rr.convert(x, self.fmt)
        out = np.empty((len(c), 2), dtype=np.int16)
        at = 0
        while at < len(c):
            if self.position % BLOCK == 0 and self.mode == TRACK and self.complete >= self.W:
                self.coef, self.reason = solve(self.sums(), self.window_log2)
                self.solved += self.reason == 0
                self.rejected += self.reason != 0
                self.history.append((self.position // BLOCK, self.coef, self.reason))
            n = min(len(c) - at, BLOCK - self.position % BLOCK)
            seg = c[at:at + n]
            out[at:at + n] = apply(seg, self.coef)
            self.partial += block_sums(seg)
            self.position += n
            at += n
            if self.position % BLOCK == 0:
                self.ring[(self.position // BLOCK - 1) % self.W] = self.partial
                self.partial = np.zeros(5, dtype=np.int64)
                self.complete = min(self.W, self.complete + 1)
        self.samples += len(c)
        return out


def correct(x: np.ndarray, fmt: int = CS16, window_log2: int = WINDOW_LOG2_DEFAULT, position: int = 0):
    """One shot: (int16 [n, 2], the Corrector behind it)."""
    ref = Corrector(fmt, window_log2, position)
    return ref.push(x), ref
