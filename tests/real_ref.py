"""Restatement of the real-input converter (include/navtex_amd_real.h), written from the header's contract, not from the
kernel: the conversion (the resampler's, per component), the indexing of even and odd samples, the fourteen taps, the sum in
int64 numpy -- and one output at a time in Python integers (output_int), which the tests hold the numpy against -- the
carried state of a stream cut into calls anywhere, and the odd sample a push holds back."""
from __future__ import annotations

import numpy as np

import resample_ref as rr

K, S = 13, 14
TAPS = (10376, 3314, 1825, 1144, 745, 486, 310, 191, 111, 60, 30, 13, 4, 1)
HISTORY = 2 * K + 2
ACC_MAX = 18610 * 65535
S16, U8, S8, F32 = rr.CS16, rr.CU8, rr.CS8, rr.CF32
DTYPES = {S16: np.int16, U8: np.uint8, S8: np.int8, F32: np.float32}


def convert(x: np.ndarray, fmt: int) -> np.ndarray:
    """[n] real samples in format fmt -> int64 in the int16 range: the rule of a component of IQ."""
    a = np.asarray(x).reshape(-1)
    return rr.convert(np.repeat(a, 2), fmt)[:, 0]


def clamp16(v):
    return np.clip(v, -32768, 32767)


def output_int(c, m: int, invert: int = 0):
    """Output m of a stream whose converted samples since the reset are c[0 ...], in Python integers: (I, Q, acc)."""
    x = lambda k: int(c[k]) if 0 <= k < len(c) else 0      # noqa: E731
    e = lambda i: x(2 * i)                                  # noqa: E731
    o = lambda i: x(2 * i + 1)                              # noqa: E731
    assert 2 * m + 1 < len(c)
    s = 1 if (m - K) % 2 == 0 else -1
    acc = sum(TAPS[j] * (o(m - K - 1 - j) - o(m - K + j)) for j in range(K + 1))
    assert abs(acc) <= ACC_MAX < 1 << 31
    q = (acc + (1 << (S - 1))) >> S
    cl = lambda v: max(-32768, min(32767, v))               # noqa: E731
    return cl(s * e(m - K)), cl(-s * q if invert else s * q), acc


def pack(iq16: np.ndarray) -> np.ndarray:
    """int16 [n, 2] -> the uint32 words the kernel writes."""
    a = iq16.astype(np.int64)
    return ((a[:, 0] & 0xffff) | ((a[:, 1] & 0xffff) << 16)).astype(np.uint32)


class Converter:
    """One stream, fed in calls of any length."""

    def __init__(self, fmt: int = S16, invert: int = 0, position: int = 0):
        self.fmt, self.invert = fmt, invert
        self.reset(position)

    def reset(self, position: int = 0) -> None:
        """Sample `position` (even), silence in front of it, no sample held."""
        assert position % 2 == 0
        self.produced = position // 2
        self.e = np.zeros(HISTORY, dtype=np.int64)          # the last 28 pairs, oldest first
        self.o = np.zeros(HISTORY, dtype=np.int64)
        self.held = np.zeros(0, dtype=np.int64)             # the odd sample of a push, converted
        self.acc_min = self.acc_max = 0

    @property
    def consumed(self) -> int:
        return 2 * self.produced + len(self.held)

    def push(self, x: np.ndarray) -> np.ndarray:
        """Any number of samples -> int16 [outputs, 2]; an odd trailing sample waits for the next call."""
        c = np.concatenate([self.held, convert(x, self.fmt)])
        n = len(c) // 2
        self.held = c[2 * n:]
        if n == 0:
            return np.zeros((0, 2), dtype=np.int16)
        E = np.concatenate([self.e, c[0:2 * n:2]])           # pair i of the call at HISTORY + i
        O = np.concatenate([self.o, c[1:2 * n:2]])
        i = np.arange(n)
        acc = np.zeros(n, dtype=np.int64)
        for j in range(K + 1):                              # o[m-K-1-j] - o[m-K+j]
            acc += TAPS[j] * (O[HISTORY - K - 1 - j + i] - O[HISTORY - K + j + i])
        assert np.abs(acc).max() <= ACC_MAX
        self.acc_min, self.acc_max = min(self.acc_min, int(acc.min())), max(self.acc_max, int(acc.max()))
        q = (acc + (1 << (S - 1))) >> S
        s = np.where((self.produced + i - K) % 2 == 0, 1, -1)
        out = np.stack([clamp16(s * E[HISTORY - K + i]), clamp16(-s * q if self.invert else s * q)], axis=1).astype(np.int16)
        self.e, self.o = E[-HISTORY:], O[-HISTORY:]
        self.produced += n
        return out


def convert_all(x: np.ndarray, fmt: int = S16, invert: int = 0, position: int = 0):
    """One shot: (int16 [n // 2, 2], the Converter behind it)."""
    ref = Converter(fmt, invert, position)
    return ref.push(x), ref


def gain(f) -> np.ndarray:
    """G(f) = sum (-1)^j A[j] cos(2 pi f (2 j + 1)) / 2^(S-1): a real tone at fr/4 + f leaves as (1 + G) / 2 of a tone at +f and
    (1 - G) / 2 of one at -f (f in units of the input rate)."""
    f = np.asarray(f, dtype=np.float64)
    j = np.arange(K + 1)
    return (((-1.0) ** j * np.array(TAPS, dtype=np.float64))[None, :] * np.cos(2 * np.pi * f[:, None] * (2 * j[None, :] + 1))).sum(axis=1) / (1 << (S - 1))
