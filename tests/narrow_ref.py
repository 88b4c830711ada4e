"""Restatement of the narrowband interpolator (include/navtex_amd_narrow.h), written from the header's contract, not from the
kernel: the rate's L / M, the conversions of both kinds, the polyphase sum in int64 numpy with the taps as an argument (and
one output at a time in Python integers, output_int, which the tests hold the numpy against), the count rule, the carried
state of a stream cut into calls anywhere, the design recipe in numpy, and the prototype's response."""
from __future__ import annotations

from fractions import Fraction
from math import ceil, pi

import numpy as np

import resample_ref as rr

OUTPUT_RATE, S = 252000, 14
S16, U8, S8, F32 = rr.CS16, rr.CU8, rr.CS8, rr.CF32
IQ, REAL = 0, 1
DTYPES = rr.DTYPES
PASS_HZ, PASS_FRACTION, STOP_DB, PASS_DB, DESIGN_DB = 25000, Fraction(2, 5), -76.0, 0.1, 90.0
MIN_RATE, MAX_RATE, MAX_PHASES, MAX_TAPS = 2000, 96000, 1024, 32768


def ratio(num: int, den: int = 1):
    """(L, M): 252000 den / num in lowest terms."""
    f = Fraction(OUTPUT_RATE * den, num)
    return f.numerator, f.denominator


def pass_edge(fi) -> float:
    return float(min(Fraction(PASS_HZ), PASS_FRACTION * Fraction(fi)))


def outputs_after(n: int, L: int, M: int) -> int:
    """ceil(n L / M): the outputs a stream has produced once it has consumed n samples."""
    return -((-n * L) // M)


def convert(samples: np.ndarray, fmt: int, kind: int) -> np.ndarray:
    """Samples in format fmt -> int64 [n, 2] in the int16 range: IQ from [n, 2], REAL from [n] with Q = 0."""
    if kind == IQ:
        return rr.convert(samples, fmt)
    a = np.asarray(samples).reshape(-1)
    c = rr.convert(np.stack([a, a], axis=1), fmt)
    c[:, 1] = 0
    return c


def pack(iq16: np.ndarray) -> np.ndarray:
    """int16 [n, 2] -> the uint32 words the kernel writes."""
    a = iq16.astype(np.int64)
    return ((a[:, 0] & 0xffff) | ((a[:, 1] & 0xffff) << 16)).astype(np.uint32)


def output_int(c, taps, L: int, M: int, n: int):
    """Output n of a stream whose converted samples since the reset are c[0 ...] ([k, 2]), in Python integers:
    ((I, Q), (acc_I, acc_Q))."""
    T = taps.shape[1]
    pos = n * M
    q, r = pos // L, pos % L
    assert q < len(c)
    accs, outs = [], []
    for comp in (0, 1):
        acc = sum(int(taps[r, t]) * (int(c[q - t, comp]) if q - t >= 0 else 0) for t in range(T))
        assert abs(acc) + (1 << (S - 1)) < 1 << 31
        accs.append(acc)
        outs.append(max(-32768, min(32767, (acc + (1 << (S - 1))) >> S)))
    return tuple(outs), tuple(accs)


class Interpolator:
    """One stream, fed in calls of any length (converted or raw samples)."""

    def __init__(self, taps: np.ndarray, L: int, M: int, fmt: int = S16, kind: int = IQ, position: int = 0):
        self.h, self.L, self.M, self.T = taps.astype(np.int64), L, M, taps.shape[1]
        assert taps.shape == (L, self.T)
        self.fmt, self.kind = fmt, kind
        self.reset(position)

    def reset(self, position: int = 0) -> None:
        """Input sample `position`, silence in front of it."""
        self.consumed = position
        self.hist = np.zeros((self.T - 1, 2), dtype=np.int64)
        self.acc_min = self.acc_max = 0

    @property
    def produced(self) -> int:
        return outputs_after(self.consumed, self.L, self.M)

    def push(self, x: np.ndarray) -> np.ndarray:
        """Any number of samples in the stream's format and kind -> int16 [outputs, 2]."""
        c = convert(x, self.fmt, self.kind)
        L, M, T = self.L, self.M, self.T
        ext = np.concatenate([self.hist, c])                                   # ext[k + T - 1] = sample consumed + k
        n0, n1 = self.produced, outputs_after(self.consumed + len(c), L, M)
        out = np.empty((n1 - n0, 2), dtype=np.int16)
        # pos = n M is taken relative to consumed L in Python integers (positions reach 2^62, and pos with them): with
        # e = n0 M - consumed L, output n0 + i has q - consumed = (e + i M) div L and r = (e + i M) mod L
        e = n0 * M - self.consumed * L
        assert 0 <= e < M
        for b in range(n0, n1, 1 << 20):
            rel = e + np.arange(b - n0, min(n1, b + (1 << 20)) - n0, dtype=np.int64) * M
            n = rel
            q, r = rel // L, rel % L
            acc = np.zeros((len(n), 2), dtype=np.int64)
            for t in range(T):
                acc += self.h[r, t][:, None] * ext[q - t + T - 1]
            assert np.abs(acc).max() + (1 << (S - 1)) < 2 ** 31, "the accumulator left int32"
            self.acc_min, self.acc_max = min(self.acc_min, int(acc.min())), max(self.acc_max, int(acc.max()))
            out[b - n0:b - n0 + len(n)] = np.clip((acc + (1 << (S - 1))) >> S, -32768, 32767).astype(np.int16)
        self.hist = ext[len(ext) - (T - 1):]
        self.consumed += len(c)
        return out


def interpolate_all(x: np.ndarray, taps: np.ndarray, L: int, M: int, fmt: int = S16, kind: int = IQ, position: int = 0):
    """One shot: (int16 [outputs, 2], the Interpolator behind it)."""
    ref = Interpolator(taps, L, M, fmt, kind, position)
    return ref.push(x), ref


# ---------------------------------------------------------------------------------------------------------------- design
def design(num: int, den: int = 1):
    """The header's recipe in numpy: (L, M, T, int16 taps [L, T])."""
    L, M = ratio(num, den)
    fi = num / den
    fp = pass_edge(Fraction(num, den))
    dw = 2 * pi * (fi - 2 * fp) / (L * fi)
    order = (DESIGN_DB - 7.95) / (2.285 * dw)
    T = int(ceil((order + 1) / L))
    T += T & 1
    T = max(T, 8)
    nt = L * T
    fc = 0.5 / L
    beta = 0.1102 * (DESIGN_DB - 8.7)
    centre = 0.5 * (nt - 1)
    d = np.arange(nt) - centre
    p = 2 * fc * np.sinc(2 * fc * d) * np.i0(beta * np.sqrt(1 - (d / (centre + 0.5)) ** 2)) / np.i0(beta)
    ph = p.reshape(T, L).T                                                     # [r, t] = p[r + t L]
    h = np.rint(ph / ph.sum(axis=1, keepdims=True) * (1 << S)).astype(np.int64)
    big = np.abs(h).argmax(axis=1)
    h[np.arange(L), big] += (1 << S) - h.sum(axis=1)
    assert np.abs(h).sum(axis=1).max() <= 65535 and np.abs(h).max() <= 32767
    return L, M, T, h.astype(np.int16)


def response_db(taps: np.ndarray, L: int, fi: float, freqs_hz: np.ndarray) -> np.ndarray:
    """|H(f)| / |H(0)| in dB of the prototype p[r + t L] = taps[r, t] at rate L fi."""
    return rr.response_db(taps, L, fi, freqs_hz)


def exact_counts(num: int, den: int, start: int, chunks) -> list:
    """The count rule in exact rational arithmetic: outputs per call of a stream that stands at `start` and is cut into
    `chunks`: every n with n / 252000 < seen / fi."""
    step = Fraction(num, den) / OUTPUT_RATE                                    # input samples per output
    def made(seen):
        total = int(Fraction(seen) / step)
        return total + 1 if Fraction(total) * step < seen else total
    out, seen = [], start
    for c in chunks:
        out.append(made(seen + c) - made(seen))
        seen += c
    return out
