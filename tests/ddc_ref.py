"""Restatement of the down-converter bank (include/navtex_amd_ddc.h), written from the header's contract, not from the
kernel: the grid rule in exact rational arithmetic, the table from `decimal`, the mixer in int64 numpy with every 32-bit sum
checked, and the resampler's restatement (tests/resample_ref.py) behind it, with the unmixed history carried per input."""
from __future__ import annotations

import functools
from decimal import ROUND_HALF_EVEN, Decimal, getcontext
from fractions import Fraction

import numpy as np

from resample_ref import convert, resample, resample_streams

N, SCALE, GUARD_HZ = 4096, 32767, 25000


def grid(fi: int, hz) -> int | None:
    """k = rint(hz N / fi), ties to even, over the rationals; None outside |k fi / N| <= fi / 2 - 25000."""
    k = round(Fraction(hz) * N / fi)                                         # Fraction.__round__: ties to even
    return k if abs(Fraction(k * fi, N)) <= Fraction(fi, 2) - GUARD_HZ else None


def k_range(fi: int) -> int:
    """The largest allowed |k|."""
    return (N * (fi - 2 * GUARD_HZ)) // (2 * fi)


def _pi() -> Decimal:
    def arctan_inv(x: int) -> Decimal:
        total = term = Decimal(1) / x
        k = 1
        while True:
            term /= -x * x
            nxt = total + term / (2 * k + 1)
            if nxt == total:
                return total
            total, k = nxt, k + 1
    return 4 * (4 * arctan_inv(5) - arctan_inv(239))


def _cos_sin(x: Decimal):
    c, s, term, k = Decimal(1), Decimal(0), Decimal(1), 0
    while True:
        k += 1
        term = term * x / k
        if abs(term) < Decimal(10) ** -55:
            return c, s
        if k % 2:
            s += term if k % 4 == 1 else -term
        else:
            c += term if k % 4 == 0 else -term


@functools.lru_cache(maxsize=None)
def _table_tuple():
    getcontext().prec = 70
    step = 2 * _pi() / N
    out = []
    for j in range(N):
        c, s = _cos_sin(step * j)                                            # the whole turn from the series: no symmetry is assumed
        out.append((int((SCALE * c).to_integral_value(rounding=ROUND_HALF_EVEN)), int((SCALE * s).to_integral_value(rounding=ROUND_HALF_EVEN))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _table_array() -> np.ndarray:
    w = np.array(_table_tuple(), dtype=np.int64)
    w.setflags(write=False)
    return w


def table() -> np.ndarray:
    """W [N, 2] int64: (rint(32767 cos(2 pi j / N)), rint(32767 sin(2 pi j / N)))."""
    return _table_array().copy()


def mix(x: np.ndarray, k: int, n_first: int) -> np.ndarray:
    """x [n, 2] int64 (converted), the samples n_first, n_first + 1, ... of the input -> x' (k = 0: x itself)."""
    x = np.asarray(x, dtype=np.int64).reshape(-1, 2)
    if k == 0 or len(x) == 0:
        return x.copy()
    w = _table_array()
    assert 0 <= n_first < 1 << 50 and abs(k) <= N                            # k n stays inside int64
    j = (k * (n_first + np.arange(len(x), dtype=np.int64))) % N              # floor modulo: 0 .. N-1 for negative k too
    c, s = w[j, 0], w[j, 1]
    si = x[:, 0] * c + x[:, 1] * s + (1 << 14)
    sq = x[:, 1] * c - x[:, 0] * s + (1 << 14)
    assert max(np.abs(si).max(), np.abs(sq).max()) < 2 ** 31, "a mixer sum left int32"
    return np.clip(np.stack([si >> 15, sq >> 15], axis=1), -32768, 32767)


def ddc(x: np.ndarray, taps: np.ndarray, L: int, M: int, k: int, consumed: int = 0, history: np.ndarray | None = None):
    """One slice over one call: x [n, 2] int64 (converted, unmixed) are the input's samples consumed, consumed + 1, ...;
    history the unmixed samples in front (the last len(history) of them; silence before).  The history is mixed with its
    true index and the current k.  Returns (int16 [n_out, 2], the new unmixed history of T-1 samples)."""
    x = np.asarray(x, dtype=np.int64).reshape(-1, 2)
    T = taps.shape[1]
    hist = np.zeros((T - 1, 2), dtype=np.int64)
    if history is not None and len(history):
        hv = np.asarray(history, dtype=np.int64).reshape(-1, 2)[-(T - 1):]
        hist[T - 1 - len(hv):] = hv
    first = max(consumed - (T - 1), 0)                                       # samples before the reset are silence: zeros stay zeros
    hm = hist.copy()
    hm[T - 1 - (consumed - first):] = mix(hist[T - 1 - (consumed - first):], k, first)
    out, _ = resample(mix(x, k, consumed), taps, L, M, consumed, hm)
    return out, np.concatenate([hist, x])[-(T - 1):]


def ddc_slices(x: np.ndarray, taps: np.ndarray, L: int, M: int, ks, block: int = 256) -> np.ndarray:
    """Every slice of one input from its reset, `block` slices at a time: the slices' mixed samples side by side through
    resample_streams (one matrix product per 256 outputs, exact in float64).  x [n, 2] int64 (converted) -> int16
    [len(ks), n_out, 2]; the words are ddc()'s (tests/test_ddc.py holds the two against each other)."""
    x = np.asarray(x, dtype=np.int64).reshape(-1, 2)
    ks = [int(k) for k in ks]
    parts = [resample_streams(np.stack([mix(x, k, 0) for k in ks[b:b + block]]), taps, L, M, out_block=256) for b in range(0, len(ks), block)]
    return np.concatenate(parts)


def ddc_all(samples: np.ndarray, fmt: int, taps: np.ndarray, L: int, M: int, k: int, consumed: int = 0) -> np.ndarray:
    """A slice of an input that stands at `consumed` with silence in front."""
    return ddc(convert(samples, fmt), taps, L, M, k, consumed)[0]
