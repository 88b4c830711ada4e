"""Restatement of the row aligner (include/navtex_amd_align.h), written from the header's contract, not from the kernels: the
conversion (the resampler's), the measurement in exact integers, the estimate in Python integers, the streaming filter in
numpy int64 and the carried samples of a pair cut into calls anywhere.  The taps are the shipped ones (nvx_align_taps needs
no device); tests/test_align.py holds them against the header's statements."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import resample_ref as rr

PHASES, T, G = 32, 16, 7
MAX_DELAY_DEFAULT, MIN_CONTRAST_DEFAULT, MAX_LAGS, MIN_WINDOW, COHERENCE_ONE = 4096, 64, 8192, 1024, 16384
CS16, CU8, CS8, CF32 = rr.CS16, rr.CU8, rr.CS8, rr.CF32
_TAPS = None


def taps() -> np.ndarray:
    """The shipped taps h_f[k] as int64 [32, 16]."""
    global _TAPS
    if _TAPS is None:
        lib = C.CDLL(str(Path(__file__).resolve().parent.parent / "navtex_amd" / "libnavtex_amd_align.so"))
        t = np.zeros((PHASES, T), dtype=np.int16)
        assert lib.nvx_align_taps(t.ctypes.data_as(C.c_void_p)) == 0
        _TAPS = t.astype(np.int64)
    return _TAPS


def pack(iq16: np.ndarray) -> np.ndarray:
    """int16 [n, 2] -> the uint32 words the kernel writes."""
    a = iq16.astype(np.int64)
    return ((a[:, 0] & 0xffff) | ((a[:, 1] & 0xffff) << 16)).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- measure
def window(n_in: int, lag_first: int, n_lags: int):
    """(n0, N), or None where the call is refused."""
    if n_lags < 64 or n_lags > MAX_LAGS or n_lags % 64:
        return None
    lag_last = lag_first + n_lags - 1
    n = n_in - (max(0, lag_last) - min(0, lag_first))
    if n < MIN_WINDOW:
        return None
    return max(0, -lag_first), n // 256 * 256


def measure(main: np.ndarray, sense: np.ndarray, fmt: int, lag_first: int, n_lags: int):
    """(R as int64 [n_lags, 2], SAA, SBB, N).  Every sum is a sum of integers below 2^53 in magnitude, so float64 dot products
    are exact in any order."""
    a, b = rr.convert(main, fmt) >> 4, rr.convert(sense, fmt) >> 4
    n0, n = window(len(a), lag_first, n_lags)
    assert n < 1 << 30
    ai, aq = a[n0:n0 + n, 0].astype(np.float64), a[n0:n0 + n, 1].astype(np.float64)
    bi, bq = b[:, 0].astype(np.float64), b[:, 1].astype(np.float64)
    r = np.zeros((n_lags, 2), dtype=np.int64)
    for k in range(n_lags):
        lo = n0 + lag_first + k
        si, sq = bi[lo:lo + n], bq[lo:lo + n]
        r[k, 0] = int(ai @ si + aq @ sq)
        r[k, 1] = int(aq @ si - ai @ sq)
    lo = n0 + lag_first
    saa = int((a[n0:n0 + n] ** 2).sum())
    sbb = int((b[lo:lo + n] ** 2).sum())
    return r, saa, sbb, n


# ------------------------------------------------------------------------------------------------------------------- find
def find(r, lag_first: int, n_window: int, saa: int, sbb: int, min_contrast: int = MIN_CONTRAST_DEFAULT) -> dict:
    """Steps 1 .. 6 in Python integers."""
    r = [(int(re), int(im)) for re, im in np.asarray(r).reshape(-1, 2)]
    n_lags = len(r)
    out = {"delay_q5": 0, "reason": 0, "coherence_q14": 0, "peak_lag": 0, "peak_power": 0, "median_power": 0}
    if saa < n_window or sbb < n_window:
        out["reason"] = 1
        return out
    s = max(0, max(max(abs(re), abs(im)) for re, im in r).bit_length() - 30)
    rs = [(re >> s, im >> s) for re, im in r]
    P = [re * re + im * im for re, im in rs]
    c = P.index(max(P))
    out["peak_lag"], out["peak_power"] = lag_first + c, P[c]
    if c < T // 2 + 2 or n_lags - 1 - c < T // 2 + 2:
        out["reason"] = 2
        return out
    out["median_power"] = sorted(P)[n_lags // 2]
    if P[c] < min_contrast * out["median_power"]:
        out["reason"] = 3
        return out
    h = taps()
    best = None
    for L in (c - 1, c, c + 1):
        for f in range(PHASES - 1, -1, -1):
            v_re = sum(int(h[f, k]) * rs[L + G - k][0] for k in range(T))
            v_im = sum(int(h[f, k]) * rs[L + G - k][1] for k in range(T))
            assert abs(v_re) < 1 << 45 and abs(v_im) < 1 << 45
            w = v_re * v_re + v_im * v_im
            if best is None or w > best[0]:
                best = (w, 32 * (lag_first + L) - f)
    out["delay_q5"] = best[1]
    den = (saa * sbb) >> (2 * s)
    if 0 < den < 1 << 112:
        out["coherence_q14"] = min(COHERENCE_ONE, best[0] // (den << 14))
    return out


# ------------------------------------------------------------------------------------------------------------------ apply
def split_delay(d: int):
    """(Dm, Ds, f) of delay_q5."""
    if d >= 0:
        dm = -(-d // 32)
        return dm, 0, 32 * dm - d
    return 0, (-d) >> 5, (-d) & 31


class Aligner:
    """One pair, fed in calls of any length."""

    def __init__(self, fmt: int = CS16, max_delay: int = MAX_DELAY_DEFAULT, delay_q5: int = 0):
        self.fmt, self.max_delay, self.H = fmt, max_delay, max_delay + T
        self.delay_q5 = 0
        self.set_delay(delay_q5)
        self.reset()

    def reset(self, position: int = 0) -> None:
        self.position = position
        self.hist_a = np.zeros((self.H, 2), dtype=np.int64)
        self.hist_b = np.zeros((self.H, 2), dtype=np.int64)

    def set_delay(self, delay_q5: int) -> None:
        assert abs(delay_q5) <= 32 * self.max_delay
        self.delay_q5 = delay_q5

    def push(self, main: np.ndarray, sense: np.ndarray):
        """-> (int16 [n, 2] of the main row, int16 [n, 2] of the sense row)."""
        a, b = rr.convert(main, self.fmt), rr.convert(sense, self.fmt)
        n = len(a)
        assert len(b) == n
        dm, ds, f = split_delay(self.delay_q5)
        xa, xb = np.concatenate([self.hist_a, a]), np.concatenate([self.hist_b, b])      # sample i of the call at H + i
        at = self.H + np.arange(n)
        out_a = xa[at - G - dm]
        h = taps()[f]
        acc = np.full((n, 2), 8192, dtype=np.int64)
        for k in range(T):
            acc += h[k] * xb[at - ds - k]
        assert n == 0 or np.abs(acc).max() < 1 << 31
        out_b = np.clip(acc >> 14, -32768, 32767)
        self.hist_a, self.hist_b = xa[len(xa) - self.H:], xb[len(xb) - self.H:]
        self.position += n
        return out_a.astype(np.int16), out_b.astype(np.int16)


def align(main: np.ndarray, sense: np.ndarray, delay_q5: int, fmt: int = CS16, max_delay: int = MAX_DELAY_DEFAULT):
    """One shot: (main out, sense out)."""
    return Aligner(fmt, max_delay, delay_q5).push(main, sense)
