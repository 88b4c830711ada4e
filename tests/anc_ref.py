"""Restatement of the antenna noise canceller (include/navtex_amd_anc.h), written from the header's contract, not from the
kernels: the conversion (the resampler's), the four block sums, the window, the six steps of the solve in Python integers,
the apply in numpy int64, and the carried state of a pair cut into calls anywhere."""
from __future__ import annotations

import numpy as np

import resample_ref as rr

BLOCK = 65536
WINDOW_LOG2_DEFAULT = 2
TRACK, HOLD = 0, 1
CS16, CU8, CS8, CF32 = rr.CS16, rr.CU8, rr.CS8, rr.CF32
C_ONE, C_MAX, COHERENCE_ONE = 8192, 32767, 16384


def solve(t, window_log2: int):
    """Steps 1 .. 6 on the window's sums (TAA, TBB, TRE, TIM): ((c_re, c_im), coherence, reason)."""
    TAA, TBB, TRE, TIM = (int(v) for v in t)
    N = 1 << (16 + window_log2)
    if TBB < 16 * N:
        return (0, 0), 0, 1
    s = max(0, max(TAA, TBB).bit_length() - 30)
    taa, tbb, tre, tim = TAA >> s, TBB >> s, TRE >> s, TIM >> s
    assert taa < 1 << 30 and tbb < 1 << 30 and abs(tre) <= 1 << 30 and abs(tim) <= 1 << 30
    if tbb < 1024:
        return (0, 0), 0, 2
    c_re = (tre * 16384 + tbb) // (2 * tbb)
    c_im = (tim * 16384 + tbb) // (2 * tbb)
    assert abs(tre * 16384 + tbb) < 1 << 45 and taa * tbb < 1 << 60 and tre * tre + tim * tim <= 1 << 61
    den = (taa * tbb) >> 14
    coherence = min(COHERENCE_ONE, (tre * tre + tim * tim) // den) if den > 0 else 0
    if max(abs(c_re), abs(c_im)) > C_MAX:
        return (0, 0), coherence, 3
    return (c_re, c_im), coherence, 0


def block_sums(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The four sums of converted samples (int64 [n, 2] each) as int64 [4]."""
    i1, q1, i2, q2 = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    return np.array([(i1 * i1 + q1 * q1).sum(), (i2 * i2 + q2 * q2).sum(), (i1 * i2 + q1 * q2).sum(), (q1 * i2 - i1 * q2).sum()], dtype=np.int64)


def apply(a: np.ndarray, b: np.ndarray, c) -> np.ndarray:
    """int64 [n, 2] converted samples of both rows -> int16 [n, 2]."""
    c_re, c_im = c
    p = c_re * b[:, 0] - c_im * b[:, 1] + 4096
    r = c_re * b[:, 1] + c_im * b[:, 0] + 4096
    assert len(a) == 0 or max(np.abs(p).max(), np.abs(r).max()) < 1 << 31
    return np.stack([np.clip(a[:, 0] - (p >> 13), -32768, 32767), np.clip(a[:, 1] - (r >> 13), -32768, 32767)], axis=1).astype(np.int16)


def pack(iq16: np.ndarray) -> np.ndarray:
    """int16 [n, 2] -> the uint32 words the kernel writes."""
    a = iq16.astype(np.int64)
    return ((a[:, 0] & 0xffff) | ((a[:, 1] & 0xffff) << 16)).astype(np.uint32)


class Canceller:
    """One pair, fed in calls of any length."""

    def __init__(self, fmt: int = CS16, window_log2: int = WINDOW_LOG2_DEFAULT, position: int = 0):
        assert window_log2 in (2, 4, 6)
        self.fmt, self.window_log2, self.W = fmt, window_log2, 1 << window_log2
        self.mode = TRACK
        self.samples = self.solved = self.rejected = 0
        self.reset(position)

    def reset(self, position: int = 0) -> None:
        """Position `position`, no block complete, the weight (0, 0); the mode and the counters stay."""
        self.position = position
        self.ring = np.zeros((self.W, 4), dtype=np.int64)      # block b in slot b mod W
        self.partial = np.zeros(4, dtype=np.int64)
        self.complete = 0
        self.c = (0, 0)
        self.coherence = 0
        self.reason = 0
        self.history = []                                      # (block, weight, coherence, reason) of every block start solved

    def set(self, c_re: int, c_im: int) -> None:
        assert abs(c_re) <= C_MAX and abs(c_im) <= C_MAX
        self.c = (c_re, c_im)

    def set_mode(self, mode: int) -> None:
        assert mode in (TRACK, HOLD)
        self.mode = mode

    def sums(self):
        """TAA, TBB, TRE, TIM over the complete blocks of the window, as Python integers."""
        return tuple(int(v) for v in self.ring.sum(axis=0))

    def push(self, main: np.ndarray, sense: np.ndarray) -> np.ndarray:
        a, b = rr.convert(main, self.fmt), rr.convert(sense, self.fmt)
        assert len(a) == len(b)
        out = np.empty((len(a), 2), dtype=np.int16)
        at = 0
        while at < len(a):
            if self.position % BLOCK == 0 and self.mode == TRACK and self.complete >= self.W:
                self.c, self.coherence, self.reason = solve(self.sums(), self.window_log2)
                self.solved += self.reason == 0
                self.rejected += self.reason != 0
                self.history.append((self.position // BLOCK, self.c, self.coherence, self.reason))
            n = min(len(a) - at, BLOCK - self.position % BLOCK)
            sa, sb = a[at:at + n], b[at:at + n]
            out[at:at + n] = apply(sa, sb, self.c)
            self.partial += block_sums(sa, sb)
            self.position += n
            at += n
            if self.position % BLOCK == 0:
                self.ring[(self.position // BLOCK - 1) % self.W] = self.partial
                self.partial = np.zeros(4, dtype=np.int64)
                self.complete = min(self.W, self.complete + 1)
        self.samples += len(a)
        return out


def cancel(main: np.ndarray, sense: np.ndarray, fmt: int = CS16, window_log2: int = WINDOW_LOG2_DEFAULT, position: int = 0):
    """One shot: (int16 [n, 2], the Canceller behind it)."""
    ref = Canceller(fmt, window_log2, position)
    return ref.push(main, sense), ref
