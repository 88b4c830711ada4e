"""Restatement of the impulse noise blanker (include/navtex_amd_blank.h), written from the header's contract, not from the
kernel: the resampler's input conversions (tests/resample_ref.py), magnitudes, block sums by absolute index, the level from
the minimum of the last four, detection, hold, and the counters -- in int64 numpy, with the carried state of the header so
that a stream can be cut into calls anywhere."""
from __future__ import annotations

import numpy as np

import resample_ref as rr

NB = 1024
THR_DEFAULT, HOLD_DEFAULT, FLOOR_DEFAULT = 1024, 32, 64
CS16, CU8, CS8, CF32 = rr.CS16, rr.CU8, rr.CS8, rr.CF32


def pack(x: np.ndarray) -> np.ndarray:
    """[n, 2] integers in the int16 range -> packed words, I in the low half."""
    x = np.asarray(x, dtype=np.int64)
    return ((x[:, 0] & 0xffff) | ((x[:, 1] & 0xffff) << 16)).astype(np.uint32)


def level_of(ref: int, thr_q8: int, floor: int) -> int:
    return max((thr_q8 * (ref >> 10)) >> 8, floor)


class Blanker:
    """One stream.  push() takes the next samples ([n, 2] in format fmt) and returns int16 [n, 2]; the counters and the
    per-sample detections and blanked flags of the last call are kept for the tests."""

    def __init__(self, fmt: int = CS16, thr_q8: int = THR_DEFAULT, hold: int = HOLD_DEFAULT, floor: int = FLOOR_DEFAULT, position: int = 0):
        assert thr_q8 == 0 or 256 <= thr_q8 <= 4096
        assert 0 <= hold <= 1024 and 0 <= floor <= 65535
        self.fmt, self.thr_q8, self.hold, self.floor = fmt, thr_q8, hold, floor
        self.samples = self.detections = self.blanked = 0
        self.reset(position)

    def reset(self, position: int = 0) -> None:
        """The stream stands at `position` with nothing in front of it: the block `position` lies in is the first."""
        self.position = position
        self.first_block = position // NB
        self.sums = []                       # of the complete blocks since the reset, the last four of them
        self.partial = 0                     # of the open block
        self.last = None                     # absolute index of the last detection

    def push(self, samples: np.ndarray) -> np.ndarray:
        x = rr.convert(samples, self.fmt)
        n = len(x)
        if n == 0:
            self.d = self.gone = np.zeros(0, dtype=bool)
            return np.zeros((0, 2), dtype=np.int16)
        m = np.abs(x[:, 0]) + np.abs(x[:, 1])
        idx = self.position + np.arange(n, dtype=np.int64)
        b = idx // NB
        b0, b1 = int(b[0]), int(b[-1])
        s = np.zeros(b1 - b0 + 1, dtype=np.int64)
        np.add.at(s, b - b0, m)
        s[0] += self.partial
        # S of the blocks in front of b0 (as far as they exist), then of b0 .. b1
        known = list(self.sums) + [int(v) for v in s]
        have = len(self.sums)                                # known[have + k] is block b0 + k
        level = np.full(b1 - b0 + 1, -1, dtype=np.int64)     # -1: nothing is detected in that block
        if self.thr_q8:
            for k in range(b1 - b0 + 1):
                if b0 + k - self.first_block >= 4:
                    assert have + k >= 4
                    level[k] = level_of(min(known[have + k - 4:have + k]), self.thr_q8, self.floor)
        lv = level[b - b0]
        d = (lv >= 0) & (m > lv)
        at = np.where(d, idx, np.int64(-1) << 40)
        at[0] = max(int(at[0]), self.last if self.last is not None else -(1 << 40))
        latest = np.maximum.accumulate(at)
        gone = idx - latest <= self.hold
        out = np.where(gone[:, None], 0, x).astype(np.int16)
        # the state behind the call
        end = self.position + n
        done = end // NB - b0                                # blocks of b0 .. b1 that are complete
        self.sums = (known[:have + done])[-4:]
        self.partial = int(s[done]) if done <= b1 - b0 else 0
        self.last = int(latest[-1]) if latest[-1] >= 0 else None
        self.position = end
        self.samples += n; self.detections += int(d.sum()); self.blanked += int(gone.sum())
        self.d, self.gone = d, gone
        return out


def blank(samples: np.ndarray, fmt: int = CS16, thr_q8: int = THR_DEFAULT, hold: int = HOLD_DEFAULT, floor: int = FLOOR_DEFAULT,
          position: int = 0):
    """A whole stream in one call: (int16 [n, 2], the Blanker behind it, for its counters and flags)."""
    b = Blanker(fmt, thr_q8, hold, floor, position)
    return b.push(samples), b
