"""Restatement of the diversity combiner (include/navtex_amd_div.h), written from the header's contract, not from the
kernels: the conversion (the resampler's), the NCO on the bank's table (tests/ddc_ref.py builds it from series, not from the
header), the block sums, the cells, the window, the solve in Python integers, the apply in numpy int64 with every bound of
the header asserted, and the carried state of a pair cut into calls anywhere."""
from __future__ import annotations

import math

import numpy as np

import ddc_ref
import resample_ref as rr

BLOCK, CELL = 256, 65536
MAX_TARGETS = 4
WINDOW_LOG2_DEFAULT = 2
TRACK, HOLD = 0, 1
CS16, CU8, CS8, CF32 = rr.CS16, rr.CU8, rr.CS8, rr.CF32
W_ONE, W_MAX, COHERENCE_ONE = 8192, 32767, 16384
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


def mix(x: np.ndarray, c: np.ndarray, s: np.ndarray) -> np.ndarray:
    """Step 2: converted samples int64 [n, 2] -> u as int64 [n, 2]."""
    u = np.stack([x[:, 0] * c + x[:, 1] * s, x[:, 1] * c - x[:, 0] * s], axis=1)
    assert len(u) == 0 or np.abs(u).max() < 1 << 31
    return u


def solve(t):
    """Step 6 on the window's sums (TAA, TBB, TRE, TIM): (lead, (w_re, w_im), coherence, reason)."""
    TAA, TBB, TRE, TIM = (int(v) for v in t)
    if TAA + TBB < 1024:
        return 0, (0, 0), 0, 1
    sh = max(0, max(TAA, TBB).bit_length() - 29)
    taa, tbb, tre, tim = TAA >> sh, TBB >> sh, TRE >> sh, TIM >> sh
    assert taa < 1 << 29 and tbb < 1 << 29 and abs(tre) <= 1 << 29 and abs(tim) <= 1 << 29      # |sum A' conj B'| <= max(TAA, TBB)
    d = taa - tbb
    q = d * d + 4 * (tre * tre + tim * tim)
    assert q < 1 << 62
    r = math.isqrt(q)
    den = r + abs(d)
    if den == 0:
        return 0, (0, 0), 0, 0
    lead = 0 if d >= 0 else 1
    clamp = lambda v: max(-W_ONE, min(W_ONE, v))          # noqa: E731
    w_re = clamp((tre * 32768 + den) // (2 * den))
    w_im = clamp(((tim if lead == 0 else -tim) * 32768 + den) // (2 * den))
    m = (taa * tbb) >> 14
    coherence = min(COHERENCE_ONE, (tre * tre + tim * tim) // m) if m > 0 else 0
    return lead, (w_re, w_im), coherence, 0


def solve_line(t) -> str:
    """What tests/harness/div_solve.cpp prints for one row of sums."""
    lead, (w_re, w_im), coherence, reason = solve(t)
    return f"{lead} {w_re} {w_im} {coherence} {reason}"


def apply(a: np.ndarray, b: np.ndarray, lead: int, w) -> np.ndarray:
    """Step 7: int64 [n, 2] converted samples of both rows -> int16 [n, 2]."""
    w_re, w_im = w
    strong, weak = (b, a) if lead else (a, b)
    p = w_re * weak[:, 0] - w_im * weak[:, 1] + 4096
    r = w_re * weak[:, 1] + w_im * weak[:, 0] + 4096
    assert len(a) == 0 or max(np.abs(p).max(), np.abs(r).max()) < 1 << 31
    return np.stack([np.clip(strong[:, 0] + (p >> 13), -32768, 32767), np.clip(strong[:, 1] + (r >> 13), -32768, 32767)], axis=1).astype(np.int16)


def pack(iq16: np.ndarray) -> np.ndarray:
    """int16 [n, 2] -> the uint32 words the kernel writes."""
    a = iq16.astype(np.int64)
    return ((a[:, 0] & 0xffff) | ((a[:, 1] & 0xffff) << 16)).astype(np.uint32)


def products(ab: np.ndarray) -> np.ndarray:
    """Steps 3 and 4 for complete blocks: A and B as int64 [m, 4] (A re, A im, B re, B im) -> SAA, SBB, SRE, SIM as int64 [4]."""
    assert len(ab) == 0 or np.abs(ab).max() <= 1 << 39
    r = ab >> 16
    ar, ai, br, bi = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    return np.array([(ar * ar + ai * ai).sum(), (br * br + bi * bi).sum(), (ar * br + ai * bi).sum(), (ai * br - ar * bi).sum()], dtype=np.int64)


class _Target:
    def __init__(self, W: int):
        self.W = W
        self.step, self.mode = 0, TRACK
        self.solved = self.rejected = 0
        self.restart(0)

    def restart(self, position: int) -> None:
        """Step 8: the sums zero, the weight (0, 0) with lead 0, the first counted cell the first that starts at or behind `position`."""
        self.first = (position + CELL - 1) // CELL
        self.ring = np.zeros((self.W, 4), dtype=np.int64)          # cell k in slot k mod W
        self.cell = np.zeros(4, dtype=np.int64)                    # the open cell's partial sums
        self.block = np.zeros(4, dtype=np.int64)                   # the open block's partial A and B
        self.complete = 0
        self.lead, self.w, self.coherence, self.reason = 0, (0, 0), 0, 0
        self.history = []                                          # (cell, lead, weight, coherence, reason) of every cell start solved

    def sums(self):
        return tuple(int(v) for v in self.ring.sum(axis=0))

    def add(self, u4: np.ndarray, position: int) -> None:
        """The mixed-down samples of both rows (int64 [n, 4]) at `position`, which do not reach over a cell's end."""
        n = len(u4)
        assert n and position % CELL + n <= CELL
        ends = np.arange(BLOCK - position % BLOCK, n + 1, BLOCK)   # the piece [.., e) ends a block
        starts = np.concatenate([[0], ends[ends < n]]).astype(np.int64)
        pieces = np.add.reduceat(u4, starts, axis=0)
        pieces[0] += self.block
        done = len(ends)
        if done:
            m0 = position // BLOCK                                 # the first block that ends here
            counted = m0 + np.arange(done) >= self.first * (CELL // BLOCK)
            self.cell += products(pieces[:done][counted])
        self.block = pieces[done].copy() if done < len(pieces) else np.zeros(4, dtype=np.int64)
        assert np.abs(self.cell).max() <= 1 << 55

    def end_cell(self, k: int) -> None:
        if k >= self.first:
            self.ring[k % self.W] = self.cell
            self.complete = min(self.W, self.complete + 1)
        else:
            assert not self.cell.any()
        self.cell = np.zeros(4, dtype=np.int64)


class Combiner:
    """One pair, fed in calls of any length."""

    def __init__(self, fmt: int = CS16, n_targets: int = 1, window_log2: int = WINDOW_LOG2_DEFAULT, position: int = 0):
        assert window_log2 in (0, 1, 2, 4) and 1 <= n_targets <= MAX_TARGETS
        self.fmt, self.window_log2, self.W = fmt, window_log2, 1 << window_log2
        self.targets = [_Target(self.W) for _ in range(n_targets)]
        self.samples = 0
        self.reset(position)

    def reset(self, position: int = 0) -> None:
        """Position `position`, every target anew; the steps, the modes and the counters stay."""
        self.position = position
        for t in self.targets:
            t.restart(position)

    def set_freq(self, target: int, step: int) -> None:
        self.targets[target].step = step & M32
        self.targets[target].restart(self.position)

    def set(self, target: int, lead: int, w_re: int, w_im: int) -> None:
        assert lead in (0, 1) and abs(w_re) <= W_MAX and abs(w_im) <= W_MAX
        self.targets[target].lead, self.targets[target].w = lead, (w_re, w_im)

    def set_mode(self, target: int, mode: int) -> None:
        assert mode in (TRACK, HOLD)
        self.targets[target].mode = mode

    def status(self, target: int = 0) -> dict:
        """What nvx_div_get returns."""
        t = self.targets[target]
        return {"lead": t.lead, "weight": tuple(int(v) for v in t.w), "mode": t.mode, "last_reason": t.reason, "coherence_q14": t.coherence,
                "sums": t.sums(), "step": t.step, "samples": self.samples, "cells_solved": t.solved, "cells_rejected": t.rejected}

    def push(self, main: np.ndarray, second: np.ndarray) -> np.ndarray:
        """-> int16 [n_targets, n, 2]."""
        a, b = rr.convert(main, self.fmt), rr.convert(second, self.fmt)
        assert len(a) == len(b)
        n = len(a)
        out = np.empty((len(self.targets), n, 2), dtype=np.int16)
        for k, t in enumerate(self.targets):
            c, s = nco(t.step, self.position, n)
            u4 = np.concatenate([mix(a, c, s), mix(b, c, s)], axis=1)
            pos, at = self.position, 0
            while at < n:
                if pos % CELL == 0 and t.mode == TRACK and pos // CELL >= t.first + self.W:
                    assert t.complete == self.W
                    t.lead, t.w, t.coherence, t.reason = solve(t.sums())
                    t.solved += t.reason == 0
                    t.rejected += t.reason != 0
                    t.history.append((pos // CELL, t.lead, t.w, t.coherence, t.reason))
                m = min(n - at, CELL - pos % CELL)
                out[k, at:at + m] = apply(a[at:at + m], b[at:at + m], t.lead, t.w)
                t.add(u4[at:at + m], pos)
                pos += m
                at += m
                if pos % CELL == 0:
                    t.end_cell(pos // CELL - 1)
        self.position += n
        self.samples += n
        return out


def combine(main: np.ndarray, second: np.ndarray, steps, fmt: int = CS16, window_log2: int = WINDOW_LOG2_DEFAULT, position: int = 0):
    """One shot with the targets at `steps`: (int16 [n_targets, n, 2], the Combiner behind it)."""
    ref = Combiner(fmt, len(steps), window_log2, position)
    for k, step in enumerate(steps):
        ref.set_freq(k, step)
    return ref.push(main, second), ref
