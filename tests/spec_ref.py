"""The spectrum monitor restated from the text of include/navtex_amd_spec.h in numpy: conversion, window, the transform stage
by stage, power and lag products, line sums, level words, the survey in ascending line order, the carry through calls of any
length, and the finder.  Every product and every sum is a numpy operation of its own, so each is rounded on its own as the
header demands; the header's bounds are asserted where the numbers arise.  The GPU tests hold the library against this with
== (the finder: with tolerances)."""
from __future__ import annotations

import functools
import math
import re
from pathlib import Path

import numpy as np

import resample_ref as rr

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_spec.h"
TABLE = ROOT / "navtex_amd" / "spec" / "nvx_spec_table.h"
CS16, CU8, CS8, CF32 = rr.CS16, rr.CU8, rr.CS8, rr.CF32
LOG2_MIN, LOG2_MAX, LOG2_DEFAULT, AVG_DEFAULT, MAX_HOP = 8, 12, 11, 8, 65536
TAB_N, TAB_OCT = 4096, 512
LEVEL_ZERO = 991 << 8
DEFAULTS = dict(guard_bins=3, min_lines=8, min_coherence=0.95, min_score_db=6.0)
ERR_ARG = -1


def octant():
    """[(cos, sin)] of 2 pi j / 4096, j = 0 .. 512, as the header holds them."""
    body = TABLE.read_text().split("NVX_SPEC_OCTANT", 1)[1]
    pairs = re.findall(r"\{\s*([-+0-9a-fx.p]+),\s*([-+0-9a-fx.p]+)\s*\}", body)
    assert len(pairs) == TAB_OCT + 1
    return [(float.fromhex(c), float.fromhex(s)) for c, s in pairs]


@functools.lru_cache(maxsize=None)
def table():
    """(C, S) [4096] each: cos and sin of 2 pi j / 4096 from the octant by the exact symmetries (nvx_spec_cs)."""
    oc = np.array(octant())
    quarter = TAB_N // 4
    r = np.arange(quarter)
    c = np.where(r <= TAB_OCT, oc[np.minimum(r, TAB_OCT), 0], oc[quarter - np.maximum(r, TAB_OCT), 1])
    s = np.where(r <= TAB_OCT, oc[np.minimum(r, TAB_OCT), 1], oc[quarter - np.maximum(r, TAB_OCT), 0])
    C = np.concatenate([c, -s, -c, s])
    S = np.concatenate([s, c, -s, -c])
    return C, S


@functools.lru_cache(maxsize=None)
def plan_tables(n_log2: int):
    """(C_N, S_N, the window, the bit reversal) of N = 2^n_log2."""
    N = 1 << n_log2
    C, S = table()
    CN, SN = C[::TAB_N // N].copy(), S[::TAB_N // N].copy()
    w = 0.5 - 0.5 * CN
    assert w.min() >= 0.0 and w.max() <= 1.0 and w[0] == 0.0 and w[N // 2] == 1.0
    rev = np.array([int(format(i, f"0{n_log2}b")[::-1], 2) for i in range(N)])
    return CN, SN, w, rev


def fft(vre: np.ndarray, vim: np.ndarray, n_log2: int):
    """The header's transform of [S, N] windowed segments: bit-reversed input, stages len = 2 .. N, its butterfly."""
    N = 1 << n_log2
    CN, SN, _, rev = plan_tables(n_log2)
    S = vre.shape[0]
    xre, xim = np.empty_like(vre), np.empty_like(vim)
    xre[:, rev], xim[:, rev] = vre, vim                     # x[rev(n)] = v[n]
    length = 2
    while length <= N:
        half = length // 2
        wr, wi = CN[np.arange(half) * (N // length)], -SN[np.arange(half) * (N // length)]
        xr, xi = xre.reshape(S, N // length, 2, half), xim.reshape(S, N // length, 2, half)
        are, aim, bre, bim = xr[:, :, 0, :], xi[:, :, 0, :], xr[:, :, 1, :], xi[:, :, 1, :]
        tre = bre * wr - bim * wi
        tim = bre * wi + bim * wr
        nre, nim = np.empty_like(xr), np.empty_like(xi)
        nre[:, :, 0, :], nim[:, :, 0, :] = are + tre, aim + tim
        nre[:, :, 1, :], nim[:, :, 1, :] = are - tre, aim - tim
        xre, xim = nre.reshape(S, N), nim.reshape(S, N)
        length *= 2
    return xre, xim


def level_words(p_line: np.ndarray) -> np.ndarray:
    """The level word of every power: clamp((u >> 44) - (991 << 8), 0, 65535)."""
    u = np.ascontiguousarray(p_line, dtype=np.float64).view(np.uint64)
    v = (u >> np.uint64(44)).astype(np.int64) - LEVEL_ZERO
    assert v.max(initial=0) <= (64 + 32) * 256, "the header's bound on the level word"
    return np.clip(v, 0, 65535).astype(np.uint16)


def level_db(words) -> np.ndarray:
    """NVX_SPEC_LEVEL_DB."""
    return 3.010299956639812 * (np.asarray(words, dtype=np.float64) / 256.0 - 32.0)


def lines_at(p: int, n_log2: int, avg: int) -> int:
    """How many lines are complete at position p."""
    H = 1 << (n_log2 - 1)
    span, hop = (avg + 1) * H, avg * H
    return 0 if p < span else (p - span) // hop + 1


class Spectrum:
    """One row of a plan.  push() returns the level words [lines, N] of the lines the call completes; the survey is in
    .sp, .sc_re, .sc_im and .lines, in the order of an output line."""
    LINES_AT_ONCE = 24

    def __init__(self, fmt: int = CS16, n_log2: int = LOG2_DEFAULT, avg: int = AVG_DEFAULT, position: int = 0):
        assert LOG2_MIN <= n_log2 <= LOG2_MAX and avg >= 1 and avg << (n_log2 - 1) <= MAX_HOP
        self.fmt, self.n_log2, self.avg = fmt, n_log2, avg
        self.N, self.H = 1 << n_log2, 1 << (n_log2 - 1)
        self.span, self.hop = (avg + 1) * self.H, avg * self.H
        self.set_position(position)

    def set_position(self, position: int) -> None:
        """As after a reset at `position`: silence in front of it."""
        self.position = position
        done = lines_at(position, self.n_log2, self.avg)
        self.carry = np.zeros((position - done * self.hop, 2), dtype=np.int64)      # the samples behind the last complete line
        self.measure()

    def reset(self) -> None:
        self.set_position(0)

    def measure(self) -> None:
        self.origin = self.position
        self.sp, self.sc_re, self.sc_im = np.zeros(self.N), np.zeros(self.N), np.zeros(self.N)
        self.lines = 0

    def lines_for(self, n_in: int) -> int:
        return lines_at(self.position + n_in, self.n_log2, self.avg) - lines_at(self.position, self.n_log2, self.avg)

    def line_sums(self, x: np.ndarray):
        """(P_line, C_line.re, C_line.im), [lines, N] each in FFT bin order, of converted samples x that begin on a line."""
        N, H, A = self.N, self.H, self.avg
        n_lines = (len(x) - self.span) // self.hop + 1
        _, _, w, _ = plan_tables(self.n_log2)
        assert np.abs(x).max(initial=0) <= 32768
        seg = np.lib.stride_tricks.sliding_window_view(x.astype(np.float64), (N, 2))[::H, 0][:n_lines * A]      # [S, N, 2]
        vre, vim = w * seg[:, :, 0], w * seg[:, :, 1]
        zre, zim = fft(vre, vim, self.n_log2)
        zre, zim = zre.reshape(n_lines, A, N), zim.reshape(n_lines, A, N)
        p = zre * zre + zim * zim
        assert p.max(initial=0.0) < 2.0 ** 55
        P, Cr, Ci = np.zeros((n_lines, N)), np.zeros((n_lines, N)), np.zeros((n_lines, N))
        for s in range(A):                                   # ascending segment order, from 0.0
            P = P + p[:, s]
            if s:
                a_re, a_im, b_re, b_im = zre[:, s], zim[:, s], zre[:, s - 1], zim[:, s - 1]
                Cr = Cr + (a_re * b_re + a_im * b_im)
                Ci = Ci + (a_im * b_re - a_re * b_im)
        return P, Cr, Ci

    def push(self, samples: np.ndarray) -> np.ndarray:
        x = np.concatenate([self.carry, rr.convert(samples, self.fmt)])
        assert len(self.carry) < self.span
        first = lines_at(self.position, self.n_log2, self.avg)         # the absolute index of the first line this call completes
        n_lines = self.lines_for(len(x) - len(self.carry))
        out = np.zeros((n_lines, self.N), dtype=np.uint16)
        for l0 in range(0, n_lines, self.LINES_AT_ONCE):
            l1 = min(n_lines, l0 + self.LINES_AT_ONCE)
            P, Cr, Ci = self.line_sums(x[l0 * self.hop:(l1 - 1) * self.hop + self.span])
            # index i of a line holds bin (i + N/2) mod N
            P, Cr, Ci = (np.roll(v, self.H, axis=1) for v in (P, Cr, Ci))
            out[l0:l1] = level_words(P)
            for j in range(l1 - l0):                         # ascending line order; a line counts if it begins at or behind the restart
                if (first + l0 + j) * self.hop >= self.origin:
                    self.sp, self.sc_re, self.sc_im = self.sp + P[j], self.sc_re + Cr[j], self.sc_im + Ci[j]
                    self.lines += 1
        self.position += len(x) - len(self.carry)
        self.carry = x[n_lines * self.hop:]
        assert len(self.carry) == self.position - lines_at(self.position, self.n_log2, self.avg) * self.hop < self.span
        return out

    def get(self):
        return self.sp.copy(), self.sc_re.copy(), self.sc_im.copy(), self.lines

    def find_lines(self, **params):
        return find_lines(self.sp, self.sc_re, self.sc_im, self.n_log2, self.avg, self.lines, **params)


def spectrum(samples, fmt=CS16, n_log2=LOG2_DEFAULT, avg=AVG_DEFAULT, cuts=None, position=0):
    """(level words [lines, N], the Spectrum) of a row fed in one call, or in calls of the lengths in `cuts`."""
    ref = Spectrum(fmt, n_log2, avg, position)
    a = np.asarray(samples).reshape(-1, 2)
    parts, at = [], 0
    for cut in (cuts if cuts is not None else [len(a)]):
        parts.append(ref.push(a[at:at + cut])); at += cut
    assert at == len(a)
    return np.concatenate(parts), ref


def coherence(sp, sc_re, sc_im, avg):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sp > 0, np.sqrt(sc_re * sc_re + sc_im * sc_im) * avg / ((avg - 1) * sp), 0.0)


def find_lines(sp, sc_re, sc_im, n_log2, avg, lines, **params):
    """The header's finder, rules 1 to 7: a list of dicts in the order kept, or ERR_ARG."""
    p = dict(DEFAULTS, **params)
    if avg < 2 or lines < p["min_lines"]:
        return ERR_ARG
    N = 1 << n_log2
    floor_p = np.sort(sp)[N // 2]
    g = coherence(sp, sc_re, sc_im, avg)
    cand = [i for i in range(N) if sp[i] > 0 and sp[i] >= floor_p * 10.0 ** (p["min_score_db"] / 10.0) and g[i] >= p["min_coherence"]]
    cand.sort(key=lambda i: (-sp[i], i))
    kept, hits = [], []
    for i in cand:
        if any(min(abs(i - k), N - abs(i - k)) <= p["guard_bins"] for k in kept):
            continue
        kept.append(i)
        k = i - N // 2
        sign = -1.0 if k & 1 else 1.0
        delta = math.atan2(sc_im[i] * sign, sc_re[i] * sign) / math.pi
        cycles = (k + delta) / N
        hits.append(dict(cycles_per_sample=cycles, step=int(np.rint((cycles - math.floor(cycles)) * 4294967296.0)) & 0xffffffff,
                         coherence=float(g[i]), score_db=10.0 * math.log10(sp[i] / floor_p) if floor_p > 0 else math.inf, bin=i))
    return hits
