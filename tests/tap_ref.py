"""Restatement of the channel tap (include/navtex_amd_tap.h), written from the header's contract, not from the kernel: the
rate's L / M, the grid rules of shift and pitch over the rationals, the bank's mixer (tests/ddc_ref.py, as it is) with the
sample's true index, the polyphase sum in int64 numpy with the taps as an argument (and one output at a time in Python
integers, output_int, which the tests hold the numpy against), the pitch epilogue of the REAL kind, the count rule, the
carried unmixed state of an input cut into calls anywhere, the design recipe in numpy, and the prototype's response.  The
bounds the header states -- the high half's sum inside int32, a run of 256 low halves inside int32, |acc| + 2^20 < 2^40 --
are asserted on every call."""
from __future__ import annotations

from fractions import Fraction
from math import ceil, pi

import numpy as np

import ddc_ref as dr
import resample_ref as rr

INPUT_RATE, S, N = 252000, 21, 4096
IQ, REAL = 0, 1
PASS_HZ, PASS_FRACTION, STOP_DB, PASS_DB, DESIGN_DB = 25000, Fraction(2, 5), -76.0, 0.1, 90.0
AUDIO_PASS_HZ, AUDIO_STOP_HZ, DEFAULT_PITCH_HZ = 400, 800, 1000
RATE_RANGE = {IQ: (2000, 96000), REAL: (8000, 48000)}
MAX_TAPS, RUN = 32768, 256


def ratio(fo: int):
    """(L, M): fo / 252000 in lowest terms."""
    f = Fraction(fo, INPUT_RATE)
    return f.numerator, f.denominator


def edges(fo: int, kind: int):
    """(pass edge, stop edge) in Hz, exact."""
    if kind == REAL:
        return Fraction(AUDIO_PASS_HZ), Fraction(AUDIO_STOP_HZ)
    fp = min(Fraction(PASS_HZ), PASS_FRACTION * fo)
    return fp, fo - fp


def outputs_after(n: int, L: int, M: int) -> int:
    """ceil(n L / M): the outputs a tap has produced once its input has consumed n samples."""
    return -((-n * L) // M)


def grid(fo: int, kind: int, hz):
    """k = rint(hz N / 252000), ties to even, over the rationals; None outside |k fi / N| <= 126000 - fp."""
    k = round(Fraction(hz) * N / INPUT_RATE)
    return k if abs(Fraction(k * INPUT_RATE, N)) <= INPUT_RATE // 2 - edges(fo, kind)[0] else None


def pitch_grid(fo: int, pitch_hz):
    """kp = rint(pitch N / fo), ties to even; None outside 800 <= kp fo / N <= fo / 2 - 800."""
    kp = round(Fraction(pitch_hz) * N / fo)
    return kp if AUDIO_STOP_HZ <= Fraction(kp * fo, N) <= Fraction(fo, 2) - AUDIO_STOP_HZ else None


def pack(iq16: np.ndarray) -> np.ndarray:
    """int16 [n, 2] -> the uint32 words the kernel writes."""
    a = iq16.astype(np.int64)
    return ((a[:, 0] & 0xffff) | ((a[:, 1] & 0xffff) << 16)).astype(np.uint32)


def check_split(taps: np.ndarray) -> None:
    """The bounds of the split h = 256 hh + hl that hold for the taps alone: sum |hh| <= 65535 per phase (the high half's sum
    stays inside int32 over a whole window of full-scale samples), and 255 * 32768 * 256 < 2^31 (so does a run of 256 low
    halves)."""
    h = taps.astype(np.int64)
    hh, hl = h >> 8, h & 255
    assert np.array_equal(256 * hh + hl, h) and hl.min() >= 0 and hl.max() <= 255 and np.abs(hh).max() <= 32767
    assert np.abs(hh).sum(axis=1).max() <= 65535 and np.abs(hh).sum(axis=1).max() * 32768 < 2 ** 31
    assert 255 * 32768 * RUN < 2 ** 31
    assert np.abs(h).sum(axis=1).max() < 1 << 24


def pitch_turn(y: np.ndarray, kp: int, m_first: int) -> np.ndarray:
    """The REAL epilogue: y int64 [n, 2] are outputs m_first, m_first + 1, ... -> int16 [n]."""
    w = dr.table()
    j = (kp * ((m_first + np.arange(len(y), dtype=np.int64)) % N)) % N
    a = y[:, 0] * w[j, 0] - y[:, 1] * w[j, 1] + (1 << 14)
    assert len(a) == 0 or np.abs(a).max() < 2 ** 31
    return np.clip(a >> 15, -32768, 32767).astype(np.int16)


def output_int(x, taps, L: int, M: int, n: int, k: int = 0):
    """Output n of a tap whose input's samples since the reset are x[0 ...] ([q, 2]), in Python integers:
    ((I, Q), (acc_I, acc_Q))."""
    T = taps.shape[1]
    w = dr.table()
    pos = n * M
    q, r = pos // L, pos % L
    assert q < len(x)

    def mixed(i):
        if i < 0:
            return (0, 0)
        a, b = int(x[i, 0]), int(x[i, 1])
        if k == 0:
            return (a, b)
        c, s = int(w[(k * i) % N, 0]), int(w[(k * i) % N, 1])
        cl = lambda v: max(-32768, min(32767, v))
        return (cl((a * c + b * s + (1 << 14)) >> 15), cl((b * c - a * s + (1 << 14)) >> 15))

    win = [mixed(q - t) for t in range(T)]
    accs, outs = [], []
    for comp in (0, 1):
        hh = sum((int(taps[r, t]) >> 8) * win[t][comp] for t in range(T))
        assert abs(hh) < 1 << 31
        acc = 0
        for t0 in range(0, T, RUN):
            run = sum((int(taps[r, t]) & 255) * win[t][comp] for t in range(t0, min(T, t0 + RUN)))
            assert abs(run) < 1 << 31
            acc += run
        acc += 256 * hh
        assert acc == sum(int(taps[r, t]) * win[t][comp] for t in range(T)) and abs(acc) + (1 << (S - 1)) < 1 << 40
        accs.append(acc)
        outs.append(max(-32768, min(32767, (acc + (1 << (S - 1))) >> S)))
    return tuple(outs), tuple(accs)


class Tap:
    """One input and its taps, fed in calls of any length.  ks: the taps' shifts in grid steps; kps: their pitches (REAL)."""

    def __init__(self, taps: np.ndarray, L: int, M: int, kind: int = IQ, ks=(0,), kps=None, position: int = 0):
        self.h, self.L, self.M, self.T = taps.astype(np.int64), L, M, taps.shape[1]
        assert taps.shape == (L, self.T)
        check_split(taps)
        self.kind, self.ks = kind, list(ks)
        self.kps = list(kps) if kps is not None else [None] * len(self.ks)
        self.reset(position)

    def reset(self, position: int = 0) -> None:
        """Input sample `position`, silence in front of it.  Shifts and pitches stay."""
        self.consumed = position
        self.hist = np.zeros((self.T - 1, 2), dtype=np.int64)
        self.acc_min = self.acc_max = 0

    @property
    def produced(self) -> int:
        return outputs_after(self.consumed, self.L, self.M)

    def push(self, x: np.ndarray) -> list:
        """Any number of int16 IQ samples [n, 2] -> per tap int16 [outputs, 2] (IQ) or [outputs] (REAL)."""
        c = np.asarray(x, dtype=np.int64).reshape(-1, 2)
        L, M, T = self.L, self.M, self.T
        ext = np.concatenate([self.hist, c])                                   # ext[i + T - 1] = sample consumed + i, unmixed
        n0, n1 = self.produced, outputs_after(self.consumed + len(c), L, M)
        e = n0 * M - self.consumed * L                                         # pos relative to consumed L, in Python integers
        assert 0 <= e < M
        n_out = n1 - n0
        first = max(self.consumed - (T - 1), 0)                                # samples before the reset are silence
        outs = []
        for k, kp in zip(self.ks, self.kps):
            mixed = ext.copy()
            lead = T - 1 - (self.consumed - first)
            mixed[lead:] = dr.mix(ext[lead:], k, first)                        # the carried samples with their true index and the current k
            acc = np.zeros((n_out, 2), dtype=np.int64)
            every = [np.ascontiguousarray(mixed[p::M]) for p in range(min(M, len(mixed)))] if n_out else []     # mixed[s::M] is every[s % M][s // M:]
            for j in range(min(L, n_out)):                                     # outputs j, j + L, ...: one phase, q in steps of M
                rel = e + j * M
                q0, r = rel // L, rel % L
                part = np.zeros((len(acc[j::L]), 2), dtype=np.int64)
                for t in range(T):
                    s = q0 - t + T - 1
                    part += self.h[r, t] * every[s % M][s // M:s // M + len(part)]
                acc[j::L] = part
            if n_out:
                assert np.abs(acc).max() + (1 << (S - 1)) < 1 << 40, "the accumulator left 40 bits"
                self.acc_min, self.acc_max = min(self.acc_min, int(acc.min())), max(self.acc_max, int(acc.max()))
            y = np.clip((acc + (1 << (S - 1))) >> S, -32768, 32767)
            outs.append(y.astype(np.int16) if self.kind == IQ else pitch_turn(y, kp, n0))
        self.hist = ext[len(ext) - (T - 1):]
        self.consumed += len(c)
        return outs


def tap_all(x: np.ndarray, taps: np.ndarray, L: int, M: int, kind: int = IQ, ks=(0,), kps=None, position: int = 0):
    """One shot: (the taps' outputs, the Tap behind them)."""
    ref = Tap(taps, L, M, kind, ks, kps, position)
    return ref.push(x), ref


# ---------------------------------------------------------------------------------------------------------------- design
def design(fo: int, kind: int = IQ):
    """The header's recipe in numpy: (L, M, T, int32 taps [L, T])."""
    L, M = ratio(fo)
    fp, fs = (float(v) for v in edges(fo, kind))
    rate = L * INPUT_RATE
    dw = 2 * pi * (fs - fp) / rate
    order = (DESIGN_DB - 7.95) / (2.285 * dw)
    T = int(ceil((order + 1) / L))
    T += T & 1
    T = max(T, 8)
    assert L * T <= MAX_TAPS
    nt = L * T
    fc = 0.5 * (fp + fs) / rate
    beta = 0.1102 * (DESIGN_DB - 8.7)
    centre = 0.5 * (nt - 1)
    d = np.arange(nt) - centre
    p = 2 * fc * np.sinc(2 * fc * d) * np.i0(beta * np.sqrt(1 - (d / (centre + 0.5)) ** 2)) / np.i0(beta)
    ph = p.reshape(T, L).T                                                     # [r, t] = p[r + t L]
    h = np.rint(ph / ph.sum(axis=1, keepdims=True) * (1 << S)).astype(np.int64)
    big = np.abs(h).argmax(axis=1)
    h[np.arange(L), big] += (1 << S) - h.sum(axis=1)
    return L, M, T, h.astype(np.int32)


def response_fft(taps: np.ndarray, L: int, oversample: int = 16):
    """(frequencies in Hz from 0 to L * 126000, |H(f)| / |H(0)| in dB) of the prototype on an FFT grid of at least `oversample`
    points per bin of the prototype's length (a side lobe of the window is about one such bin wide)."""
    p = taps.astype(np.float64).T.reshape(-1)
    nfft = 1 << int(np.ceil(np.log2(oversample * len(p))))
    mag = np.abs(np.fft.rfft(p, nfft))
    return np.arange(len(mag)) * (L * INPUT_RATE / nfft), 20 * np.log10(np.maximum(mag, 1e-30) / p.sum())


def response_db(taps: np.ndarray, L: int, freqs_hz: np.ndarray) -> np.ndarray:
    """|H(f)| / |H(0)| in dB of the prototype p[r + t L] = taps[r, t] at rate L * 252000."""
    return rr.response_db(taps, L, INPUT_RATE, freqs_hz)


def exact_counts(fo: int, start: int, chunks) -> list:
    """The count rule in exact rational arithmetic: outputs per call of an input that stands at `start` and is cut into
    `chunks`: every n with n / fo < seen / 252000."""
    step = Fraction(INPUT_RATE, fo)                                            # input samples per output
    def made(seen):
        total = int(Fraction(seen) / step)
        return total + 1 if Fraction(total) * step < seen else total
    out, seen = [], start
    for c in chunks:
        out.append(made(seen + c) - made(seen))
        seen += c
    return out
