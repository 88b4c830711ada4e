"""Restatement of the resampler (include/navtex_amd_resample.h), written from the header's contract, not from the kernel:
the input conversions, the polyphase filter in int64 arithmetic with the taps as an argument, the count rule, the
prototype's response, and a small CPFSK source for arbitrary rates (nvx_synth_host makes 2.016 MS/s and 252 kS/s only)."""
from __future__ import annotations

from fractions import Fraction
from math import gcd

import numpy as np

OUTPUT_RATE, S = 252000, 15
CS16, CU8, CS8, CF32 = 0, 1, 2, 3
DTYPES = {CS16: np.int16, CU8: np.uint8, CS8: np.int8, CF32: np.float32}
RATES = (2048000, 2400000, 2000000, 1920000, 3200000, 1024000, 768000, 384000, 256000, 250000, 192000, 96000)
T_OF_RATE = dict(zip(RATES, (58, 68, 58, 56, 92, 30, 22, 12, 8, 8, 8, 12)))
PASS_HZ, STOP_DB, PASS_DB = 25000, -76.0, 0.1


def ratio(fi: int):
    g = gcd(OUTPUT_RATE, fi)
    return OUTPUT_RATE // g, fi // g


def outputs_after(n: int, L: int, M: int) -> int:
    """ceil(n L / M): the outputs a stream has produced once it has consumed n samples."""
    return -((-n * L) // M)


def convert(samples: np.ndarray, fmt: int) -> np.ndarray:
    """[n, 2] samples in format fmt -> int64 in the int16 range."""
    a = np.asarray(samples).reshape(-1, 2)
    if fmt == CS16:
        return a.astype(np.int16).astype(np.int64)
    if fmt == CU8:
        return (2 * a.astype(np.uint8).astype(np.int64) - 255) * 128
    if fmt == CS8:
        return a.astype(np.int8).astype(np.int64) * 256
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.rint(a.astype(np.float32) * np.float32(32768.0))              # one float32 product, ties to even
        y = np.clip(y, np.float32(-32768.0), np.float32(32767.0))
    return np.where(np.isnan(y), 0, y).astype(np.int64)


def resample(x: np.ndarray, taps: np.ndarray, L: int, M: int, consumed: int = 0, history: np.ndarray | None = None):
    """Outputs n with consumed L <= n M < (consumed + len(x)) L of a stream whose samples in front of x are `history`
    (the last len(history) of them; silence before).  x: [n, 2] int64 (converted); taps [L, T].  Returns (int16 [n_out, 2],
    the new history of T-1 samples)."""
    x = np.asarray(x, dtype=np.int64).reshape(-1, 2)
    T = taps.shape[1]
    h = taps.astype(np.int64)
    hist = np.zeros((T - 1, 2), dtype=np.int64)
    if history is not None and len(history):
        hv = np.asarray(history, dtype=np.int64).reshape(-1, 2)[-(T - 1):]
        hist[T - 1 - len(hv):] = hv
    ext = np.concatenate([hist, x])                                            # ext[k + T - 1] = sample consumed + k
    n0, n1 = outputs_after(consumed, L, M), outputs_after(consumed + len(x), L, M)
    n = np.arange(n0, n1, dtype=np.int64)
    pos = n * M
    q, r = pos // L - consumed, pos % L                                        # q: index into x
    acc = np.zeros((len(n), 2), dtype=np.int64)
    for t in range(T):
        acc += h[r, t][:, None] * ext[q - t + T - 1]
    assert len(n) == 0 or (np.abs(acc).max() + (1 << (S - 1)) < 2 ** 31), "the accumulator left int32"
    out = np.clip((acc + (1 << (S - 1))) >> S, -32768, 32767).astype(np.int16)
    return out, ext[len(ext) - (T - 1):]


def resample_all(samples: np.ndarray, fmt: int, taps: np.ndarray, L: int, M: int, block: int = 1 << 22) -> np.ndarray:
    """A whole stream from its reset (in blocks, to bound the memory: the cut changes nothing)."""
    samples = np.asarray(samples).reshape(-1, 2)
    parts, hist = [], None
    for c in range(0, len(samples), block):
        out, hist = resample(convert(samples[c:c + block], fmt), taps, L, M, c, hist)
        parts.append(out)
    return np.concatenate(parts) if parts else np.zeros((0, 2), dtype=np.int16)


def resample_streams(x: np.ndarray, taps: np.ndarray, L: int, M: int, out_block: int = 32) -> np.ndarray:
    """resample() from a reset for many streams of one length at once: x [streams, n, 2] int64 (converted) -> int16
    [streams, n_out, 2].  All streams share (q, r), so a block of outputs is one matrix product of the streams' samples with
    the block's taps laid out by input index.  The products run in float64 and are exact: every term is below 2^31 and every
    partial sum of the at most T terms of an output below 2^53, so the words equal resample()'s."""
    x = np.asarray(x, dtype=np.int64)
    ns, n, T = x.shape[0], x.shape[1], taps.shape[1]
    ext = np.zeros((ns, 2, n + T - 1), dtype=np.float64)                       # ext[.., k + T - 1] = sample k; silence in front
    ext[:, :, T - 1:] = x.transpose(0, 2, 1)
    n_out = outputs_after(n, L, M)
    out = np.empty((ns, n_out, 2), dtype=np.int16)
    for o in range(0, n_out, out_block):
        idx = np.arange(o, min(n_out, o + out_block), dtype=np.int64)
        q, r = idx * M // L, idx * M % L
        lo, hi = int(q[0]), int(q[-1]) + T                                     # ext[lo .. hi): samples q[0] - (T-1) .. q[-1]
        w = np.zeros((hi - lo, len(idx)), dtype=np.float64)
        for t in range(T):
            w[q - t + T - 1 - lo, np.arange(len(idx))] = taps[r, t]
        acc = ext[:, :, lo:hi] @ w                                             # [streams, 2, outputs]
        assert np.abs(acc).max() + (1 << (S - 1)) < 2 ** 31, "the accumulator left int32"
        y = np.clip((acc.astype(np.int64) + (1 << (S - 1))) >> S, -32768, 32767).astype(np.int16)
        out[:, idx, :] = y.transpose(0, 2, 1)
    return out


def response_db(taps: np.ndarray, L: int, fi: int, freqs_hz: np.ndarray) -> np.ndarray:
    """|H(f)| / |H(0)| in dB of the prototype p[r + t L] = taps[r, t] at rate L fi."""
    p = taps.astype(np.float64).T.reshape(-1)                                  # [t, r] flattened: index t L + r
    k = np.arange(len(p))
    out = np.empty(len(freqs_hz))
    for i0 in range(0, len(freqs_hz), 2048):
        f = np.asarray(freqs_hz[i0:i0 + 2048], dtype=np.float64)
        e = np.exp(-2j * np.pi * np.outer(f / (L * fi), k))
        out[i0:i0 + 2048] = np.abs(e @ p)
    return 20 * np.log10(np.maximum(out, 1e-30) / p.sum())


def stop_edge(fi: int) -> int:
    return min(fi, OUTPUT_RATE) - PASS_HZ


# --------------------------------------------------------------------------------------------------------------- source
def cpfsk(bits: str, rate: int, n: int, freq_hz: float = 14000.0, amplitude: float = 8000.0, noise_amp: float = 1500.0,
          shift_hz: float = 85.0, seed: int = 1, bit_offset: int = 0) -> np.ndarray:
    """n samples of int16 IQ at `rate`: 100 Bd continuous-phase FSK of the 'B'/'Y' string (B = +shift, Y = -shift, as the
    product's generator has it; the last bit is held to the end), over uniform noise of +-noise_amp per component."""
    rng = np.random.default_rng(seed)
    sym = np.array([1.0 if c == "B" else -1.0 for c in bits])
    out = np.empty((n, 2), dtype=np.int16)
    turns = 0.0                                                                # the phase in turns, kept small
    for c in range(0, n, 1 << 20):
        t = np.arange(c, min(n, c + (1 << 20)), dtype=np.int64) + bit_offset
        idx = np.minimum(t * 100 // rate, len(sym) - 1)
        ph = turns + np.cumsum((freq_hz + shift_hz * sym[idx]) / rate)
        turns = float(ph[-1] % 1.0)
        iq = amplitude * np.stack([np.cos(2 * np.pi * ph), np.sin(2 * np.pi * ph)], axis=1)
        iq += rng.uniform(-noise_amp, noise_amp, size=iq.shape)
        out[c:c + len(t)] = np.clip(np.rint(iq), -32768, 32767).astype(np.int16)
    return out


def to_format(iq16: np.ndarray, fmt: int, gain: float = 1.0) -> np.ndarray:
    """An int16 source requantised to the format a radio of that kind delivers."""
    if fmt == CS16 and gain == 1.0:
        return np.asarray(iq16, dtype=np.int16)
    a = iq16.astype(np.float64) * gain
    if fmt == CS16:
        return np.clip(np.rint(a), -32768, 32767).astype(np.int16)
    if fmt == CU8:
        return np.clip(np.rint(a / 256.0 + 127.5), 0, 255).astype(np.uint8)
    if fmt == CS8:
        return np.clip(np.rint(a / 256.0), -128, 127).astype(np.int8)
    return (a / 32768.0).astype(np.float32)


def exact_counts(fi: int, chunks) -> list:
    """The count rule in exact rational arithmetic: outputs per chunk of a stream cut into `chunks`."""
    L, M = ratio(fi)
    step, out, seen, made = Fraction(M, L), [], 0, 0
    for c in chunks:
        seen += c
        # every n with n M / L < seen
        total = int(Fraction(seen) / step)
        if Fraction(total) * step < seen:
            total += 1
        out.append(total - made)
        made = total
    return out
