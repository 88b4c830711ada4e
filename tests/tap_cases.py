"""The channel tap's cases, shared by tests/test_tap.py (CPU), tests/test_gpu_tap.py and tests/test_gpu_tap_edges.py: the
rates whose design is held to the
two bars, rows of tones and noise and full-scale random rows, rows at the rails matched to a phase's taps, and the end-to-end
cases -- a 252 kS/s row with stations, the taps that take them out, the way back through the interpolator and where the chain
is tuned.  Nothing is kept: a test that wants several rows at once holds them itself for as long as it runs.  Behind them what
the two GPU files share: the resident call under sentinels (_run_resident, _same), the shifts and pitches set and read back
(_set_shifts, _flat), and the cut plan of the edge cases (edge_cuts)."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import resample_ref as rr
import signals
import tap_ref as tp

IQ_RATES = (2000, 6250, 8000, 11025, 12000, 24000, 48000, 96000)
REAL_RATES = (8000, 11025, 12000, 44100, 48000)
DESIGNS = tuple((fo, tp.IQ) for fo in IQ_RATES) + tuple((fo, tp.REAL) for fo in REAL_RATES)
# recorded from the C design: (L, M, T)
PLAN_OF = {(2000, tp.IQ): (1, 126, 3602), (6250, tp.IQ): (25, 1008, 1154), (8000, tp.IQ): (2, 63, 902), (11025, tp.IQ): (7, 160, 654),
           (12000, tp.IQ): (1, 21, 602), (24000, tp.IQ): (2, 21, 302), (48000, tp.IQ): (4, 21, 152), (96000, tp.IQ): (8, 21, 32),
           (8000, tp.REAL): (2, 63, 3602), (11025, tp.REAL): (7, 160, 3602), (12000, tp.REAL): (1, 21, 3602), (44100, tp.REAL): (7, 40, 3602),
           (48000, tp.REAL): (4, 21, 3602)}

# End to end: stations of amplitude 8000 over noise 1500 in a 252 kS/s row, signals.stream_text(seed), 40 phasing characters.
#   stations: {seed: centre in the row};  rate, kind: of the tap;  back: how the tap's output returns to 252 kS/s --
#   "iq" (narrow_ref's IQ kind), "real" (its REAL kind) or "converter" (real_ref, then the IQ kind with rate_den 2)
E2E = {"i": dict(stations={31: 14000.0, 32: -14000.0}, rate=12000, kind=tp.IQ, back="iq"),
       "ii": dict(stations={33: 14000.0, 34: -14000.0}, rate=48000, kind=tp.IQ, back="iq"),
       "iii": dict(stations={35: 14000.0}, rate=8000, kind=tp.REAL, back="real"),
       "iv": dict(stations={36: 14000.0}, rate=11025, kind=tp.REAL, back="converter"),
       "v": dict(stations={37: 9371.0}, rate=12000, kind=tp.IQ, back="iq")}
AMPLITUDE, NOISE, PHASING = 8000, 1500, 40


def text(seed: int, short: bool = False) -> str:
    """The station's message: signals.stream_text(seed), or a message of one short line (the device tests: a fifth of the row)."""
    if not short:
        return signals.stream_text(seed)
    return f"ZCZC {chr(ord('A') + seed % 26)}{chr(ord('A') + (seed // 26) % 26)}{seed % 100:02d}\nTAP {seed}\nNNNN\n"


def row(nv, case: str, short: bool = False) -> np.ndarray:
    """The 252 kS/s row of the case: int16 [n, 2], its stations summed, noise once."""
    c = E2E[case]
    bits = {seed: nv.sitor_encode(text(seed, short), PHASING) for seed in c["stations"]}
    n = (max(len(b) for b in bits.values()) + 300) * 2520
    total = np.zeros((n, 2), dtype=np.int32)
    for i, (seed, hz) in enumerate(c["stations"].items()):
        total += rr.cpfsk(bits[seed], tp.INPUT_RATE, n, freq_hz=hz, amplitude=AMPLITUDE, noise_amp=NOISE if i == 0 else 0, seed=seed, bit_offset=777 * i)
    return np.clip(total, -32768, 32767).astype(np.int16)


def tuned_hz(case: str, hz: float, k: int, kp: int | None = None) -> float:
    """Where the chain behind the way back is tuned for a station at `hz` taken by a tap at grid step k (and pitch step kp): the
    shift's residue; for audio on top of the applied pitch; through the converter a quarter of the audio rate lower."""
    c = E2E[case]
    residue = Fraction(hz) - Fraction(k * tp.INPUT_RATE, tp.N)
    if c["kind"] == tp.REAL:
        residue += Fraction(kp * c["rate"], tp.N)
        if c["back"] == "converter":
            residue -= Fraction(c["rate"], 4)
    return float(residue)


# ----------------------------------------------------------------------------------------------------------------- rows
def signal(n: int, seed: int) -> np.ndarray:
    """A few tones and noise: int16 [n, 2]."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    z = 9000 * np.exp(2j * np.pi * (0.0007 * k + seed / 7)) + 4000 * np.exp(-2j * np.pi * 0.0113 * k) + 2500 * np.exp(2j * np.pi * 0.31 * k)
    a = np.stack([z.real, z.imag], axis=1) + rng.uniform(-3000, 3000, size=(n, 2))
    return np.rint(a).astype(np.int16)


def full_scale(n: int, seed: int) -> np.ndarray:
    """Full-scale random samples, -32768 among them: int16 [n, 2]."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-32768, 32768, size=(n, 2)).astype(np.int16)
    a[rng.integers(0, n, size=n // 16)] = (-32768, 32767)
    return a


def rails(taps: np.ndarray, L: int, M: int, windows: int) -> np.ndarray:
    """`windows` windows of T samples with silence between them, each matched in sign to the phase r with the largest sum of
    |h|: +full scale where that phase's tap is positive and -full scale where it is negative, every second window negated,
    and Q the negative of I.  A decimator stands on few samples: every window ends on the q of an output of phase r, so
    that output's sum is +-(sum |h|) * full scale (through a tap with k = 0: the mixer would turn the signs away)."""
    T = taps.shape[1]
    r = int(np.abs(taps.astype(np.int64)).sum(axis=1).argmax())
    sign = np.where(taps[r, ::-1] >= 0, 1, -1)              # sample q - t meets h[r][t]: the window ascends, the taps descend
    ends, n, free = [], 0, T - 1
    while len(ends) < windows:
        if (n * M) % L == r and (n * M) // L >= free:
            ends.append((n * M) // L)
            free = ends[-1] + T + 1
        n += 1
    out = np.zeros((ends[-1] + 3, 2), dtype=np.int16)
    for w, q in enumerate(ends):
        s = sign if w % 2 == 0 else -sign
        out[q - T + 1:q + 1, 0] = np.where(s > 0, 32767, -32768)
        out[q - T + 1:q + 1, 1] = np.where(s > 0, -32768, 32767)
    return out


# ------------------------------------------------------------------------------------------------ the edge cases (GPU edges)
# Shifts per input and tap, Hz: input 0 has k = 0 and k = 15, input 1 k = -325 and k = 1 (odd steps: every bit of the sample's
# index counts); the audio kind's pitches: kp = 341 at 12 kS/s (odd) and 512
EDGE_SHIFTS = ((0.0, 922.9), (-20000.0, 61.5))
EDGE_PITCHES = (999.0, 1500.0)
# (tile_out, form, T) of the plans the edge cases run at
EDGE_PLANS = {(2000, tp.IQ): (128, 1, 3602), (2016, tp.IQ): (128, 2, 3574), (12000, tp.REAL): (256, 1, 3602), (12000, tp.IQ): (256, 1, 602),
              (96000, tp.IQ): (256, 2, 32)}


def edge_cuts(L: int, M: int, T: int, tile_out: int) -> list:
    """Calls of 0, 1, T - 2, T - 1, T, 5000, 0, 1, 130, 0, 1 samples -- the five behind the 5000 are shorter than the history, and
    their state row is written from the one read -- and a rest that takes the total to 3 T + 9000 at least and is itself
    longer than a tile: the last call has two tiles and takes its first window from a carried state row."""
    cuts = [0, 1, T - 2, T - 1, T, 5000, 0, 1, 130, 0, 1]
    return cuts + [max(3 * T + 9000 - sum(cuts), (tile_out + 1) * M // L + 1)]


def edge_rows(n: int, fo: int) -> list:
    """The two inputs of the cut case at output rate fo."""
    return [signal(n, 400 + s + fo) for s in range(2)]


def low_run(taps: np.ndarray) -> int:
    """The largest sum of hl = h & 255 over 256 consecutive taps of a phase (over all of them where T < 256), wherever the run
    starts: 32768 times it is what a constant row at the negative rail puts into an int32 run of low halves."""
    hl = taps.astype(np.int64) & 255
    w = min(tp.RUN, hl.shape[1])
    cs = np.concatenate([np.zeros((len(hl), 1), dtype=np.int64), np.cumsum(hl, axis=1)], axis=1)
    return int((cs[:, w:] - cs[:, :-w]).max())


# ------------------------------------------------------------------------------------------------ the resident call (GPU)
SENTINEL = {tp.IQ: 0x5a5a1234, tp.REAL: 0x5a5a}
OUT_DTYPE = {tp.IQ: np.uint32, tp.REAL: np.uint16}


def _run_resident(nv, c, rows, cuts, pitch_extra=0, out_first=0):
    """The inputs' rows (int16 [n, 2], all of one length) through nvx_tap_resident in calls of `cuts` samples; every call's
    input is uploaded to the start of the input rows as whole rows: behind a call's n_in samples the row is full scale up to
    the pitch, so a read behind n_in changes the output.  Sentinels around every output row.  Returns per output row int16
    [outputs, 2] (IQ) or [outputs] (REAL)."""
    ni, n = len(rows), len(rows[0])
    assert sum(cuts) == n and ni == c.n_inputs
    size, dt = tp_bytes(c.kind), OUT_DTYPE[c.kind]
    start = c.position(0)
    n_out = tp.outputs_after(start[0] + n, c.L, c.M) - start[1]
    n_rows = ni * c.n_taps
    pitch_out = out_first + n_out + pitch_extra
    pitch_in = max(max(cuts), 1) + 3 + 5 * pitch_extra
    d_in = nv.DeviceBuffer(ni * pitch_in * 4)
    d_out = nv.DeviceBuffer(max(n_rows * pitch_out, 1) * size)
    d_out.upload(np.full(max(n_rows * pitch_out, 1), SENTINEL[c.kind], dtype=dt))
    block = np.empty((ni, pitch_in, 2), dtype=np.int16)
    pos = made = 0
    for cut in cuts:
        block[:, cut:] = 32767
        for s in range(ni):
            block[s, :cut] = rows[s][pos:pos + cut]
        d_in.upload(block)
        got = c.resident(d_in, pitch_in, cut, d_out, pitch_out, out_first + made)
        assert got == tp.outputs_after(start[0] + pos + cut, c.L, c.M) - tp.outputs_after(start[0] + pos, c.L, c.M), (pos, cut)
        pos += cut; made += got
    assert made == n_out and c.position(ni - 1) == (start[0] + n, start[1] + n_out)
    words = d_out.download(max(n_rows * pitch_out, 1) * size, dtype=dt)[:n_rows * pitch_out].reshape(n_rows, pitch_out)
    d_in.free(); d_out.free()
    assert np.all(words[:, :out_first] == SENTINEL[c.kind]) and np.all(words[:, out_first + n_out:] == SENTINEL[c.kind]), "samples outside the span were written"
    body = np.ascontiguousarray(words[:, out_first:out_first + n_out]).view(np.int16)
    return [body[r].reshape(n_out, 2) if c.kind == tp.IQ else body[r] for r in range(n_rows)]


def tp_bytes(kind):
    return 4 if kind == tp.IQ else 2


def _same(got, want, what):
    assert len(got) == len(want)
    for s in range(len(want)):
        assert got[s].shape == want[s].shape, (what, s, got[s].shape, want[s].shape)
        if not np.array_equal(got[s], want[s]):
            diff = got[s] != want[s]
            first = int(np.argmax(diff.reshape(len(diff), -1).any(axis=1)))
            raise AssertionError((what, "row", s, "first difference at", first, got[s][first], want[s][first], "differences", int(diff.sum())))


def _set_shifts(c, shifts, kind, pitches=None):
    """Shifts (Hz per input and tap) and pitches (Hz per tap, every input) -> (ks per input, kps per tap) as applied."""
    ks = []
    for i, per_tap in enumerate(shifts):
        for t, hz in enumerate(per_tap):
            applied = c.set_shift(t, hz, input=i)
            k = tp.grid(c.rate, kind, hz)
            assert c.get_shift(t, i) == (k, applied) and applied == k * 252000 / 4096
        ks.append([tp.grid(c.rate, kind, hz) for hz in per_tap])
    kps = None
    if kind == tp.REAL:
        kps = []
        for t, hz in enumerate(pitches):
            if hz is not None:
                applied = c.set_pitch(t, hz)
                assert applied == tp.pitch_grid(c.rate, hz) * c.rate / 4096
            kps.append(c.get_pitch(t)[0])
            assert kps[-1] == tp.pitch_grid(c.rate, hz if hz is not None else tp.DEFAULT_PITCH_HZ)
    return ks, kps


def _flat(per_input):
    return [row for rows in per_input for row in rows]
