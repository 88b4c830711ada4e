"""The zoom bank's cases, shared by tests/test_zoom.py (CPU), tests/test_gpu_zoom.py and tests/test_gpu_zoom_edges.py: the
wide row of a radio at 1.008 MS/s with the three NAVTEX services far apart and an interferer one output band beside the weak
one, what a user without the zoom would do with it (zoom_ref.naive), tones on FFT bins, the rails of the mixer and of a
stage, full-scale random rows, and rows of a few tones in every format.  Nothing is kept: a test that wants several rows at
once holds them itself for as long as it runs.  Behind them what the two GPU files share: the resident call under sentinels
(_run_resident, _first_difference)."""
from __future__ import annotations

import numpy as np

import iqc_cases as ic
import real_cases as rc
import resample_ref as rr
import signals
import zoom_ref as zr

SEEDS = ic.SEEDS
RATE, K = 1008000, 2                       # of the wide row; the zoomed rows have ic.RATE = 252 000
HZ_A, HZ_B = -300000.0, 350000.0           # where the two zooms are asked to sit; the grid puts them 11.7 Hz and 15.6 Hz beside
AMP_518, AMP_490 = ic.AMP_518, ic.AMP_490
TEXT_INTERFERER, TEXT_4209 = 5, 9
BIT_OFFSET_490 = ic.BIT_OFFSET_490
# Uniform noise of +-NOISE per component on the wide row.  The rule: start at iqc_cases' 1500 and lower it in steps of 250
# until the restatement's zoom-A row delivers the 490 message from twelve seeds of twelve; 1500 does (tests/test_zoom.py holds
# it to that).
NOISE = ic.NOISE
# The interferer's amplitude.  The rule: start at AMP_518 and double it, to at most 12 000, until the naive row delivers the
# 490 message from none of twelve seeds; 8000 does (tests/test_zoom.py holds it to that).
INTERFERER = AMP_518
TONE_OUTPUTS, TONE_AMP = 4096, 20000
TONE_BINS = (37, -1000, 1638, -1638)       # of 4096 outputs; the inner 80 % of the band ends at +-1638


def centres():
    """((kz, applied Hz) of zoom A, of zoom B) by the grid rule."""
    ka, kb = zr.grid(RATE, HZ_A), zr.grid(RATE, HZ_B)
    return (ka, ka * RATE / zr.N), (kb, kb * RATE / zr.N)


def texts():
    """(the 518 text, the 490 text, the interferer's, the 4209 one)."""
    return ic.texts() + (signals.stream_text(TEXT_INTERFERER), signals.stream_text(TEXT_4209))


def wide_row(nv, seed: int, noise: float = NOISE, interferer: float = INTERFERER) -> np.ndarray:
    """int16 [4 n, 2], n whole frames of 252 kS/s: 518 at +14 kHz and 490 at -14 kHz of zoom A's applied centre, the interferer
    252 kHz above the 490 carrier, the third station at +14 kHz of zoom B's applied centre."""
    (_, fa), (_, fb) = centres()
    bits = [nv.sitor_encode(t, 40) for t in texts()]
    n = (max(len(b) for b in bits) + 300) * 2520 // nv.FRAME_IN * nv.FRAME_IN * (1 << K)
    a = rr.cpfsk(bits[0], RATE, n, freq_hz=fa + 14000, amplitude=AMP_518, noise_amp=0, seed=seed).astype(np.int32)
    a += rr.cpfsk(bits[1], RATE, n, freq_hz=fa - 14000, amplitude=AMP_490, noise_amp=noise, seed=seed, bit_offset=BIT_OFFSET_490)
    a += rr.cpfsk(bits[2], RATE, n, freq_hz=fa - 14000 + 252000, amplitude=interferer, noise_amp=0, seed=seed, bit_offset=777)
    a += rr.cpfsk(bits[3], RATE, n, freq_hz=fb + 14000, amplitude=AMP_518, noise_amp=0, seed=seed, bit_offset=4321)
    return np.clip(a, -32768, 32767).astype(np.int16)


delivered = ic.delivered


# ---------------------------------------------------------------------------------------------------------------- edges
def tone(k: int, kz: int, b: int, fold: int = 0, outputs: int = TONE_OUTPUTS, amp: float = TONE_AMP, lead: int = 64) -> np.ndarray:
    """A complex tone that comes out on bin b of an FFT over `outputs` outputs of a zoom at step kz: input frequency
    kz / 4096 + (b + fold * outputs) / (D outputs) cycles per sample -- fold = 1 .. D - 1 puts it on an alias of the bin --,
    D (lead + outputs) samples as int16 [n, 2] (the first `lead` outputs are the filters filling)."""
    D = 1 << k
    n = np.arange(D * (lead + outputs), dtype=np.int64)
    den = zr.N * D * outputs                                 # the frequency in units of 1 / den cycles per sample, exactly
    turns = ((kz * D * outputs + (b + fold * outputs) * zr.N) * n) % den
    ph = 2 * np.pi * turns / float(den)
    return np.rint(amp * np.stack([np.cos(ph), np.sin(ph)], axis=1)).astype(np.int16)


def tone_levels(iq: np.ndarray, b: int, amp: float = TONE_AMP):
    """(rms of the last TONE_OUTPUTS outputs in dB against a complex tone of amplitude amp, level on bin b in dB against
    one, Blackman window)."""
    n = TONE_OUTPUTS
    z = (iq[-n:, 0].astype(np.float64) + 1j * iq[-n:, 1].astype(np.float64))
    w = np.blackman(n)
    f = np.abs(np.fft.fft(z * w))
    rms = np.sqrt(np.mean(np.abs(z) ** 2))
    return float(20 * np.log10(max(rms, 1e-9) / amp)), float(20 * np.log10(max(f[b % n], 1e-9) / (amp * w.sum())))


def lowest(fmt: int):
    return np.float32(-1.0) if fmt == zr.CF32 else np.iinfo(zr.DTYPES[fmt]).min


def highest(fmt: int):
    return np.float32(1.0) if fmt == zr.CF32 else np.iinfo(zr.DTYPES[fmt]).max


def rails_low(fmt: int, n: int) -> np.ndarray:
    """Every component at the format's lowest value: with kz = 512 every eighth sample stands at 45 degrees of the table and
    the mixer's sum reaches +-46340 and clamps."""
    return np.full((n, 2), lowest(fmt), dtype=zr.DTYPES[fmt])


def rails_taps(fmt: int, n: int, period: int = 128) -> np.ndarray:
    """Bursts of 55 samples every `period`, alternately with the signs of the stage's taps and against them (zero taps count
    as positive), full scale on both components; the format's lowest value between them.  Stage 1's sum for the output centred
    on a burst is the largest, or the smallest, the format allows, and the output clamps."""
    h = zr.lowpass()
    x = np.full((n, 2), lowest(fmt), dtype=zr.DTYPES[fmt])
    for i, c in enumerate(range(64, n - 64, period)):       # c is even: sample c is a stage-1 output's centre
        up = (h[::-1] >= 0) if i % 2 == 0 else (h[::-1] < 0)
        x[c - 27:c + 28, :] = np.where(up, highest(fmt), lowest(fmt))[:, None]
    return x


def full_scale(fmt: int, n: int, seed: int) -> np.ndarray:
    """Full-scale random samples [n, 2] in format fmt; float32 with the specials of the CF32 rule (real_cases.full_scale)."""
    return rc.full_scale(fmt, 2 * n, seed).reshape(n, 2)


def signal(fmt: int, n: int, seed: int) -> np.ndarray:
    """A few complex tones across the band and noise, [n, 2] in format fmt: rows for the cut and format cases."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    z = 9000 * np.exp(2j * np.pi * (0.27 * t + seed / 7.0)) + 5000 * np.exp(-2j * np.pi * 0.113 * t) + 3000 * np.exp(2j * np.pi * 0.0031 * t)
    a = np.stack([z.real, z.imag], axis=1) + rng.uniform(-3000, 3000, size=(n, 2))
    return rr.to_format(np.rint(a).astype(np.int16), fmt)


# ------------------------------------------------------------------------------------------------ the resident call (GPU)
SENTINEL = 0x5a5a1234


def _run_resident(nv, z, rows, cuts, pitch_extra=0, out_first=0):
    """The rows ([n, 2] samples each, all of one length) through nvx_zoom_resident in calls of `cuts` samples (multiples of D);
    every call's input is uploaded to the start of the input rows as whole rows: behind a call's n_in samples the row is full
    scale up to the pitch, so a read behind n_in changes the output.  Sentinels around every output row.  Returns int16
    [inputs * zooms, n / D, 2]."""
    ni, n, D = len(rows), len(rows[0]), z.decim
    assert sum(cuts) == n and ni == z.n_inputs and n % D == 0
    dt = rows[0].dtype
    n_rows = ni * z.n_zooms
    pitch_out = out_first + n // D + pitch_extra
    pitch_in = (max(max(cuts), 1) + 15) // 16 * 16 + 16 * pitch_extra
    d_in = nv.DeviceBuffer(ni * pitch_in * 2 * dt.itemsize)
    d_out = nv.DeviceBuffer(n_rows * pitch_out * 4)
    d_out.upload(np.full(n_rows * pitch_out, SENTINEL, dtype=np.uint32))
    block = np.empty((ni, pitch_in, 2), dtype=dt)
    start = z.position(0)
    pos = 0
    for cut in cuts:
        block[:, cut:] = 1.0 if dt == np.float32 else np.iinfo(dt).max
        for s in range(ni):
            block[s, :cut] = rows[s][pos:pos + cut]
        d_in.upload(block)
        assert z.resident(d_in, pitch_in, cut, d_out, pitch_out, out_first + pos // D) == cut // D
        pos += cut
    assert z.position(ni - 1) == (start[0] + n, start[1] + n // D)
    words = d_out.download(n_rows * pitch_out * 4, dtype=np.uint32).reshape(n_rows, pitch_out)
    d_in.free(); d_out.free()
    assert np.all(words[:, :out_first] == SENTINEL) and np.all(words[:, out_first + n // D:] == SENTINEL), "words outside the span were written"
    return np.ascontiguousarray(words[:, out_first:out_first + n // D]).view(np.int16).reshape(n_rows, n // D, 2)


def _first_difference(got, want):
    return int(np.argmax(np.any(got != want, axis=1)))


def _same(got, want, what):
    """got [rows, n, 2] against want: a list, per input, of [zooms, n, 2]."""
    flat = [w for per_input in want for w in per_input]
    assert len(flat) == len(got), what
    for r, w in enumerate(flat):
        assert got[r].shape == w.shape and np.array_equal(got[r], w), (what, r, _first_difference(got[r], w))
