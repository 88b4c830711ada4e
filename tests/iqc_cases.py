"""The IQ corrector's cases, shared by tests/test_iqc.py (CPU), tests/test_gpu_iqc.py and tests/test_gpu_iqc_edges.py: two stations at mirrored
frequencies of one 252 kS/s stream -- 518 strong at +14 kHz, 490 weak under noise at -14 kHz -- the impairment of a zero-IF
radio (gain, phase, DC offset), and a noise-free tone on an FFT bin.  Nothing is kept: a row is 24 MB, and a test that wants
several at once holds them itself for as long as it runs.  Behind them a model of where a call's tiles meet the ends of blocks,
and the cut plan of the block-end sweep, whose coverage tests/test_iqc.py asserts without a GPU."""
from __future__ import annotations

import numpy as np

import iqc_ref as ir
import resample_ref as rr
import signals

SEEDS = tuple(range(11, 23))
RATE = 252000
TEXT_518, TEXT_490 = 3, 7
AMP_518, AMP_490, NOISE = 8000, 300, 1500
BIT_OFFSET_490 = 1234
GAIN, PHASE_DEG, DC_I, DC_Q = 1.05, 3.0, 300, -200
TONE_BIN, TONE_AMP = 3641, 8000


def texts():
    return signals.stream_text(TEXT_518), signals.stream_text(TEXT_490)


def rows(nv, seed: int, amp_490: float = AMP_490, noise: float = NOISE) -> np.ndarray:
    """The clean row as int16 [n, 2], n whole frames: the two stations and uniform noise."""
    bits = [nv.sitor_encode(t, 40) for t in texts()]
    n = (max(len(b) for b in bits) + 300) * 2520 // nv.FRAME_IN * nv.FRAME_IN
    a = rr.cpfsk(bits[0], RATE, n, freq_hz=14000, amplitude=AMP_518, noise_amp=0, seed=seed).astype(np.int32)
    a += rr.cpfsk(bits[1], RATE, n, freq_hz=-14000, amplitude=amp_490, noise_amp=noise, seed=seed, bit_offset=BIT_OFFSET_490)
    return np.clip(a, -32768, 32767).astype(np.int16)


def impair(x: np.ndarray) -> np.ndarray:
    """I' = I + 300, Q' = 1.05 (Q cos 3 deg + I sin 3 deg) - 200, rounded and clipped."""
    ph = np.deg2rad(PHASE_DEG)
    i, q = x[:, 0].astype(np.float64), x[:, 1].astype(np.float64)
    y = np.stack([i + DC_I, GAIN * (q * np.cos(ph) + i * np.sin(ph)) + DC_Q], axis=1)
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)


def tone(n: int) -> np.ndarray:
    """A noise-free tone on bin TONE_BIN of a 65 536-point FFT, as int16 [n, 2]."""
    ph = 2 * np.pi * ((TONE_BIN * np.arange(n, dtype=np.int64)) % 65536) / 65536.0
    return np.rint(TONE_AMP * np.stack([np.cos(ph), np.sin(ph)], axis=1)).astype(np.int16)


def image_dbc(block: np.ndarray) -> float:
    """The image of the tone in a block of 65 536 samples (Hann window), in dB against the tone."""
    z = (block[:, 0].astype(np.float64) + 1j * block[:, 1].astype(np.float64)) * np.hanning(65536)
    f = np.abs(np.fft.fft(z))
    peak = lambda k: f[[(k - 1) % 65536, k, (k + 1) % 65536]].max()      # noqa: E731
    return float(20 * np.log10(max(peak(65536 - TONE_BIN), 1e-9) / peak(TONE_BIN)))


def delivered(oracle, iq252: np.ndarray, frame_in: int):
    """({518: [texts], 490: [texts]} the oracle's two chains decode from a row at 252 kS/s, and (bits of 518, bits of 490)."""
    ref = oracle.Pipe(chain_mask=3)
    ref.push(iq252[:len(iq252) // frame_in * frame_in])
    return {f: [m[2] for m in ref.messages if m[0] == f] for f in (518, 490)}, (ref.bits(0), ref.bits(1))


# ------------------------------------------------------------------------------------------ rows for the restatement's edges
def impaired_noise(n: int, seed: int, amp: int = 6000) -> np.ndarray:
    """Uniform noise whose level changes every 50 000 samples, through impair(): every window solves to other coefficients."""
    rng = np.random.default_rng(seed)
    level = rng.uniform(0.3, 1.0, size=n // 50000 + 1)[np.arange(n) // 50000]
    x = rng.uniform(-amp, amp, size=(n, 2)) * level[:, None]
    return impair(np.rint(x).astype(np.int16))


def silence_with_dc(n: int) -> np.ndarray:
    """(300, -200) throughout: reason 1, with the offset removed all the same."""
    return np.tile(np.array([[DC_I, DC_Q]], dtype=np.int16), (n, 1))


def q_equals_i(n: int, seed: int) -> np.ndarray:
    """Q = I: the coherence is 1, reason 2."""
    i = np.random.default_rng(seed).integers(-5000, 5001, size=n).astype(np.int16)
    return np.stack([i, i], axis=1)


def q_three_i_rotated(n: int, seed: int) -> np.ndarray:
    """Q at three times the level of I and all but independent of it: step 7 passes (|a| is about 0.15), step 9 finds g near
    1/3: reason 4."""
    rng = np.random.default_rng(seed)
    i, j = rng.integers(-3000, 3001, size=n), rng.integers(-3000, 3001, size=n)
    return np.stack([i, np.rint(3 * (0.05 * i + j))], axis=1).astype(np.int16)


def rails(n: int, alternating: bool) -> np.ndarray:
    """Every sample at (-32768, -32768), or the rails alternating in sign: I every sample, Q every third."""
    x = np.full((n, 2), -32768, dtype=np.int16)
    if alternating:
        x[1::2, 0] = 32767
        x[(np.arange(n) // 3) % 2 == 1, 1] = 32767
    return x


def _extremes(fmt, n, seed):
    """Three rows in format fmt: every sample at the lowest value, the rails alternating in sign, and full-scale random."""
    dt = rr.DTYPES[fmt]
    rng = np.random.default_rng(seed)
    if fmt == ir.CF32:
        lo, hi = np.float32(-1.0), np.float32(32767.0 / 32768.0)
        rnd = rng.uniform(-1.3, 1.3, size=(n, 2)).astype(np.float32)
        special = np.array([np.nan, np.inf, -np.inf, 1e-42, -1e-42, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768,
                            32766.5 / 32768, 32767.5 / 32768, -32768.5 / 32768, 1.0, -1.0, 3e38, -3e38, 0.0, -0.0, 123.5 / 32768], dtype=np.float32)
        at = rng.integers(0, n, size=(400, 2))
        rnd[at[:, 0], at[:, 1] % 2] = special[rng.integers(0, len(special), size=400)]
        rnd[:len(special), 0] = special
    else:
        lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
        rnd = rng.integers(int(lo), int(hi) + 1, size=(n, 2)).astype(dt)
    low = np.full((n, 2), lo, dtype=dt)
    alt = low.copy()
    alt[1::2, 0] = hi
    alt[(np.arange(n) // 3) % 2 == 1, 1] = hi
    return [low, alt, rnd]


def q_fifth_of_i(n: int, seed: int) -> np.ndarray:
    """I = 5 i, Q = i: the coherence passes step 7 (a is -1/5), and what is left of Q behind it is nothing: v <= 0, reason 3."""
    i = np.random.default_rng(seed).integers(-6000, 6001, size=n)
    return np.stack([5 * i, i], axis=1).astype(np.int16)


# --------------------------------------------------------------------------- where a call's tiles meet the ends of blocks
BLOCK, TILE = 65536, 4096


def block_ends_in_tiles(position: int, n_in: int) -> list:
    """From the header's blocks (65 536 samples, counted from the stream's reset) and the kernels' tiles (4096 samples,
    counted from the call's first sample): for every tile of a call of n_in samples at `position` in which a block ends
    with samples of the call behind it, (n_a, whole) -- the tile's samples in front of that end, and whether all 4096
    samples of the tile belong to the call."""
    off0 = position % BLOCK
    ends = []
    for tbase in range(0, n_in, TILE):
        boff = off0 + tbase
        n_a = BLOCK - (boff & (BLOCK - 1))
        if n_a < TILE and tbase + n_a < n_in:
            ends.append((n_a, tbase + TILE <= n_in))
    return ends


# The block-end sweep: every n_a the kernels treat differently -- the first and last samples of a tile, of a lane's group of 4 or
# 8, of a step of 256 or 512, of a wave's region of 1024, and both sides of each.
SWEEP_N_A = (1, 3, 4, 255, 256, 257, 512, 1023, 1024, 1025, 1028, 1536, 2047, 2048, 2049, 2052, 2560, 3071, 3072, 3073, 3583, 4088, 4092, 4095)
# the visits that end the call d samples behind the block's end, in the same tile: {n_a: d}
SWEEP_SHORT = {255: 1, 257: 5, 1023: 1, 1025: 90, 2049: 5, 3073: 90, 4088: 5}
# the visits whose call ends on the block's end (no split: the block behind belongs to the next call), by the visit they follow
SWEEP_EXACT = {4: 1024, 257: 256, 1028: 3, 2049: 2048, 3073: 4095, 4092: 3583}
SWEEP_FIRST_END = 5                                            # the first block whose end is visited: blocks 0 .. 3 fill W = 4


def sweep_cuts():
    """The call lengths of the sweep, from position 0: block ends SWEEP_FIRST_END, SWEEP_FIRST_END + 1, ... are visited one
    after the other.  A visit (n_a, t) starts a call at E - 4096 t - n_a, E the block's end, so that E lies n_a samples into
    the call's tile t; t cycles through 0, 1 and 2.  The call runs on to the start of the next visit, or ends d samples
    behind E, or on E."""
    visits = []
    for n_a in SWEEP_N_A:
        visits.append((n_a, SWEEP_SHORT.get(n_a)))
        if n_a in SWEEP_EXACT:
            visits.append((SWEEP_EXACT[n_a], 0))
    cuts, pos = [], 0
    for k, (n_a, d) in enumerate(visits):
        end = (SWEEP_FIRST_END + k) * BLOCK
        start = end - TILE * (k % 3) - n_a
        cuts.append(start - pos)                               # up to the visit: no block ends in it behind the call's first tile
        pos = start
        if d is not None:
            cuts.append(end + d - pos)
            pos = end + d
    cuts.append((SWEEP_FIRST_END + len(visits)) * BLOCK + 777 - pos)
    return cuts


def sweep_coverage(cuts, position: int = 0):
    """What a cut plan reaches, by block_ends_in_tiles: (the n_a of every split, those of the splits in a tile that is not
    whole, the calls that end on a block's end having started inside a block)."""
    splits, ragged, exact = [], [], 0
    for cut in cuts:
        for n_a, whole in block_ends_in_tiles(position, cut):
            splits.append(n_a)
            if not whole:
                ragged.append(n_a)
        exact += cut > 0 and position % BLOCK != 0 and (position + cut) % BLOCK == 0
        position += cut
    return splits, ragged, exact


def sweep_rows(fmt: int) -> list:
    """The sweep's two streams in format fmt: impaired noise, for which every window solves to other coefficients, so that a
    sample given the wrong side's shows in the output; and full-scale random input (float32 specials), in which a sample
    added to the wrong block changes the sums and the solves behind them."""
    n = sum(sweep_cuts())
    gain = 3.0 if fmt in (rr.CU8, rr.CS8) else 1.0
    return [rr.to_format(impaired_noise(n, 900 + fmt), fmt, gain=gain), _extremes(fmt, n, 910 + fmt)[2]]
