"""The real-input converter's cases, shared by tests/test_real.py (CPU), tests/test_gpu_real.py and
tests/test_gpu_real_edges.py: the real row of a
direct-sampling receiver at 504 kS/s with two stations -- 518 strong at 140 kHz, 490 weak under noise at 112 kHz, which the
converter puts at +-14 kHz of a 252 kS/s stream --, what a user without the converter would do with it (naive), the same two
stations built directly as complex (the reference row), tones on FFT bins, the rails, and full-scale random rows.  Nothing
is kept: a test that wants several rows at once holds them itself for as long as it runs.  Behind them what the two GPU files
share: the call lengths of the vector-store case and where the kernel's lanes stand at their ends (end_of_call), and the
resident call under sentinels (_run_resident, _same, _first_difference)."""
from __future__ import annotations

import numpy as np

import iqc_cases as ic
import real_ref as rf
import resample_ref as rr

SEEDS = ic.SEEDS
RATE = 504000                             # of the real row; the converted row has ic.RATE = 252 000
F_518, F_490 = 140000, 112000             # RATE / 4 + 14 kHz and - 14 kHz
AMP_518, AMP_490 = ic.AMP_518, ic.AMP_490
BIT_OFFSET_490 = ic.BIT_OFFSET_490
# Uniform noise of +-NOISE on the real samples.  The rule: start at iqc_cases' 1500 and lower it in steps of 250 until the
# reference row delivers the 490 message from twelve seeds of twelve; 1500 does (tests/test_real.py holds it to that).
NOISE = 1500
TONE_OUTPUTS, TONE_AMP = 16384, 20000
TONE_BINS = (37, -1000, 2600, -4099, 6553, -6553)          # of 16 384 outputs; the inner 80 % of the band ends at +-6553


texts = ic.texts


def real_row(nv, seed: int, noise: float = NOISE) -> np.ndarray:
    """int16 [2 n], n whole frames of 252 kS/s: the I column of the two stations' sum at 504 kS/s."""
    bits = [nv.sitor_encode(t, 40) for t in texts()]
    n = (max(len(b) for b in bits) + 300) * 2520 // nv.FRAME_IN * nv.FRAME_IN
    a = rr.cpfsk(bits[0], RATE, 2 * n, freq_hz=F_518, amplitude=AMP_518, noise_amp=0, seed=seed)[:, 0].astype(np.int32)
    a += rr.cpfsk(bits[1], RATE, 2 * n, freq_hz=F_490, amplitude=AMP_490, noise_amp=noise, seed=seed, bit_offset=BIT_OFFSET_490)[:, 0]
    return np.clip(a, -32768, 32767).astype(np.int16)


def reference_row(nv, seed: int, noise: float = NOISE) -> np.ndarray:
    """The same two stations built directly as complex at 252 kS/s and +-14 kHz: int16 [n, 2]."""
    return ic.rows(nv, seed, noise=noise)


def naive(x: np.ndarray, fmt: int = rf.S16) -> np.ndarray:
    """The same shift and decimation with Q = 0: int16 [n // 2, 2].  Without the Q branch nothing tells +d from -d."""
    e = rf.convert(x, fmt)[0::2][:len(x) // 2]
    m = np.arange(len(e))
    d = np.concatenate([np.zeros(rf.K, dtype=np.int64), e])[:len(e)]            # e[m - K]
    s = np.where((m - rf.K) % 2 == 0, 1, -1)
    return np.stack([rf.clamp16(s * d), np.zeros(len(e), dtype=np.int64)], axis=1).astype(np.int16)


delivered = ic.delivered


# ---------------------------------------------------------------------------------------------------------------- edges
def tone(b: int, outputs: int = TONE_OUTPUTS, amp: float = TONE_AMP, lead: int = 64) -> np.ndarray:
    """A real tone that comes out on bin b of an FFT over `outputs` outputs: input frequency 1/4 + b / (2 outputs) of the
    rate, 2 (lead + outputs) samples as int16 (the first `lead` outputs are the filter filling)."""
    k = np.arange(2 * (lead + outputs), dtype=np.int64)
    turns = ((outputs // 2 + b) * k) % (2 * outputs)
    return np.rint(amp * np.cos(2 * np.pi * turns / (2.0 * outputs))).astype(np.int16)


def tone_levels(iq: np.ndarray, b: int, amp: float = TONE_AMP):
    """(gain in dB against a complex tone of amplitude amp, image in dBc) of the last len - lead outputs, Blackman window."""
    n = TONE_OUTPUTS
    z = (iq[-n:, 0].astype(np.float64) + 1j * iq[-n:, 1].astype(np.float64))
    w = np.blackman(n)
    f = np.abs(np.fft.fft(z * w))
    return float(20 * np.log10(f[b % n] / (amp * w.sum()))), float(20 * np.log10(max(f[-b % n], 1e-9) / f[b % n]))


def rails_low(n: int) -> np.ndarray:
    """Every sample at -32768: I clamps at +32767 on every other output, the Q sum is zero."""
    return np.full(n, -32768, dtype=np.int16)


def rails_step(n: int, half_period: int = 40) -> np.ndarray:
    """Even samples at -32768; odd samples 40 at 32767, 40 at -32768, alternately: where the odd samples step down every
    difference o[m-K-1-j] - o[m-K+j] is +65535 and acc = +18610 * 65535, where they step up it is the negative."""
    x = np.full(n, -32768, dtype=np.int16)
    o = np.where((np.arange(n // 2) // half_period) % 2 == 0, 32767, -32768)
    x[1::2] = o[:len(x[1::2])]
    return x


def full_scale(fmt: int, n: int, seed: int) -> np.ndarray:
    """Full-scale random samples in format fmt; float32 with the specials of the CF32 rule."""
    rng = np.random.default_rng(seed)
    if fmt != rf.F32:
        info = np.iinfo(rf.DTYPES[fmt])
        return rng.integers(info.min, info.max + 1, size=n).astype(rf.DTYPES[fmt])
    x = rng.uniform(-1.3, 1.3, size=n).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 1e-42, -1e-42, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768,
                        32766.5 / 32768, 32767.5 / 32768, -32768.5 / 32768, 1.0, -1.0, 3e38, -3e38, 0.0, -0.0, 123.5 / 32768], dtype=np.float32)
    x[rng.integers(0, n, size=min(400, n))] = special[rng.integers(0, len(special), size=min(400, n))]
    x[:len(special)] = special
    return x


def signal(fmt: int, n: int, seed: int) -> np.ndarray:
    """A few tones and noise in format fmt: rows for the cut and format cases."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    a = 9000 * np.cos(2 * np.pi * 0.27 * k + seed) + 4000 * np.cos(2 * np.pi * 0.113 * k) + rng.uniform(-3000, 3000, size=n)
    a16 = np.rint(a).astype(np.int16)
    if fmt == rf.S16:
        return a16
    if fmt == rf.U8:
        return np.clip(np.rint(a16 / 128.0 + 127.5), 0, 255).astype(np.uint8)
    if fmt == rf.S8:
        return np.clip(np.rint(a16 / 128.0), -128, 127).astype(np.int8)
    return (a16 / 32768.0).astype(np.float32)


# ------------------------------------------------------------------------------------------- the vector stores (GPU edges)
TILE, REGION = 4096, 1024                 # outputs of a tile, and of the region of it a wave loads
# outputs of a call: the last pair in wave 2, inside a lane's group of either width and three words into a store group; and a
# multiple of 4 that is none of 8: the bytes' group of 8 pairs is cut, the store group whole
VEC_OUTPUTS = (2 * TILE + 2967, 2 * TILE + 1028)
VEC_CUT = TILE + 1001                     # an odd number of pairs: the call behind it starts on a word that is not 16-byte aligned
VEC_STREAMS = 3


def end_of_call(n: int, spt: int):
    """Where the kernel's loads meet the end of a call of n outputs, from the kernel's layout (a wave loads a region of 1024
    pairs of the tile in steps of 64 lanes x spt pairs; spt = 4, or 8 for the 8-bit formats): (wave, step, lane) of the group
    the last pair lies in, the pairs of that group inside the call, and the words of the last store group of 4 inside it."""
    last = (n - 1) % TILE
    wave, r = divmod(last, REGION)
    step, r = divmod(r, 64 * spt)
    lane, k = divmod(r, spt)
    return (wave, step, lane), k + 1, (n - 1) % 4 + 1


def vec_rows(fmt: int, n_out: int) -> list:
    """The rows of the vector-store case: VEC_STREAMS x 2 n_out samples, a seed each.  The last pair of the row, and of a
    first call of VEC_CUT pairs, stands at the format's lowest value: within its call the pair's odd sample reaches the
    call's last output alone, through the tap of weight 1, and only half of full scale and more is sure to move it."""
    rows = [signal(fmt, 2 * n_out, 300 + 10 * fmt + s) for s in range(VEC_STREAMS)]
    low = np.float32(-1.0) if fmt == rf.F32 else np.iinfo(rf.DTYPES[fmt]).min
    for row in rows:
        row[2 * VEC_CUT - 2:2 * VEC_CUT] = low
        row[-2:] = low
    return rows


# ------------------------------------------------------------------------------------------------ the resident call (GPU)
SENTINEL = 0x5a5a1234


def _run_resident(nv, c, rows, cuts, pitch_extra=0, out_first=0, aligned=None):
    """The rows ([n] samples each, all of one length) through nvx_real_resident in calls of `cuts` samples (even); every call's
    input is uploaded to the start of the input rows as whole rows: behind a call's n_in samples the row is full scale up to
    the pitch, so a read behind n_in changes the output.  Sentinels around every output row.  `aligned`, one flag per call: the
    call's first output word of every row is (or is not) 16-byte aligned, which is what chooses between the 16-byte and the
    word-by-word stores.  Returns int16 [streams, n / 2, 2]."""
    ns, n = len(rows), len(rows[0])
    assert sum(cuts) == n and ns == c.n_streams and n % 2 == 0
    dt = rows[0].dtype
    pitch_out = out_first + n // 2 + pitch_extra
    pitch_in = (max(max(cuts), 1) + 15) // 16 * 16 + 16 * pitch_extra
    d_in = nv.DeviceBuffer(ns * pitch_in * dt.itemsize)
    d_out = nv.DeviceBuffer(ns * pitch_out * 4)
    d_out.upload(np.full(ns * pitch_out, SENTINEL, dtype=np.uint32))
    block = np.empty((ns, pitch_in), dtype=dt)
    start = c.position(0)
    pos = 0
    for call, cut in enumerate(cuts):
        block[:, cut:] = 1.0 if dt == np.float32 else np.iinfo(dt).max
        for s in range(ns):
            block[s, :cut] = rows[s][pos:pos + cut]
        d_in.upload(block)
        if aligned is not None:
            assert ((d_out.ptr + 4 * (out_first + pos // 2)) % 16 == 0 and pitch_out % 4 == 0) == aligned[call], (call, out_first, pos, pitch_out)
        c.resident(d_in, pitch_in, cut, d_out, pitch_out, out_first + pos // 2)
        pos += cut
    assert c.position(ns - 1) == (start[0] + n, start[1] + n // 2)
    words = d_out.download(ns * pitch_out * 4, dtype=np.uint32).reshape(ns, pitch_out)
    d_in.free(); d_out.free()
    assert np.all(words[:, :out_first] == SENTINEL) and np.all(words[:, out_first + n // 2:] == SENTINEL), "words outside the span were written"
    return np.ascontiguousarray(words[:, out_first:out_first + n // 2]).view(np.int16).reshape(ns, n // 2, 2)


def _first_difference(got, want):
    return int(np.argmax(np.any(got != want, axis=1)))


def _same(got, want, what):
    for s in range(len(want)):
        assert got[s].shape == want[s].shape and np.array_equal(got[s], want[s]), (what, s, _first_difference(got[s], want[s]))
