"""Restatement of the impulse noise blanker (include/navtex_amd_blank.h), written from the header's contract, not from the
kernel: the resampler's input conversions (tests/resample_ref.py), magnitudes, block sums by absolute index, the level from
the minimum of the last four, detection, hold, and the counters -- in int64 numpy, with the carried state of the header so
that a stream can be cut into calls anywhere.  blank_streams is the same for many equal rows at once.  Behind it the inputs
of tests/test_gpu_blank_edges.py, built by magnitude so that every sum, level and probe is exact in every format; the
properties they are built for are asserted on the restatement in tests/test_blank.py."""
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


# ------------------------------------------------------------------------------------------------ many rows at once
def blank_streams(rows, fmt: int = CS16, thr_q8: int = THR_DEFAULT, hold: int = HOLD_DEFAULT, floor: int = FLOOR_DEFAULT, position: int = 0,
                  batch: int = 1 << 22):
    """Equal-length rows [R, n, 2] in format fmt, each a stream that starts at `position` with nothing in front of it, in one
    call: (int16 [R, n, 2], detections [R], blanked [R]) -- Blanker's words and counters, vectorised along the row axis and
    walked in batches of about `batch` samples, so that the temporaries stay bounded.  int32 throughout: a block's sum is at
    most 2^26, and a call is shorter than 2^30 samples."""
    rows = np.asarray(rows)
    R, n = rows.shape[:2]
    assert rows.shape[2:] == (2,) and 0 < n < (1 << 30) and (thr_q8 == 0 or 256 <= thr_q8 <= 4096) and 0 <= hold <= 1024 and 0 <= floor <= 65535
    out = np.empty((R, n, 2), dtype=np.int16)
    detections, blanked = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    idx = np.arange(n, dtype=np.int32)
    b = (position % NB + idx) // NB                           # the block of the call a sample lies in; block 0 is the reset's
    nb = int(b[-1]) + 1
    starts = np.flatnonzero(np.r_[True, b[1:] != b[:-1]])
    step = max(1, batch // n)
    for r0 in range(0, R, step):
        x = rr.convert(rows[r0:r0 + step].reshape(-1, 2), fmt).astype(np.int32).reshape(-1, n, 2)
        m = np.abs(x[:, :, 0]) + np.abs(x[:, :, 1])
        level = np.full((len(x), nb), -1, dtype=np.int64)     # -1: nothing is detected in that block
        if thr_q8 and nb > 4:
            s = np.add.reduceat(m, starts, axis=1, dtype=np.int64)
            ref = np.lib.stride_tricks.sliding_window_view(s, 4, axis=1).min(axis=2)[:, :nb - 4]      # of blocks k - 4 .. k - 1, for k >= 4
            level[:, 4:] = np.maximum((thr_q8 * (ref >> 10)) >> 8, floor)
        lv = level[:, b]
        d = (lv >= 0) & (m > lv)
        latest = np.maximum.accumulate(np.where(d, idx, np.int32(-(1 << 30))), axis=1)
        gone = idx - latest <= hold
        out[r0:r0 + step] = np.where(gone[:, :, None], 0, x)
        detections[r0:r0 + step] = d.sum(axis=1)
        blanked[r0:r0 + step] = gone.sum(axis=1)
    return out, detections, blanked


# --------------------------------------------------------------------------------------- inputs built by magnitude
TILE = 4 * NB
SPT = {CS16: 4, CU8: 8, CS8: 8, CF32: 4}                     # samples per lane and step of the kernel; a step is 64 of them


def unit(fmt: int) -> int:
    """The step of the magnitudes a format can carry (CU8's smallest is one unit, the others' zero)."""
    return 256 if fmt in (CU8, CS8) else 1


def samples_of(fmt: int, m, rng) -> np.ndarray:
    """Samples [n, 2] in format fmt whose converted |I| + |Q| is m exactly, split between I and Q and signed by rng.  m is a
    multiple of unit(fmt); at most 65 534 (16-bit, float32), 65 024 (CS8), 65 280 (CU8, and at least 256)."""
    m = np.asarray(m, dtype=np.int64)
    sign = 1 - 2 * rng.integers(0, 2, size=(len(m), 2))
    if fmt in (CS16, CF32):
        assert m.min() >= 0 and m.max() <= 65534
        a = np.clip(rng.integers(0, m + 1), m - 32767, 32767)
        x = np.stack([a, m - a], axis=1) * sign
        return x.astype(np.int16) if fmt == CS16 else (x / 32768.0).astype(np.float32)
    t = m // 256
    assert not (m % 256).any()
    if fmt == CS8:
        assert t.min() >= 0 and t.max() <= 254
        a = np.clip(rng.integers(0, t + 1), t - 127, 127)
        return (np.stack([a, t - a], axis=1) * sign).astype(np.int8)
    assert t.min() >= 1 and t.max() <= 255                   # (2u - 255) * 128: odd multiples of 128, two of them make 256 t
    a = 2 * np.clip(rng.integers(1, t + 1), np.maximum(1, t - 127), 128) - 1
    return ((255 + np.stack([a, 2 * t - a], axis=1) * sign) // 2).astype(np.uint8)


def _noise_m(fmt, rng, lo, hi, size):
    u = unit(fmt)
    return rng.integers(-(-lo // u), hi // u + 1, size=size) * u


def _fill_to(fmt, rng, M, free, total):
    """The samples M[free] (indices) get magnitudes about equal, jittered in pairs, whose sum is `total` exactly."""
    u, F = unit(fmt), len(free)
    assert total % u == 0 and total >= 0 and F > 0
    q, r = divmod(total // u, F)
    assert q >= (1 if fmt == CU8 else 0), "the block cannot be that quiet"
    v = np.full(F, q, dtype=np.int64)
    v[:r] += 1
    j = rng.integers(0, q // 4 + 1, size=F // 2)
    v[:F // 2] += j; v[F // 2:2 * (F // 2)] -= j
    M[free] = rng.permutation(v) * u


# ---- (a) form 2: what a later chunk's pre-roll has to carry
FORM2_N2, FORM2_N3 = 64 * TILE + 5, 3000
SPIKE_M, BURST_M, BURST_LEN = 51200, 20480, 20
RING_MEANS = (1024, 1600, 2200, 2800)                        # of the four blocks a probed block's level comes from
RING_PROBE = 5120                                            # above the level 1024 gives (4096), below the one 1600 would give (6400)


def form2_trap_row(fmt: int, first: int, hold: int, stream: int, slots, seed: int):
    """One stream of first + 64 * 4096 + 5 + 3000 samples for calls of just these lengths at the default threshold and
    floor: the second call's later chunks start at C = first + 32 * 4096 and first + 64 * 4096, off = 1024 - first % 1024
    samples in front of a block end.  Around each C (E = C + off - 1024 is where the block B0 that holds C opens, Bj the
    block j further on):
      1. a single spike at C - hold, the only detection whose hold reaches C: C goes, C + 1 stays;
      2. the four blocks in front of the probed block P (B0 where at least 64 of its samples lie behind C, else B1) have
         the sums 1024 * RING_MEANS exactly, the smallest in ring slot slots[chunk] (0: oldest); two samples of P at
         RING_PROBE are detections by that minimum alone;
      3. B0 is quiet in front of C and loud behind it.  Where one sample lies in front (off = 1023), its sum is 1024 * 768
         exactly and the smallest of B2's ring: two samples of B2 at the level 3072 are no detections, and are with one
         unit less in the sum.  Where 1017 or 1023 do, a sum without them sends the levels of B1 .. B4 to the floor;
      4. bursts of 20 samples in the first seven regions of the pre-roll and a loud block B-6.
    Returns (samples [n, 2] in fmt, info): info['starts'] the two C, info['det'] the detections the design means (bool
    [n]), info['probes'] the samples of trap 2, info['quiet'] those of trap 3 (not detected), info['blocks0'] the two E."""
    rng = np.random.default_rng(seed)
    u = unit(fmt)
    n = first + FORM2_N2 + FORM2_N3
    off = NB - first % NB
    M = _noise_m(fmt, rng, 512, 2560, n)
    det = np.zeros(n, dtype=bool)
    info = {"starts": [], "probes": [], "quiet": [], "blocks0": [], "off": off}
    for chunk, c in enumerate((32 * TILE, 64 * TILE)):
        C = first + c
        E = C + off - NB
        fixed = np.zeros(n, dtype=bool)

        def put(at, m, detected):
            M[at] = m; fixed[at] = True
            if detected is not None:
                det[at] = detected
        loud = np.arange(E - 6 * NB, E - 5 * NB)
        put(loud, _noise_m(fmt, rng, 15360, 25600, NB), True)
        for r in range(7):
            at = C - 2 * TILE + NB * r + 300 + 100 * stream
            put(np.arange(at, at + BURST_LEN), BURST_M, True)
        behind = np.arange(C, min(E + NB, C + 7))            # B0 behind C: loud, a few fixed samples where it is short
        if off < NB:
            put(behind, 3072, None)
        put(C - hold, SPIKE_M, True)
        p_block = 0 if off >= 64 else 1
        probes = E + NB * p_block + np.array([200, 600])
        put(probes, RING_PROBE, True)
        quiet = E + 2 * NB + np.array([400, 700])
        if off == NB - 1:
            put(quiet, 4 * 768, False)
            info["quiet"] += quiet.tolist()
        # the sums: the ring of P with its smallest in the slot asked for, the blocks around it
        means = {j: 1500 for j in range(-4, 4)}
        ring = [m for m in RING_MEANS[1:]]
        ring.insert(slots[chunk], RING_MEANS[0])
        for k in range(4):
            means[p_block - 4 + k] = ring[k]
        if p_block == 0:
            means[0], means[1] = 768, 1800
        else:
            means[-4], means[1] = 2000, 1800
        for j in range(-4, 4):
            lo, hi = E + NB * j, E + NB * (j + 1)
            if hi > n:
                continue
            free = lo + np.flatnonzero(~fixed[lo:hi])
            if j == 0 and 1 < off < NB and p_block == 0:     # one quiet sample in front (off = 1023)
                M[C - 1] = u; fixed[C - 1] = True
                free = free[free != C - 1]
            _fill_to(fmt, rng, M, free, means[j] * NB - int(M[lo:hi][fixed[lo:hi]].sum()))
            assert int(M[lo:hi].sum()) == means[j] * NB
        info["starts"].append(C); info["blocks0"].append(E); info["probes"] += probes.tolist()
    info["det"] = det
    return samples_of(fmt, M, rng), info


def form2_trap_rows(fmt: int, first: int, hold: int, cell: int):
    """Two streams of form2_trap_row; the smallest ring sum sits in slot (2 * stream + chunk + cell) % 4, so the four
    (stream, chunk) pairs of a cell cover the four slots.  Returns (rows, infos, slots)."""
    slots = [[(2 * s + chunk + cell) % 4 for chunk in range(2)] for s in range(2)]
    made = [form2_trap_row(fmt, first, hold, s, slots[s], 1000 * cell + 10 * fmt + s) for s in range(2)]
    return [m[0] for m in made], [m[1] for m in made], slots


FORM2_PHASES = (4096 + 1023, 4096, 4096 + 1, 4096 + 1017)       # `first`: off = 1, 1024, 1023, 7


def form2_cells():
    """(fmt, first, hold, out_first) of every cell of case a, in order; a cell's index seeds it and turns its slots."""
    cells = [(fmt, first, 1024, 0) for fmt in (CS16, CU8, CS8, CF32) for first in FORM2_PHASES]
    cells += [(fmt, first, hold, 0) for fmt in (CS16, CU8) for first in FORM2_PHASES[:2] for hold in (0, 32)]
    cells += [(CS16, FORM2_PHASES[2], 1024, 5), (CU8, FORM2_PHASES[3], 32, 1), (CS8, FORM2_PHASES[0], 1024, 3), (CF32, FORM2_PHASES[1], 0, 7)]
    return cells


# ---- (c) single spikes at every boundary of the kernel's walk
SPIKE_OFF = 517                                              # samples from a region's start to the block end in it
SPIKE_FIRST = 5 * NB + NB - SPIKE_OFF                        # the warm-up call in front: five blocks and a part
SPIKE_HOLDS = (0, 1, 3, 4, 7, 8, 31, 255, 256, 257, 511, 512, 1023, 1024)


def spike_offsets(fmt: int):
    """Tile offsets of the spikes: lane, row, broadcast, step, region and tile seams and both sides of the block end."""
    spt = SPT[fmt]
    step = 64 * spt
    return sorted({0, 1, spt - 1, spt, 16 * spt - 1, 16 * spt, 32 * spt, 48 * spt, step - 1, step, NB - 1, NB, TILE - 1, TILE, SPIKE_OFF - 1, SPIKE_OFF})


def spike_row(fmt: int, seed: int):
    """CS16 or CU8: noise of |I|, |Q| <= 200; a warm-up call of SPIKE_FIRST samples, then one call with spike j at its
    sample (2 + j) * 4096 + the j-th tile offset (a tile and more apart) and a ragged last tile.  Returns (the samples of
    both calls, the spikes' samples in them)."""
    rng = np.random.default_rng(seed)
    offs = spike_offsets(fmt)
    at = SPIKE_FIRST + np.array([(2 + j) * TILE + o for j, o in enumerate(offs)])
    n = SPIKE_FIRST + (len(offs) + 4) * TILE - 37
    assert np.diff(at).min() > 2 * NB + 64 and at[-1] + NB < n and n - SPIKE_FIRST <= 32 * TILE
    if fmt == CS16:
        x = rng.integers(-200, 201, size=(n, 2)).astype(np.int16)
        x[at] = (30000, -30000)
    else:
        assert fmt == CU8
        x = rng.integers(127, 129, size=(n, 2)).astype(np.uint8)
        x[at] = (255, 0)
    return x, at


# ---- (d) the level's arithmetic on blocks of constant magnitude
def word_of(m: int, negative: bool = False):
    """A CS16 sample of magnitude m <= 65 536."""
    assert 0 <= m <= 65536
    if m <= 32767 and not negative:
        return (m, 0)
    return (-min(m, 32768), -(m - min(m, 32768)))


def level_row(position: int, thr_q8: int, floor: int, blocks):
    """CS16, for hold = 0: a stream that starts at `position`; block k of it (the one `position` lies in is block 0) holds
    I = +-c, Q = 0 for blocks[k] = (c, extra, probe): `extra` is added to the magnitude of one sample, and with `probe` a
    full block behind the first four carries a sample at the level and one at the level + 1 (where that is a magnitude).
    The sums are kept in Python integers as the row is written, so every probe is exact by construction.  Returns
    (int16 [n, 2], at_level, above): the probes' samples."""
    rng = np.random.default_rng(position + thr_q8 + floor)
    p0 = position % NB
    n = len(blocks) * NB - p0
    x = np.zeros((n, 2), dtype=np.int16)
    sums, at_level, above = [], [], []
    for k, (c, extra, probe) in enumerate(blocks):
        lo, hi = max(k * NB - p0, 0), (k + 1) * NB - p0
        x[lo:hi, 0] = c * (1 - 2 * rng.integers(0, 2, size=hi - lo)) if c <= 32767 else -32768
        x[lo:hi, 1] = 0 if c <= 32768 else -(c - 32768)
        s = c * (hi - lo)
        if extra:
            x[lo + 5] = word_of(c + extra, True); s += extra
        if probe and k >= 4 and thr_q8 and hi - lo == NB:
            L = level_of(min(sums[-4:]), thr_q8, floor)
            if L + 1 <= 65536:
                x[lo + 311] = word_of(L); x[lo + 733] = word_of(L + 1, True)
                s += 2 * L + 1 - 2 * c
                at_level.append(lo + 311); above.append(lo + 733)
        sums.append(s)
    assert [int(v) for v in np.add.reduceat(np.abs(x.astype(np.int64)).sum(axis=1), [max(k * NB - p0, 0) for k in range(len(blocks))])] == sums
    return x, np.array(at_level, dtype=np.int64), np.array(above, dtype=np.int64)


LEVEL_BLOCKS = ([(300, 0, True)] * 5 + [(900, 0, True), (500, 0, True)] + [(900, 0, True)] * 5             # the minimum in slots 3, 2, 1, 0
                + [(700, 1023, False)] + [(2000, 0, True)] * 5 + [(700, 1024, False)] + [(2000, 0, True)] * 5    # ref >> 10: 700 and 701
                + [(100, 0, True)] * 4 + [(20000, 0, False)] * 6 + [(100, 0, True)] * 2)                      # four loud blocks, then passed
LEVEL_POSITIONS = (389, 3 * NB + 801)
LEVEL_THR = (256, 257, 1024, 1365, 4095, 4096)
LEVEL_FLOORS = (0, 64, 65535)


def silent_row(position: int, n_blocks: int = 10, seed: int = 5):
    """CS16 silence with forty samples of magnitude 1 .. 20 in every block: a block's sum stays below 1024."""
    rng = np.random.default_rng(seed)
    n = n_blocks * NB - position % NB
    x = np.zeros((n, 2), dtype=np.int16)
    for k in range(n_blocks):
        lo, hi = max(k * NB - position % NB, 0), (k + 1) * NB - position % NB
        at = lo + rng.choice(hi - lo, size=min(40, hi - lo), replace=False)
        v = rng.integers(1, 21, size=len(at)) * (1 - 2 * rng.integers(0, 2, size=len(at)))
        x[at, rng.integers(0, 2, size=len(at))] = v
    return x


RAIL_BLOCKS = [(65536, 0, False)] * 5 + [(100, 0, False)] * 6   # (-32768, -32768): thr_q8 * (ref >> 10) = 2^28 at 4096
