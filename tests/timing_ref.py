"""Plain numpy restatement of the demodulator's bit-timing filter and mark/space decision (receiver/decoder.C:73-215),
written from the reference's definitions, not from the kernels or the oracle, plus what the GPU tests need to compare
the device's debug taps (nvx_debug_dphi / nvx_debug_timing) with the oracle's (oracle_binding.decode_taps).

With g = 900 S/s sample index since reset:
  |corr|(g)  = |sum_i mask[i] * dphi(g - 8 + i)|, i ascending, for g >= 8 (decoder.C:157-177)
  S(g)       = sum over ring positions p = c, c + 9, ..., c + 558 ascending of the |corr| value held at p, c = (g - 574) mod 9;
               the ring (567 entries) holds |corr| value kappa at position kappa mod 567, kappa = g - 8 (decoder.C:181-197)
  arg-max    = first maximum of S(g - 8 .. g) at g >= 582, (g - 582) mod 9 == 0 (decoder.C:202-215)
Sums are accumulated element-wise in numpy in the reference's order, so every rounding is the reference's."""
from __future__ import annotations

import numpy as np

MASK = (0, 1, 1, 1, 0, -1, -1, -1, 0)          # receiver/decoder.h correlation_mask
RING = 567                                      # CORRELATION_BUF_SAMPLE_SIZE
G_DAB, G_CB, G_CSA = 8, 574, 582
MOD = 9 * RING                                  # the ring algebra repeats every 5103 samples


def corr(dphi: np.ndarray) -> np.ndarray:
    n = dphi.shape[0]
    out = np.full(n, np.nan)
    if n <= G_DAB:
        return out
    acc = np.zeros(n - G_DAB)
    for i, m in enumerate(MASK):
        acc = acc + float(m) * dphi[i:n - G_DAB + i]
    out[G_DAB:] = np.abs(acc)
    return out


def class_sums(c: np.ndarray) -> np.ndarray:
    n = c.shape[0]
    out = np.full(n, np.nan)
    if n <= G_CB:
        return out
    g = np.arange(G_CB, n)
    cls = (g - G_CB) % 9
    kappa = g - G_DAB
    acc = np.zeros(g.shape[0])
    for j in range(RING // 9):
        p = cls + 9 * j                                  # ring position, ascending
        held = kappa - (kappa - p) % RING                # the newest |corr| value kappa' <= kappa stored at p
        acc = acc + c[held + G_DAB]
    out[G_CB:] = acc
    return out


def evaluations(n: int) -> np.ndarray:
    """Samples at which the timing filter evaluates (decoder.C:200-202)."""
    return np.arange(G_CSA, n, 9)


def argmax(s: np.ndarray) -> np.ndarray:
    """-1 everywhere but at the evaluations: the first maximum of S(g - 8 .. g)."""
    out = np.full(s.shape[0], -1, dtype=np.int32)
    g = evaluations(s.shape[0])
    if g.size:
        win = s[g[:, None] + np.arange(-8, 1)[None, :]]
        out[g] = np.argmax(win, axis=1)                  # numpy's arg-max is the first one, as strict '>' from -1.0
    return out


def margins(s: np.ndarray):
    """Per evaluation: (best, best - runner_up), runner_up = the second largest of the nine (equal to best on a tie)."""
    g = evaluations(s.shape[0])
    win = np.sort(s[g[:, None] + np.arange(-8, 1)[None, :]], axis=1)
    return win[:, -1], win[:, -1] - win[:, -2]


def tie_stats(sums):
    """What nvx_demod_tie_stats must report over the class sums of several chains: (near_ties, evaluations, min_margin as
    float32) -- an evaluation counts when best > 0, a near tie when margin < best * 2^-40."""
    near, evals, mins = 0, 0, []
    for s in sums:
        best, m = margins(s)
        live = best > 0
        evals += int(live.sum())
        near += int((m[live] < best[live] * 2.0 ** -40).sum())
        if live.any():
            mins.append(np.float32(m[live] / best[live]).min())
    return near, evals, (min(mins) if mins else None)


def decisions(y3: np.ndarray, fR: np.ndarray, fI: np.ndarray) -> np.ndarray:
    """Mark/space decision ('B' = 1) of a five-sample window ENDING at every sample t (decoder.C:96-132, history of zeros in
    front of sample 0): float * float and double * float products, double sums, accumulators rounded to float."""
    y = np.vstack([np.zeros((4, 2)), np.asarray(y3, dtype=np.float64)])
    n = y.shape[0] - 4
    f32, f64 = np.float32, np.float64
    BR = BI = YR = YI = np.zeros(n, dtype=f32)
    for i in range(5):
        sR, sI = y[i:i + n, 0], y[i:i + n, 1]
        r32 = sR.astype(f32)
        YR = (YR.astype(f64) + ((r32 * fR[i]).astype(f64) - sI * f64(fI[i]))).astype(f32)
        YI = (YI.astype(f64) + ((r32 * fI[i]).astype(f64) + sI * f64(fR[i]))).astype(f32)
        BR = (BR.astype(f64) + ((r32 * fR[i]).astype(f64) + sI * f64(fI[i]))).astype(f32)
        BI = (BI.astype(f64) + (((-sR).astype(f32) * fI[i]).astype(f64) + sI * f64(fR[i]))).astype(f32)
    Brot = BR * BR + BI * BI
    Yrot = YR * YR + YI * YI
    return (Brot > Yrot).astype(np.uint8)


def u64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class DeviceTaps:
    """Collects, launch by launch, what a Pipeline's demodulator saw and computed for every decoded (stream, chain): y3,
    delta-phi, |corr|, class sums and the front kernel's words.  Every call of `launch(op)` must make exactly one launch
    (`launches` = 0 allows none): the debug taps hold the LAST launch only."""

    def __init__(self, p, chains, push_mode: bool):
        self.p, self.chains, self.push_mode = p, list(chains), push_mode
        self.parts = {sc: {k: [] for k in ("y3", "dphi", "corr", "csum", "words")} for sc in self.chains}
        self.n_launches = 0

    def launch(self, op, launches: int = 1):
        before = self.p.integrity_stats()[2]
        op()
        self.p.flush() if self.push_mode else self.p.fetch()
        got = self.p.integrity_stats()[2] - before
        assert got == launches, f"{got} launches where {launches} were meant"
        if not got:
            return
        self.n_launches += 1
        for sc in self.chains:
            y3 = self.p.debug_y3(*sc)
            c, s, w = self.p.debug_timing(*sc)
            n = y3.shape[0]
            assert c.shape[0] == n and w.shape[0] == (n + 8) // 9
            d = self.p.debug_dphi(*sc)[:n]
            for k, v in (("y3", y3), ("dphi", d), ("corr", c), ("csum", s), ("words", w)):
                self.parts[sc][k].append(v)

    def chain(self, sc):
        return {k: np.concatenate(v) if v else np.zeros((0, 2) if k == "y3" else 0) for k, v in self.parts[sc].items()}
