"""Restatement of the multi-tap noise canceller (include/navtex_amd_wanc.h), written from the header's contract, not from the
kernels: the conversion (the resampler's), the 4 K + 1 block sums in numpy int64, the window, the seven steps of the solve in
Python floats (IEEE binary64, every operation rounded on its own) and integers, the apply in numpy int64 with the header's
bounds asserted, and the carried state of a pair cut into calls anywhere."""
from __future__ import annotations

import math

import numpy as np

import resample_ref as rr

BLOCK = 65536
WINDOW_LOG2_DEFAULT, TAPS_DEFAULT, LOAD_LOG2_DEFAULT = 2, 8, 12
TRACK, HOLD = 0, 1
CS16, CU8, CS8, CF32 = rr.CS16, rr.CU8, rr.CS8, rr.CF32
W_ONE, W_MAX, L1_MAX, COHERENCE_ONE = 8192, 32767, 65534, 16384


def n_sums(K: int) -> int:
    return 4 * K + 1


def solve(t, K: int, window_log2: int, load_log2: int):
    """Steps 1 .. 7 on the window's sums (Re R[0 .. K), Im R, Re Q, Im Q, TAA): ((w_re, w_im) as tuples, coherence, reason)."""
    t = [int(v) for v in t]
    assert len(t) == n_sums(K) and all(abs(v) <= 1 << 53 for v in t)
    zero = ((0,) * K, (0,) * K)
    R0, TAA = t[0], t[4 * K]
    N = 1 << (16 + window_log2)
    if R0 < 16 * N:
        return zero, 0, 1
    rr_, ri, qr, qi = ([float(v) for v in t[i * K:(i + 1) * K]] for i in range(4))
    diag = float(R0 + (R0 >> load_log2) + 1)
    Lr = [[0.0] * K for _ in range(K)]
    Li = [[0.0] * K for _ in range(K)]
    d, e = [0.0] * K, [0.0] * K
    for j in range(K):
        s = diag
        for m in range(j):
            s = s - (Lr[j][m] * Lr[j][m] + Li[j][m] * Li[j][m]) * d[m]
        d[j] = s
        if not (0.0 < s < math.inf):
            return zero, 0, 2
        e[j] = 1.0 / s
        for i in range(j + 1, K):
            sr, si = rr_[i - j], ri[i - j]
            for m in range(j):
                ur = Lr[i][m] * Lr[j][m] + Li[i][m] * Li[j][m]
                ui = Li[i][m] * Lr[j][m] - Lr[i][m] * Li[j][m]
                sr = sr - ur * d[m]
                si = si - ui * d[m]
            Lr[i][j], Li[i][j] = sr * e[j], si * e[j]
    xr, xi = [0.0] * K, [0.0] * K
    for j in range(K):
        zr, zi = qr[j], qi[j]
        for m in range(j):
            zr, zi = zr - (Lr[j][m] * xr[m] - Li[j][m] * xi[m]), zi - (Lr[j][m] * xi[m] + Li[j][m] * xr[m])
        xr[j], xi[j] = zr, zi
    for j in range(K):
        xr[j], xi[j] = xr[j] * e[j], xi[j] * e[j]
    for j in range(K - 1, -1, -1):
        vr, vi = xr[j], xi[j]
        for i in range(j + 1, K):
            vr, vi = vr - (Lr[i][j] * xr[i] + Li[i][j] * xi[i]), vi - (Lr[i][j] * xi[i] - Li[i][j] * xr[i])
        xr[j], xi[j] = vr, vi
    c = 0.0
    for k in range(K):
        c = c + (xr[k] * qr[k] + xi[k] * qi[k])
    coherence = 0
    if TAA > 0:
        v = (16384.0 * c) / float(TAA)
        coherence = 0 if not v >= 1.0 else (COHERENCE_ONE if v >= 16384.0 else int(v))
    w = []
    for x in xr + xi:
        v = 8192.0 * x
        if not (math.isfinite(v) and -32767.0 <= round(v) <= 32767.0):
            return zero, coherence, 3
        w.append(int(round(v)))                                # Python rounds halves to even
    if sum(abs(v) for v in w) > L1_MAX:
        return zero, coherence, 3
    return (tuple(w[:K]), tuple(w[K:])), coherence, 0


def _conj_products(x: np.ndarray, y: np.ndarray):
    """sum x conj(y) of int64 [n, 2] rows: (re, im), with the header's bounds on every term."""
    re = x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]
    im = x[:, 1] * y[:, 0] - x[:, 0] * y[:, 1]
    if len(x):
        assert -(1 << 31) + 65536 <= re.min() and re.max() <= 1 << 31 and np.abs(im).max() <= (1 << 31) - 32768
    return int(re.sum()), int(im.sum())


def block_sums(ad: np.ndarray, bh: np.ndarray, K: int) -> np.ndarray:
    """ad: the delayed main samples a[n - G] of the span, int64 [n, 2]; bh: the sense samples b[n - (K - 1)] .. b[n_last], int64
    [n + K - 1, 2].  The 4 K + 1 sums as int64."""
    n = len(ad)
    out = np.zeros(n_sums(K), dtype=np.int64)
    cur = bh[K - 1:]
    for k in range(K):
        lag = bh[K - 1 - k:K - 1 - k + n]
        out[k], out[K + k] = _conj_products(cur, lag)
        out[2 * K + k], out[3 * K + k] = _conj_products(ad, lag)
    out[4 * K] = int((ad[:, 0] * ad[:, 0] + ad[:, 1] * ad[:, 1]).sum())
    assert out[K] == 0
    return out


def apply(ad: np.ndarray, bh: np.ndarray, w, K: int) -> np.ndarray:
    """The delayed main samples and the sense span as in block_sums -> int16 [n, 2]."""
    n = len(ad)
    w_re, w_im = w
    assert all(abs(v) <= W_MAX for v in w_re + w_im) and sum(abs(v) for v in w_re + w_im) <= L1_MAX
    p = np.full(n, 4096, dtype=np.int64)
    r = np.full(n, 4096, dtype=np.int64)
    for k in range(K):
        lag = bh[K - 1 - k:K - 1 - k + n]
        p += w_re[k] * lag[:, 0] - w_im[k] * lag[:, 1]
        r += w_re[k] * lag[:, 1] + w_im[k] * lag[:, 0]
        assert n == 0 or max(np.abs(p).max(), np.abs(r).max()) < 1 << 31
    return np.stack([np.clip(ad[:, 0] - (p >> 13), -32768, 32767), np.clip(ad[:, 1] - (r >> 13), -32768, 32767)], axis=1).astype(np.int16)


def pack(iq16: np.ndarray) -> np.ndarray:
    """int16 [n, 2] -> the uint32 words the kernel writes."""
    a = iq16.astype(np.int64)
    return ((a[:, 0] & 0xffff) | ((a[:, 1] & 0xffff) << 16)).astype(np.uint32)


class Canceller:
    """One pair, fed in calls of any length."""

    def __init__(self, fmt: int = CS16, n_taps: int = TAPS_DEFAULT, window_log2: int = WINDOW_LOG2_DEFAULT, load_log2: int = LOAD_LOG2_DEFAULT,
                 position: int = 0):
        assert window_log2 in (2, 4, 6) and n_taps in (4, 8, 16) and 8 <= load_log2 <= 20
        self.fmt, self.K, self.G, self.window_log2, self.W, self.load_log2 = fmt, n_taps, n_taps // 2, window_log2, 1 << window_log2, load_log2
        self.mode = TRACK
        self.samples = self.solved = self.rejected = 0
        self.reset(position)

    def reset(self, position: int = 0) -> None:
        """Position `position`, no block complete, zero weights, silence in front; the mode and the counters stay."""
        K = self.K
        self.position = position
        self.ring = np.zeros((self.W, n_sums(K)), dtype=np.int64)      # block b in slot b mod W
        self.partial = np.zeros(n_sums(K), dtype=np.int64)
        self.complete = 0
        self.w = ((0,) * K, (0,) * K)
        self.coherence = 0
        self.reason = 0
        self.hist_b = np.zeros((K - 1, 2), dtype=np.int64)             # b[position - (K - 1)] ..
        self.hist_a = np.zeros((self.G, 2), dtype=np.int64)            # a[position - G] ..
        self.history = []                                              # (block, weights, coherence, reason) of every block start solved

    def set(self, w_re, w_im) -> None:
        w = (tuple(int(v) for v in w_re), tuple(int(v) for v in w_im))
        assert len(w[0]) == len(w[1]) == self.K and all(abs(v) <= W_MAX for v in w[0] + w[1]) and sum(abs(v) for v in w[0] + w[1]) <= L1_MAX
        self.w = w

    def set_mode(self, mode: int) -> None:
        assert mode in (TRACK, HOLD)
        self.mode = mode

    def sums(self):
        """The window's sums over its complete blocks, as Python integers."""
        return tuple(int(v) for v in self.ring.sum(axis=0))

    def push(self, main: np.ndarray, sense: np.ndarray) -> np.ndarray:
        a, b = rr.convert(main, self.fmt), rr.convert(sense, self.fmt)
        assert len(a) == len(b)
        K, G = self.K, self.G
        n_all = len(a)
        ad = np.concatenate([self.hist_a, a])[:n_all]                  # a[n - G] for the call's n
        bh = np.concatenate([self.hist_b, b])                          # b[n - (K - 1)] ..
        out = np.empty((n_all, 2), dtype=np.int16)
        at = 0
        while at < n_all:
            if self.position % BLOCK == 0 and self.mode == TRACK and self.complete >= self.W:
                self.w, self.coherence, self.reason = solve(self.sums(), K, self.window_log2, self.load_log2)
                self.solved += self.reason == 0
                self.rejected += self.reason != 0
                self.history.append((self.position // BLOCK, self.w, self.coherence, self.reason))
            n = min(n_all - at, BLOCK - self.position % BLOCK)
            sa, sb = ad[at:at + n], bh[at:at + n + K - 1]
            out[at:at + n] = apply(sa, sb, self.w, K)
            self.partial += block_sums(sa, sb, K)
            self.position += n
            at += n
            if self.position % BLOCK == 0:
                self.ring[(self.position // BLOCK - 1) % self.W] = self.partial
                self.partial = np.zeros(n_sums(K), dtype=np.int64)
                self.complete = min(self.W, self.complete + 1)
        self.hist_a = np.concatenate([self.hist_a, a])[n_all:n_all + G]
        self.hist_b = bh[n_all:]
        assert len(self.hist_a) == G and len(self.hist_b) == K - 1
        self.samples += n_all
        return out


def cancel(main: np.ndarray, sense: np.ndarray, fmt: int = CS16, n_taps: int = TAPS_DEFAULT, window_log2: int = WINDOW_LOG2_DEFAULT,
           load_log2: int = LOAD_LOG2_DEFAULT, position: int = 0):
    """One shot: (int16 [n, 2], the Canceller behind it)."""
    ref = Canceller(fmt, n_taps, window_log2, load_log2, position)
    return ref.push(main, sense), ref
