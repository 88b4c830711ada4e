"""Restatement of per-chain carrier tuning (include/navtex_amd_tune.h), written from the header's contract, not from
the kernels: the oracle's stage 0 / FIR1, then per chain and frame either the oracle's reference mixer (the chain at its
nominal k) or the tuned mixer in numpy -- u(o) = (I cr - Q ci, I ci + Q cr), (cr, ci) = T[(k o) mod N], T parsed from
navtex_amd/csrc/nvx_tune_table.h (numpy applies each fp64 operation on its own, no contraction) -- then the oracle's
FIR2, FIR3 and decoder.  k may change at a frame boundary (a frame is N = 20160 FIR1 outputs)."""
from __future__ import annotations

import functools
import re
from pathlib import Path

import numpy as np

import oracle_binding as ob

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "navtex_amd" / "csrc" / "nvx_tune_table.h"
N = 20160
OCT = N // 8
NOMINAL = (4480, -4480)
STEP_HZ = 3.125


def octant():
    """[(cos, sin)] of 2 pi j / N, j = 0 .. N/8, as the header holds them."""
    body = HEADER.read_text().split("NVX_TUNE_OCTANT", 1)[1]
    pairs = re.findall(r"\{\s*([-+0-9a-fx.p]+),\s*([-+0-9a-fx.p]+)\s*\}", body)
    assert len(pairs) == OCT + 1
    return [(float.fromhex(c), float.fromhex(s)) for c, s in pairs]


@functools.lru_cache(maxsize=None)
def table():
    """(cr, ci) [N] each: T[j] = (cos, -sin) of 2 pi j / N from the octant by the exact symmetries."""
    oc = np.array(octant())
    j = np.arange(N)
    q, r = j // (N // 4), j % (N // 4)
    lo = r <= OCT
    c = np.where(lo, oc[np.minimum(r, OCT), 0], oc[np.minimum(N // 4 - r, OCT), 1])
    s = np.where(lo, oc[np.minimum(r, OCT), 1], oc[np.minimum(N // 4 - r, OCT), 0])
    cq = np.select([q == 0, q == 1, q == 2, q == 3], [c, -s, -c, s])
    sq = np.select([q == 0, q == 1, q == 2, q == 3], [s, c, -s, -c])
    return cq, -sq


def k_of(hz: float) -> int:
    return int(np.rint(hz / STEP_HZ))


def mix_tuned(y1: np.ndarray, k: int, o0: int = 0) -> np.ndarray:
    """The tuned mixer over FIR1 outputs o0, o0 + 1, ... (o0 counted since the stream's reset)."""
    cr, ci = table()
    idx = (k % N) * ((o0 + np.arange(y1.shape[0])) % N) % N
    I, Q = y1[:, 0], y1[:, 1]
    a, b = cr[idx], ci[idx]
    return np.stack([I * a - Q * b, I * b + Q * a], axis=1)


def front(iq: np.ndarray, raw: bool, stage0_order: int = 1) -> np.ndarray:
    """FIR1 output of a stream from its reset: IQ int16 [n, 2] at 2.016 MS/s (raw) or 252 kS/s."""
    if raw:
        x = ob.stage0_cic3(iq) if stage0_order == 3 else ob.stage0(iq)
    else:
        x = np.ascontiguousarray(iq, dtype=np.int16).reshape(-1, 2)
    return ob.fir1(x)


def chain(y1: np.ndarray, ch: int, ks) -> np.ndarray:
    """y3 of chain ch (0 = 518, 1 = 490): ks = one k, or a k per frame (the last one holds for the rest)."""
    ks = [ks] if np.isscalar(ks) else list(ks)
    n_fr = (y1.shape[0] + N - 1) // N
    ks = ks + [ks[-1]] * max(0, n_fr - len(ks))
    ref = None
    parts = []
    for f in range(n_fr):
        seg = y1[f * N:(f + 1) * N]
        if ks[f] == NOMINAL[ch]:
            if ref is None:
                ref = ob.mix(y1, ch)             # the reference mixer (index o mod 9: a frame starts at 0)
            parts.append(ref[f * N:(f + 1) * N])
        else:
            parts.append(mix_tuned(seg, ks[f], f * N))
    return ob.fir3(ob.fir2(np.concatenate(parts)))


def decode(y3: np.ndarray) -> str:
    return ob.decode(y3)[0]


def messages(bits: str, freq: int = 518):
    cl = ob.CharLayer(freq)
    cl.feed(bits)
    return [m for _, _, m in cl.messages]
