"""Restatement of automatic frequency control (include/navtex_amd_afc.h), written from the header's text, not from
nvx_afc_law.h: the law in numpy float64 (every operation a numpy scalar operation of its own: no contraction), with
NVX_AFC_C parsed from the header; the k sequence of a chain from its per-launch records; and the inputs the tests track:
a synthetic stream (nv.synth_host, as signal_ref.synth builds it) multiplied by a float64 chirp and rounded to int16, and
two segments whose carriers differ joined at a frame boundary."""
from __future__ import annotations

import math
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "navtex_amd_afc.h").read_text()
C = np.float64(float.fromhex(re.search(r"#define NVX_AFC_C\s+(0x[0-9a-fA-F.]+p[-+]?\d+)", HEADER).group(1)))
STEP_HZ = 3.125
K_MAX = int(25000.0 / STEP_HZ)
DEFAULTS = dict(gain_shift=1, max_step=8, range_k=48, min_samples=256, contrast_min=0.7)
UPDATE, CLAMP = 4, 8                  # what step() reports beside K[L+2]: the gate passed and d was finite; a limit cut the step


def step(par: dict, kc: int, k0: int, k1: int, rec: dict):
    """(K[L+2], flags) of a tracking chain that took part in launch L: rec = its record of that launch (samples, b_samples,
    sum_dphi_b, sum_dphi_y, sum_mf_hi, sum_mf_lo), k0 = K[L], k1 = K[L+1]."""
    f64 = np.float64
    n, nb = int(rec["samples"]), int(rec["b_samples"])
    ny = n - nb
    hi, lo = f64(rec["sum_mf_hi"]), f64(rec["sum_mf_lo"])
    with np.errstate(all="ignore"):
        if n < par["min_samples"]:
            return k1, 0
        if 8 * nb < n or 8 * ny < n:
            return k1, 0
        if not ((hi - lo) >= f64(par["contrast_min"]) * (hi + lo)):
            return k1, 0
        e = (f64(rec["sum_dphi_b"]) / f64(nb) + f64(rec["sum_dphi_y"]) / f64(ny)) * C
        r = e - f64(k1 - k0)
        d = np.rint(np.ldexp(r, -par["gain_shift"]))
    if not np.isfinite(d):
        return k1, 0
    flags = UPDATE
    if abs(d) > par["max_step"]:
        d, flags = math.copysign(par["max_step"], d), flags | CLAMP
    k2 = k1 + int(d)
    for lo_k, hi_k in ((kc - par["range_k"], kc + par["range_k"]), (-K_MAX, K_MAX)):
        if not lo_k <= k2 <= hi_k:
            k2, flags = min(max(k2, lo_k), hi_k), flags | CLAMP
    return k2, flags


def trace(par: dict, kc: int, records, n_launches: int | None = None):
    """K[0 .. n) of a chain whose tracking starts (enable, reset, nvx_set_carrier) in front of launch 0: records[L] = its
    record of launch L, or None where its stream took no part (a hold).  Returns (K, flags per launch); n_launches up to
    len(records) + 2: the records decide the k of two launches more."""
    K, F = [kc, kc], []
    for L in range(len(records)):
        if records[L] is None:
            K.append(K[L + 1]); F.append(None)
        else:
            k2, f = step(par, kc, K[L], K[L + 1], records[L])
            K.append(k2); F.append(f)
    return K[:len(records) if n_launches is None else n_launches], F


def chirp(iq: np.ndarray, rate: int, hz1: float, ramp: int, chunk: int = 1 << 22) -> np.ndarray:
    """IQ int16 [n, 2] times exp(j phi): the frequency rises linearly from 0 to hz1 over the first `ramp` samples and
    holds; float64 throughout, rounded to nearest (ties to even) and clipped to int16."""
    iq = np.ascontiguousarray(iq, dtype=np.int16).reshape(-1, 2)
    out = np.empty_like(iq)
    for a in range(0, iq.shape[0], chunk):
        n = np.arange(a, min(a + chunk, iq.shape[0]), dtype=np.float64)
        m = np.minimum(n, float(ramp))
        cycles = (hz1 / (2.0 * ramp)) * m * m / rate + hz1 * (n - m) / rate if ramp else hz1 * n / rate
        ph = 2.0 * np.pi * (cycles - np.floor(cycles))
        c, s = np.cos(ph), np.sin(ph)
        x, y = iq[a:a + n.shape[0], 0].astype(np.float64), iq[a:a + n.shape[0], 1].astype(np.float64)
        out[a:a + n.shape[0], 0] = np.clip(np.rint(x * c - y * s), -32768, 32767).astype(np.int16)
        out[a:a + n.shape[0], 1] = np.clip(np.rint(x * s + y * c), -32768, 32767).astype(np.int16)
    return out


def carriers(nv, text: str, delta: int, amp: int = 8000):
    bits = nv.sitor_encode(text, 40)
    return [dict(freq_hz=14000 + delta, bits=bits, bit_offset=301, phase0=5, amplitude=amp),
            dict(freq_hz=-14000 + delta, bits=bits, bit_offset=777, phase0=9, amplitude=amp)], len(bits)


def segment(nv, rate: int, frames: int, text: str, delta: int = 0, seed: int = 11, noise: int = 1500, amp: int = 8000) -> np.ndarray:
    """`frames` frames of a NAVTEX carrier per chain, delta Hz off nominal (signal_ref.synth's stream with a text of ours)."""
    frame = nv.FRAME_RAW if rate == nv.RATE_RAW else nv.FRAME_IN
    car, _ = carriers(nv, text, delta, amp)
    return nv.synth_host(nv.make_stream(car, seed=seed, noise_amp=noise), rate, frames * frame)


def frames_for(nv, text: str, spare: int = 4) -> int:
    """Frames that hold `text`'s transmission from its first bit (100 bits a second, 0.32 s a frame) and `spare` more."""
    return int(math.ceil(len(nv.sitor_encode(text, 40)) / 100.0 / 0.32)) + spare


FILLER = "CARRIER WARMING UP = THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG 0123456789\nNNNN\n"
MESSAGE = "ZCZC QA07\nAFC HOLD TEST\nNNNN\n"
DRIFT_HZ, DRIFT_FRAMES = 90, 30


def drift_then_hold(nv, rate: int, hz: int = DRIFT_HZ, ramp_frames: int = DRIFT_FRAMES, seed: int = 11):
    """(IQ, frames of the ramp, frames in all): FILLER (no ZCZC: no message) while both carriers drift from 0 to +hz over ramp_frames frames,
    then MESSAGE on carriers that hold at +hz."""
    frame = nv.FRAME_RAW if rate == nv.RATE_RAW else nv.FRAME_IN
    a = chirp(segment(nv, rate, ramp_frames, FILLER, 0, seed), rate, float(hz), ramp_frames * frame)
    hold = frames_for(nv, MESSAGE)
    b = segment(nv, rate, hold, MESSAGE, hz, seed + 1)
    return np.concatenate([a, b]), ramp_frames, ramp_frames + hold


def stepped(nv, rate: int, frames_a: int, frames_b: int, hz: int, seed: int = 11) -> np.ndarray:
    """Two segments joined at a frame boundary: carriers at nominal, then hz off."""
    return np.concatenate([segment(nv, rate, frames_a, FILLER, 0, seed), segment(nv, rate, frames_b, FILLER, hz, seed + 1)])
