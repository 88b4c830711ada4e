"""Numpy restatement of the signal report (include/navtex_amd_signal.h) from a chain's 900 S/s samples y3 and its
discriminator output delta-phi, written from the header's definition, not from the kernels.

Per sample t with g(t) >= 8 (g = index since the stream's reset): P = I*I + Q*Q, phi = delta-phi, d = the decision of the
five-sample window ending at t ('B' = 1), hi / lo = max / min of that window's float32 energies Brot / Yrot.  The window
energies are restated in float32 / float64 exactly as timing_ref.decisions states the decision (receiver/decoder.C:96-132,
zeros in front of sample 0), and the decisions they give must be timing_ref.decisions'."""
from __future__ import annotations

import math

import numpy as np

G_DAB = 8
HZ = 900.0 / (2.0 * math.pi)
SUMS = ("sum_power", "sum_dphi_b", "sum_dphi2_b", "sum_dphi_y", "sum_dphi2_y", "sum_mf_hi", "sum_mf_lo")
DERIVED = ("power_db", "b_hz", "y_hz", "offset_hz", "shift_hz", "eye_snr_db", "contrast")


def energies(y3: np.ndarray, fR: np.ndarray, fI: np.ndarray):
    """(Brot, Yrot) as float32 of the window ENDING at every sample (history of zeros in front of sample 0)."""
    y = np.vstack([np.zeros((4, 2)), np.asarray(y3, dtype=np.float64).reshape(-1, 2)])
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
    return BR * BR + BI * BI, YR * YR + YI * YI


def terms(y3: np.ndarray, dphi: np.ndarray, fR, fI, start: int = 0, stop: int | None = None):
    """Per counted sample: (P, phi, d, hi, lo).  y3 / dphi: a chain's samples since its stream's reset (g = index); the
    samples counted are those in [start, stop) with g >= 8 (earlier samples still fill the windows)."""
    y3 = np.asarray(y3, dtype=np.float64).reshape(-1, 2)
    B, Y = energies(y3, fR, fI)
    d = (B > Y).astype(np.uint8)
    hi = np.maximum(B, Y).astype(np.float64)
    lo = np.minimum(B, Y).astype(np.float64)
    P = y3[:, 0] * y3[:, 0] + y3[:, 1] * y3[:, 1]
    g = np.arange(y3.shape[0])
    keep = (g >= max(start, G_DAB)) & (g < (y3.shape[0] if stop is None else stop))
    return P[keep], np.asarray(dphi, dtype=np.float64)[keep], d[keep], hi[keep], lo[keep]


def report(y3: np.ndarray, dphi: np.ndarray, fR, fI, start: int = 0, stop: int | None = None) -> dict:
    """The record over samples [start, stop) of a chain: counts, sums and, under 'mag_<sum>', the sum of its terms'
    magnitudes (the scale of the tolerance a device sum is held to)."""
    P, phi, d, hi, lo = terms(y3, dphi, fR, fI, start, stop)
    b = d == 1
    cols = {"sum_power": P, "sum_dphi_b": phi[b], "sum_dphi2_b": phi[b] * phi[b], "sum_dphi_y": phi[~b],
            "sum_dphi2_y": phi[~b] * phi[~b], "sum_mf_hi": hi, "sum_mf_lo": lo}
    r = {"samples": int(P.shape[0]), "b_samples": int(b.sum())}
    for k, v in cols.items():
        r[k] = math.fsum(v)
        r["mag_" + k] = math.fsum(np.abs(v))
    return r


def merge(a: dict, b: dict) -> dict:
    return {k: a[k] + b[k] for k in a}


def derive(r: dict) -> dict:
    """The header's derived fields from counts and sums, in double; NaN where a denominator is 0."""
    nan = float("nan")
    n, nb = r["samples"], r["b_samples"]
    ny = n - nb
    out = {"power_db": 10.0 * math.log10(r["sum_power"] / n) if n and r["sum_power"] > 0 else (-math.inf if n else nan)}
    mb = r["sum_dphi_b"] / nb if nb else nan
    my = r["sum_dphi_y"] / ny if ny else nan
    out["b_hz"], out["y_hz"] = mb * HZ, my * HZ
    out["offset_hz"] = (out["b_hz"] + out["y_hz"]) / 2.0
    out["shift_hz"] = out["b_hz"] - out["y_hz"]
    vb = max(0.0, r["sum_dphi2_b"] / nb - mb * mb) if nb else 0.0
    vy = max(0.0, r["sum_dphi2_y"] / ny - my * my) if ny else 0.0
    noise = (vb + vy) / 2.0
    half = (mb - my) / 2.0
    out["eye_snr_db"] = 10.0 * math.log10(half * half / noise) if nb and ny and noise > 0 else nan
    mf = r["sum_mf_hi"] + r["sum_mf_lo"]
    out["contrast"] = (r["sum_mf_hi"] - r["sum_mf_lo"]) / mf if mf != 0 else nan
    return out


def check_sums(got: dict, want: dict, rel: float = 1e-12, where: str = "") -> None:
    """Counts equal; every sum within rel of the sum of its terms' magnitudes."""
    assert got["samples"] == want["samples"] and got["b_samples"] == want["b_samples"], \
        (where, got["samples"], want["samples"], got["b_samples"], want["b_samples"])
    for k in SUMS:
        tol = rel * want["mag_" + k]
        assert abs(got[k] - want[k]) <= tol, (where, k, got[k], want[k], tol)


def check_derived(got: dict, rel: float = 1e-13) -> None:
    """The derived fields of a report are the header's formulas applied to its own sums."""
    want = derive(got)
    for k in DERIVED:
        a, b = got[k], want[k]
        if math.isnan(b):
            assert math.isnan(a), (k, a)
        elif math.isinf(b):
            assert a == b, (k, a, b)
        else:
            assert abs(a - b) <= rel * max(1.0, abs(b)), (k, a, b)


# ---- the physical checks (tests/test_signal_report.py on the oracle's y3, tests/test_gpu_signal_report.py on the
# device's), with tolerances measured on the oracle's y3 over 20 s of a synthetic NAVTEX carrier per chain (+14 kHz: the
# 518 chain, -14 kHz: the 490 chain), amplitude 8000, noise_amp 1500, both input rates:
#   offset_hz - delta, delta in {-30, -10, 0, +20} Hz:  -2.3 .. +9.9 Hz.  The estimate leans toward +2 Hz at 0 (the
#                       message's own mix of tones and transitions) and is compressed at +-30 Hz, where one tone nears the
#                       edge of the channel filter (-30: +5.9 .. +9.9).  Asserted: within OFFSET_TOL, and rising with delta.
#   shift_hz:           134 .. 148 Hz (transition samples pull both class means inward).  Asserted: in SHIFT_BAND.
#   amplitude x 2:      +6.020 dB on both chains and rates (the noise is far below the carrier).  Asserted: 6.02 +- 0.02.
#   eye_snr_db, amplitude 300, noise_amp 1000 / 3000 / 8000 / 20000: 6.1 .. -12.9 dB (252 kS/s), 6.3 .. -5.1 (raw rate),
#                       strictly falling.  Asserted: strictly falling.
#   noise only:         eye -15.0 .. -13.6 dB, contrast 0.489 .. 0.496; the carriers above: eye >= 4.5 dB, contrast
#                       >= 0.85.  Asserted: separated by EYE_SPLIT_DB and CONTRAST_SPLIT.
SECONDS = 20
OFFSETS = (-30, -10, 0, 20)
OFFSET_TOL = 11.0
SHIFT_BAND = (120.0, 165.0)
AMP_DB, AMP_DB_TOL = 6.02, 0.02
NOISE_LEVELS = (1000, 3000, 8000, 20000)
EYE_SPLIT_DB, CONTRAST_SPLIT = -5.0, 0.7


def synth(nv, rate: int, delta: int = 0, amp: int = 8000, noise: int = 1500, carrier: bool = True, secs: int = SECONDS):
    """(IQ int16 [n, 2], frames): a NAVTEX carrier per chain, delta Hz off its nominal frequency, whole frames."""
    import signals
    frame = nv.FRAME_RAW if rate == nv.RATE_RAW else nv.FRAME_IN
    frames = int(secs * rate) // frame
    bits = nv.sitor_encode(signals.stream_text(7), 40)
    car = ([dict(freq_hz=14000 + delta, bits=bits, bit_offset=301, phase0=5, amplitude=amp),
            dict(freq_hz=-14000 + delta, bits=bits, bit_offset=777, phase0=9, amplitude=amp)] if carrier else [])
    return nv.synth_host(nv.make_stream(car, seed=11, noise_amp=noise), rate, frames * frame), frames


def check_physics(reports) -> None:
    """reports(rate, chain, delta=0, amp=8000, noise=1500, carrier=True) -> a report dict with the derived fields."""
    for chain in (0, 1):
        offs = [reports(chain, delta=d)["offset_hz"] for d in OFFSETS]
        for d, o in zip(OFFSETS, offs):
            assert abs(o - d) <= OFFSET_TOL, (chain, d, o)
        assert all(b > a for a, b in zip(offs, offs[1:])), (chain, offs)
        base = reports(chain)
        assert SHIFT_BAND[0] <= base["shift_hz"] <= SHIFT_BAND[1], (chain, base["shift_hz"])
        gain = reports(chain, amp=16000)["power_db"] - base["power_db"]
        assert abs(gain - AMP_DB) <= AMP_DB_TOL, (chain, gain)
        eyes = [reports(chain, amp=300, noise=n)["eye_snr_db"] for n in NOISE_LEVELS]
        assert all(b < a for a, b in zip(eyes, eyes[1:])), (chain, eyes)
        quiet = reports(chain, carrier=False)
        assert quiet["eye_snr_db"] < EYE_SPLIT_DB < base["eye_snr_db"], (chain, quiet["eye_snr_db"], base["eye_snr_db"])
        assert quiet["contrast"] < CONTRAST_SPLIT < base["contrast"], (chain, quiet["contrast"], base["contrast"])
