"""The down-converter bank's end-to-end case, computed once per process and shared by tests/test_ddc.py (restatements
only) and tests/test_gpu_ddc.py (the same input on the device): one 2.4 MS/s unsigned 8-bit input that holds three stations
with different texts, and the three slices the restatement (tests/ddc_ref.py) makes of it."""
from __future__ import annotations

import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import ddc_ref as dr
import resample_ref as rr

RATE = 2400000
PER_FRAME = RATE * 8 // 25                  # input samples per frame of 80640 outputs
# (carrier in the input, the slice's requested shift, text)
STATIONS = ((-400000 + 14000, -400000, "ZCZC DA01\nLOW\nNNNN\n"),
            (14000, 0, "ZCZC DB02\nMID\nNNNN\n"),
            (612345 - 14000, 612345, "ZCZC DC03\nHIGH\nNNNN\n"))


@functools.lru_cache(maxsize=None)
def source():
    """(samples uint8 [n, 2], frames): the three stations at amplitude 8000 each over a little noise, requantised to 8 bits."""
    import navtex_amd as nv
    bits = [nv.sitor_encode(text, 8) for _, _, text in STATIONS]
    frames = (max(len(b) for b in bits) + 150) * (RATE // 100) // PER_FRAME + 1
    n = frames * PER_FRAME
    with ThreadPoolExecutor(3) as ex:                                          # numpy releases the lock: the stations side by side
        parts = list(ex.map(lambda a: rr.cpfsk(a[1][1], RATE, n, freq_hz=a[1][0][0], amplitude=8000, noise_amp=500, seed=40 + a[0]),
                            enumerate(zip(STATIONS, bits))))
    total = np.sum(parts, axis=0, dtype=np.int32)
    src = rr.to_format(total, rr.CU8)
    src.setflags(write=False)
    return src, frames


@functools.lru_cache(maxsize=None)
def slices():
    """(rows int16 [3, n_out, 2], ks, residues in Hz): the restatement's three slices, with the plan's own taps."""
    import navtex_amd.ddc as dd
    import navtex_amd.resample as rs
    L, M, T, S, taps = rs.design(RATE)
    src, frames = source()
    x = rr.convert(src, rr.CU8)
    ks, residues = [], []
    for _, want_hz, _ in STATIONS:
        k, applied = dd.grid(RATE, want_hz)
        assert k == dr.grid(RATE, want_hz) and abs(want_hz - applied) <= RATE / 8192
        ks.append(k); residues.append(want_hz - applied)

    def one(k, block=1 << 18):                                                 # in blocks that stay in the cache: the cut changes nothing
        parts, hist = [], None
        for p in range(0, len(x), block):
            out, hist = dr.ddc(x[p:p + block], taps, L, M, k, p, hist)
            parts.append(out)
        return np.concatenate(parts)
    with ThreadPoolExecutor(3) as ex:
        rows = list(ex.map(one, ks))
    out = np.stack(rows)
    out.setflags(write=False)
    return out, tuple(ks), tuple(residues)
