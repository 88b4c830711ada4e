"""ctypes binding of libnavtex_amd_align.so, the row aligner (the C ABI in include/navtex_amd_align.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _companion, _native as N


PHASES, TAPS, GROUP_DELAY = 32, 16, 7
MAX_DELAY_DEFAULT, MAX_DELAY_LIMIT, MIN_CONTRAST_DEFAULT = 4096, 1 << 20, 64
MAX_LAGS, MIN_WINDOW, COHERENCE_ONE = 8192, 1024, 16384
CS16, CU8, CS8, CF32 = 0, 1, 2, 3
BYTES_PER_SAMPLE = {CS16: 4, CU8: 2, CS8: 2, CF32: 8}
_DTYPES = {CS16: np.int16, CU8: np.uint8, CS8: np.int8, CF32: np.float32}


class Config(C.Structure):
    """nvx_align_config."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("format", C.c_int), ("n_pairs", C.c_int), ("max_delay", C.c_int),
                ("min_contrast", C.c_int)]


class Estimate(C.Structure):
    """nvx_align_estimate."""
    _fields_ = [("delay_q5", C.c_int32), ("reason", C.c_int32), ("coherence_q14", C.c_int32), ("peak_lag", C.c_int32), ("peak_power", C.c_uint64),
                ("median_power", C.c_uint64)]


def _signatures() -> dict:
    vp, sz, i, u64, i64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_int64
    ip, qp = C.POINTER(i), C.POINTER(u64)
    return {
        "nvx_align_config_default": (None, [C.POINTER(Config)]),
        "nvx_align_create": (i, [C.POINTER(Config), C.POINTER(vp)]),
        "nvx_align_destroy": (None, [vp]),
        "nvx_align_measure_resident": (i, [vp, i, vp, sz, vp, sz, sz, i, i, vp, vp, vp]),
        "nvx_align_window": (u64, [sz, i, i]),
        "nvx_align_find": (i, [vp, i, i, u64, i64, i64, i, C.POINTER(Estimate)]),
        "nvx_align_set_delay": (i, [vp, i, i]),
        "nvx_align_get_delay": (i, [vp, i, ip]),
        "nvx_align_resident": (i, [vp, vp, sz, vp, sz, sz, vp, sz, vp, sz, sz, vp]),
        "nvx_align_push": (i, [vp, i, vp, vp, sz, vp, vp]),
        "nvx_align_reset": (i, [vp, i]),
        "nvx_align_position": (i, [vp, i, qp]),
        "nvx_align_plan": (i, [vp, ip, ip, ip, ip]),
        "nvx_align_delay": (i, []),
        "nvx_align_taps": (i, [vp]),
        "nvx_align_timing": (i, [vp, i]),
        "nvx_align_time_stats": (i, [vp, C.POINTER(C.c_double), qp, i]),
        "nvx_align_last_error": (C.c_char_p, []),
        "nvx_align_debug_last_launch": (C.c_int64, [vp, ip, ip, ip]),
        "nvx_align_debug_set_position": (i, [vp, i, u64]),
    }


lib = _companion.load("NAVTEX_AMD_ALIGN_LIB", "libnavtex_amd_align.so", _signatures())


AlignError, _check = _companion.errors("AlignError", __name__, lib.nvx_align_last_error)


def taps() -> np.ndarray:
    """nvx_align_taps: the shipped taps, int16 [32, 16]; needs no device."""
    t = np.empty((PHASES, TAPS), dtype=np.int16)
    _check(lib.nvx_align_taps(N.as_ptr(t)), "nvx_align_taps")
    return t


def window(n_in: int, lag_first: int, n_lags: int) -> int:
    """nvx_align_window: N of a measurement, 0 where it is refused."""
    return lib.nvx_align_window(n_in, lag_first, n_lags)


def find(r: np.ndarray, lag_first: int, n_window: int, saa: int, sbb: int, min_contrast: int = MIN_CONTRAST_DEFAULT) -> dict:
    """nvx_align_find on one pair's table (int64 [n_lags, 2]); needs no device."""
    r = np.ascontiguousarray(r, dtype=np.int64).reshape(-1, 2)
    e = Estimate()
    _check(lib.nvx_align_find(N.as_ptr(r), lag_first, r.shape[0], n_window, saa, sbb, min_contrast, C.byref(e)), "nvx_align_find")
    return {"delay_q5": e.delay_q5, "reason": e.reason, "coherence_q14": e.coherence_q14, "peak_lag": e.peak_lag, "peak_power": e.peak_power,
            "median_power": e.median_power}


class Aligner(_companion.Handle):
    """nvx_row_aligner wrapper: n_pairs pairs of rows (main, sense) in `format` -> the same rows as packed int16 IQ at the same
    rate, moved against each other by each pair's delay."""
    _destroy = lib.nvx_align_destroy

    def __init__(self, format: int = CS16, n_pairs: int = 1, max_delay: int = MAX_DELAY_DEFAULT, min_contrast: int = MIN_CONTRAST_DEFAULT,
                 device: int = 0):
        cfg = Config()
        lib.nvx_align_config_default(C.byref(cfg))
        cfg.device, cfg.format, cfg.n_pairs, cfg.max_delay, cfg.min_contrast = device, format, n_pairs, max_delay, min_contrast
        h = C.c_void_p()
        _check(lib.nvx_align_create(C.byref(cfg), C.byref(h)), "nvx_align_create")
        self._h = h
        self.device, self.format, self.n_pairs, self.max_delay, self.min_contrast = device, format, n_pairs, max_delay, min_contrast

    def measure_resident(self, d_main, pitch_main: int, d_sense, pitch_sense: int, n_in: int, lag_first: int, n_lags: int,
                         format: Optional[int] = None, hip_stream: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """nvx_align_measure_resident: (R as int64 [n_pairs, n_lags, 2], (SAA, SBB) as int64 [n_pairs, 2]); waits."""
        r = np.zeros((self.n_pairs, max(n_lags, 0), 2), dtype=np.int64)
        p = np.zeros((self.n_pairs, 2), dtype=np.int64)
        _check(lib.nvx_align_measure_resident(self._h, self.format if format is None else format, d_main.ptr, pitch_main, d_sense.ptr, pitch_sense, n_in,
                                              lag_first, n_lags, N.as_ptr(r) if r.size else N.as_ptr(p), N.as_ptr(p), hip_stream or None),
               "nvx_align_measure_resident")
        return r, p

    def find(self, r: np.ndarray, lag_first: int, n_window: int, saa: int, sbb: int) -> dict:
        """nvx_align_find with the plan's min_contrast."""
        return find(r, lag_first, n_window, saa, sbb, self.min_contrast)

    def set_delay(self, delay_q5: int, pair: int = -1) -> None:
        """nvx_align_set_delay: from the next call's first sample on."""
        _check(lib.nvx_align_set_delay(self._h, pair, delay_q5), "nvx_align_set_delay")

    def get_delay(self, pair: int = 0) -> int:
        d = C.c_int()
        _check(lib.nvx_align_get_delay(self._h, pair, C.byref(d)), "nvx_align_get_delay")
        return d.value

    def resident(self, d_main, pitch_main: int, d_sense, pitch_sense: int, n_in: int, d_out_main, pitch_out_main: int, d_out_sense,
                 pitch_out_sense: int, out_first: int = 0, hip_stream: Optional[int] = None) -> None:
        """nvx_align_resident: the operands are DeviceBuffers; ordered on hip_stream, not waited for."""
        _check(lib.nvx_align_resident(self._h, d_main.ptr, pitch_main, d_sense.ptr, pitch_sense, n_in, d_out_main.ptr, pitch_out_main, d_out_sense.ptr,
                                      pitch_out_sense, out_first, hip_stream or None), "nvx_align_resident")

    def push(self, pair: int, main: np.ndarray, sense: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """nvx_align_push: one pair's samples ([n, 2] each, in the plan's format) -> two int16 [n, 2]."""
        a = np.ascontiguousarray(main, dtype=_DTYPES[self.format]).reshape(-1, 2)
        b = np.ascontiguousarray(sense, dtype=_DTYPES[self.format]).reshape(-1, 2)
        if a.shape != b.shape:
            raise ValueError(f"main has {a.shape[0]} samples, sense {b.shape[0]}")
        om = np.empty((max(a.shape[0], 1), 2), dtype=np.int16)
        os_ = np.empty((max(a.shape[0], 1), 2), dtype=np.int16)
        _check(lib.nvx_align_push(self._h, pair, N.as_ptr(a) if a.size else N.as_ptr(om), N.as_ptr(b) if b.size else N.as_ptr(om), a.shape[0],
                                  N.as_ptr(om), N.as_ptr(os_)), "nvx_align_push")
        return om[:a.shape[0]], os_[:a.shape[0]]

    def reset(self, pair: int = -1) -> None:
        _check(lib.nvx_align_reset(self._h, pair), "nvx_align_reset")

    def position(self, pair: int = 0) -> int:
        """Samples consumed by `pair` since its reset."""
        c = C.c_uint64()
        _check(lib.nvx_align_position(self._h, pair, C.byref(c)), "nvx_align_position")
        return c.value

    def timing(self, enable: bool = True) -> None:
        _check(lib.nvx_align_timing(self._h, int(enable)), "nvx_align_timing")

    def time_stats(self, reset: bool = False) -> Tuple[float, int]:
        s, n = C.c_double(), C.c_uint64()
        _check(lib.nvx_align_time_stats(self._h, C.byref(s), C.byref(n), int(reset)), "nvx_align_time_stats")
        return s.value, n.value

    def debug_last_launch(self) -> dict:
        """For tests (nvx_align_debug_last_launch): the shape of the last apply as the host handed it over."""
        chunks, tpc, form = C.c_int(), C.c_int(), C.c_int()
        n = _check(lib.nvx_align_debug_last_launch(self._h, C.byref(chunks), C.byref(tpc), C.byref(form)), "nvx_align_debug_last_launch")
        return {"launches": n, "chunks": chunks.value, "tiles_per_chunk": tpc.value, "form": form.value}

    def debug_set_position(self, position: int, pair: int = -1) -> None:
        """For tests (nvx_align_debug_set_position)."""
        _check(lib.nvx_align_debug_set_position(self._h, pair, position), "nvx_align_debug_set_position")
