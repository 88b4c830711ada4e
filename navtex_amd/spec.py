"""ctypes binding of libnavtex_amd_spec.so, the spectrum monitor (the C ABI in include/navtex_amd_spec.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

from . import _companion, _native as N


LOG2_MIN, LOG2_MAX, LOG2_DEFAULT = 8, 12, 11
AVG_DEFAULT = 8
MAX_HOP = 65536
LEVEL_ZERO = 991 << 8
CS16, CU8, CS8, CF32 = 0, 1, 2, 3
BYTES_PER_SAMPLE = {CS16: 4, CU8: 2, CS8: 2, CF32: 8}
_DTYPES = {CS16: np.int16, CU8: np.uint8, CS8: np.int8, CF32: np.float32}


class Config(C.Structure):
    """nvx_spec_config."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("format", C.c_int), ("n_rows", C.c_int), ("n_log2", C.c_int), ("avg", C.c_int)]


class Params(C.Structure):
    """nvx_spec_params."""
    _fields_ = [("struct_size", C.c_uint32), ("guard_bins", C.c_int), ("min_lines", C.c_int), ("reserved", C.c_int), ("min_coherence", C.c_double),
                ("min_score_db", C.c_double)]


class Hit(C.Structure):
    """nvx_spec_hit."""
    _fields_ = [("cycles_per_sample", C.c_double), ("coherence", C.c_double), ("score_db", C.c_double), ("step", C.c_uint32), ("bin", C.c_int)]


def _signatures() -> dict:
    vp, sz, i, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64
    ip, qp, dp = C.POINTER(i), C.POINTER(u64), C.POINTER(C.c_double)
    return {
        "nvx_spec_config_default": (None, [C.POINTER(Config)]),
        "nvx_spec_create": (i, [C.POINTER(Config), C.POINTER(vp)]),
        "nvx_spec_destroy": (None, [vp]),
        "nvx_spec_lines_for": (C.c_int64, [vp, i, sz]),
        "nvx_spec_resident": (i, [vp, vp, sz, sz, vp, sz, vp]),
        "nvx_spec_push": (i, [vp, i, vp, sz, vp, sz]),
        "nvx_spec_reset": (i, [vp, i]),
        "nvx_spec_measure": (i, [vp, i]),
        "nvx_spec_get": (i, [vp, i, vp, vp, vp, qp]),
        "nvx_spec_position": (i, [vp, i, qp]),
        "nvx_spec_plan": (i, [vp, ip, ip, ip, ip]),
        "nvx_spec_params_default": (None, [C.POINTER(Params)]),
        "nvx_spec_find_lines": (i, [vp, vp, vp, i, i, u64, C.POINTER(Params), C.POINTER(Hit), i]),
        "nvx_spec_timing": (i, [vp, i]),
        "nvx_spec_time_stats": (i, [vp, dp, qp, i]),
        "nvx_spec_last_error": (C.c_char_p, []),
        "nvx_spec_debug_last_launch": (C.c_int64, [vp, ip, ip, ip, ip]),
        "nvx_spec_debug_set_position": (i, [vp, i, u64]),
        "nvx_spec_debug_set_scratch": (i, [vp, sz]),
    }


lib = _companion.load("NAVTEX_AMD_SPEC_LIB", "libnavtex_amd_spec.so", _signatures())


SpecError, _check = _companion.errors("SpecError", __name__, lib.nvx_spec_last_error)


def level_db(words) -> np.ndarray:
    """NVX_SPEC_LEVEL_DB: level words -> dB."""
    return 3.010299956639812 * (np.asarray(words, dtype=np.float64) / 256.0 - 32.0)


def find_lines(power: np.ndarray, lag_re: np.ndarray, lag_im: np.ndarray, n_log2: int, avg: int, lines: int, cap: int = 64, **params) -> List[dict]:
    """nvx_spec_find_lines: a survey -> the steady lines in it, in the order kept (host only, needs no device).  Keyword
    arguments override the defaults of nvx_spec_params."""
    p = Params()
    lib.nvx_spec_params_default(C.byref(p))
    for k, v in params.items():
        if not hasattr(p, k):
            raise TypeError(f"nvx_spec_params has no {k}")
        setattr(p, k, v)
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (power, lag_re, lag_im)]
    if any(a.shape != (1 << n_log2,) for a in arrays):
        raise ValueError("power, lag_re and lag_im are [2^n_log2] each")
    hits = (Hit * max(cap, 1))()
    n = lib.nvx_spec_find_lines(N.as_ptr(arrays[0]), N.as_ptr(arrays[1]), N.as_ptr(arrays[2]), n_log2, avg, lines, C.byref(p), hits, cap)
    if n < 0:
        raise SpecError(n, "nvx_spec_find_lines")
    return [dict(cycles_per_sample=h.cycles_per_sample, step=h.step, coherence=h.coherence, score_db=h.score_db, bin=h.bin) for h in hits[:min(n, cap)]]


class Spectrum(_companion.Handle):
    """nvx_spectrum wrapper: n_rows rows in `format` -> waterfall lines of N = 2^n_log2 level words per row, `avg` half-overlapped
    segments to a line, and a survey per row for find_lines."""
    _destroy = lib.nvx_spec_destroy

    def __init__(self, format: int = CS16, n_rows: int = 1, n_log2: int = LOG2_DEFAULT, avg: int = AVG_DEFAULT, device: int = 0):
        cfg = Config()
        lib.nvx_spec_config_default(C.byref(cfg))
        cfg.device, cfg.format, cfg.n_rows, cfg.n_log2, cfg.avg = device, format, n_rows, n_log2, avg
        h = C.c_void_p()
        _check(lib.nvx_spec_create(C.byref(cfg), C.byref(h)), "nvx_spec_create")
        self._h = h
        self.device, self.format, self.n_rows, self.n_log2, self.avg, self.n = device, format, n_rows, n_log2, avg, 1 << n_log2

    def lines_for(self, n_in: int, row: int = 0) -> int:
        return _check(lib.nvx_spec_lines_for(self._h, row, n_in), "nvx_spec_lines_for")

    def resident(self, d_in, pitch_in: int, n_in: int, d_levels=None, line_cap: int = 0, hip_stream: Optional[int] = None) -> int:
        """nvx_spec_resident: d_in and d_levels (None: survey only) are DeviceBuffers; ordered on hip_stream, not waited for.
        Returns the lines completed per row."""
        return _check(lib.nvx_spec_resident(self._h, d_in.ptr, pitch_in, n_in, d_levels.ptr if d_levels is not None else None, line_cap,
                                            hip_stream or None), "nvx_spec_resident")

    def push(self, row: int, samples: np.ndarray, levels: bool = True) -> np.ndarray:
        """nvx_spec_push: one row's samples ([n, 2], in the plan's format) -> uint16 [lines, N] (levels=False: survey only,
        [lines, 0])."""
        a = np.ascontiguousarray(samples, dtype=_DTYPES[self.format]).reshape(-1, 2)
        cap = self.lines_for(a.shape[0], row)
        out = np.empty((max(cap, 1), self.n), dtype=np.uint16)
        n = _check(lib.nvx_spec_push(self._h, row, N.as_ptr(a) if a.size else N.as_ptr(out), a.shape[0], N.as_ptr(out) if levels else None, cap),
                   "nvx_spec_push")
        return out[:n] if levels else out[:n, :0]

    def reset(self, row: int = -1) -> None:
        _check(lib.nvx_spec_reset(self._h, row), "nvx_spec_reset")

    def measure(self, row: int = -1) -> None:
        _check(lib.nvx_spec_measure(self._h, row), "nvx_spec_measure")

    def get(self, row: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
        """nvx_spec_get: (power, lag_re, lag_im, lines) of the row's survey; waits for the device."""
        p, re, im = (np.empty(self.n, dtype=np.float64) for _ in range(3))
        lines = C.c_uint64()
        _check(lib.nvx_spec_get(self._h, row, N.as_ptr(p), N.as_ptr(re), N.as_ptr(im), C.byref(lines)), "nvx_spec_get")
        return p, re, im, lines.value

    def find_lines(self, row: int = 0, cap: int = 64, **params) -> List[dict]:
        p, re, im, lines = self.get(row)
        return find_lines(p, re, im, self.n_log2, self.avg, lines, cap, **params)

    def position(self, row: int = 0) -> int:
        """Samples consumed by `row` since its reset."""
        c = C.c_uint64()
        _check(lib.nvx_spec_position(self._h, row, C.byref(c)), "nvx_spec_position")
        return c.value

    def timing(self, enable: bool = True) -> None:
        _check(lib.nvx_spec_timing(self._h, int(enable)), "nvx_spec_timing")

    def time_stats(self, reset: bool = False) -> Tuple[float, int]:
        s, n = C.c_double(), C.c_uint64()
        _check(lib.nvx_spec_time_stats(self._h, C.byref(s), C.byref(n), int(reset)), "nvx_spec_time_stats")
        return s.value, n.value

    def debug_last_launch(self) -> dict:
        """For tests (nvx_spec_debug_last_launch): the shape of the last call as the host handed it over."""
        lines, per, batches, carried = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        n = _check(lib.nvx_spec_debug_last_launch(self._h, C.byref(lines), C.byref(per), C.byref(batches), C.byref(carried)), "nvx_spec_debug_last_launch")
        return {"launches": n, "lines": lines.value, "batch_lines": per.value, "batches": batches.value, "carried": carried.value}

    def debug_set_position(self, position: int, row: int = -1) -> None:
        """For tests (nvx_spec_debug_set_position)."""
        _check(lib.nvx_spec_debug_set_position(self._h, row, position), "nvx_spec_debug_set_position")

    def debug_set_scratch(self, nbytes: int) -> None:
        """For tests (nvx_spec_debug_set_scratch)."""
        _check(lib.nvx_spec_debug_set_scratch(self._h, nbytes), "nvx_spec_debug_set_scratch")
