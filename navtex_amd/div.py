"""ctypes binding of libnavtex_amd_div.so, the diversity combiner (the C ABI in include/navtex_amd_div.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _companion, _native as N


BLOCK, CELL = 256, 65536
MAX_TARGETS = 4
WINDOW_LOG2_DEFAULT = 2
W_ONE, W_MAX, COHERENCE_ONE = 8192, 32767, 16384
TRACK, HOLD = 0, 1
CS16, CU8, CS8, CF32 = 0, 1, 2, 3
BYTES_PER_SAMPLE = {CS16: 4, CU8: 2, CS8: 2, CF32: 8}
_DTYPES = {CS16: np.int16, CU8: np.uint8, CS8: np.int8, CF32: np.float32}


class Config(C.Structure):
    """nvx_div_config."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("format", C.c_int), ("n_pairs", C.c_int), ("n_targets", C.c_int),
                ("window_log2", C.c_int)]


class Status(C.Structure):
    """nvx_div_status."""
    _fields_ = [("lead", C.c_int32), ("w_re", C.c_int32), ("w_im", C.c_int32), ("mode", C.c_int32), ("last_reason", C.c_int32),
                ("coherence_q14", C.c_int32), ("sums", C.c_int64 * 4), ("step", C.c_uint32), ("reserved", C.c_uint32), ("samples", C.c_uint64),
                ("cells_solved", C.c_uint64), ("cells_rejected", C.c_uint64)]


def _signatures() -> dict:
    vp, sz, i, u32, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64
    ip, qp = C.POINTER(i), C.POINTER(u64)
    return {
        "nvx_div_config_default": (None, [C.POINTER(Config)]),
        "nvx_div_create": (i, [C.POINTER(Config), C.POINTER(vp)]),
        "nvx_div_destroy": (None, [vp]),
        "nvx_div_resident": (i, [vp, vp, sz, vp, sz, sz, vp, sz, sz, vp]),
        "nvx_div_push": (i, [vp, i, vp, vp, sz, vp]),
        "nvx_div_set_freq": (i, [vp, i, i, u32]),
        "nvx_div_set": (i, [vp, i, i, i, i, i]),
        "nvx_div_set_mode": (i, [vp, i, i, i]),
        "nvx_div_reset": (i, [vp, i]),
        "nvx_div_get": (i, [vp, i, i, C.POINTER(Status)]),
        "nvx_div_position": (i, [vp, i, qp]),
        "nvx_div_plan": (i, [vp, ip, ip, ip, ip]),
        "nvx_div_step_from_hz": (u32, [C.c_double, C.c_double]),
        "nvx_div_hz_from_step": (C.c_double, [u32, C.c_double]),
        "nvx_div_timing": (i, [vp, i]),
        "nvx_div_time_stats": (i, [vp, C.POINTER(C.c_double), qp, i]),
        "nvx_div_last_error": (C.c_char_p, []),
        "nvx_div_debug_last_launch": (C.c_int64, [vp, ip, ip, ip, ip]),
        "nvx_div_debug_set_position": (i, [vp, i, u64]),
    }


lib = _companion.load("NAVTEX_AMD_DIV_LIB", "libnavtex_amd_div.so", _signatures())


DivError, _check = _companion.errors("DivError", __name__, lib.nvx_div_last_error)


def step_from_hz(hz: float, rate: float) -> int:
    return lib.nvx_div_step_from_hz(hz, rate)


def hz_from_step(step: int, rate: float) -> float:
    return lib.nvx_div_hz_from_step(step, rate)


class Combiner(_companion.Handle):
    """nvx_diversity_combiner wrapper: n_pairs pairs of rows (main, second) in `format` -> n_targets rows of packed int16 IQ per
    pair at the same rate, the weaker row co-phased and added to the stronger one in each target's band."""
    _destroy = lib.nvx_div_destroy

    def __init__(self, format: int = CS16, n_pairs: int = 1, n_targets: int = 1, window_log2: int = WINDOW_LOG2_DEFAULT, device: int = 0):
        cfg = Config()
        lib.nvx_div_config_default(C.byref(cfg))
        cfg.device, cfg.format, cfg.n_pairs, cfg.n_targets, cfg.window_log2 = device, format, n_pairs, n_targets, window_log2
        h = C.c_void_p()
        _check(lib.nvx_div_create(C.byref(cfg), C.byref(h)), "nvx_div_create")
        self._h = h
        self.device, self.format, self.n_pairs, self.n_targets, self.window_log2 = device, format, n_pairs, n_targets, window_log2

    def resident(self, d_main, pitch_main: int, d_second, pitch_second: int, n_in: int, d_out, pitch_out: int, out_first: int = 0,
                 hip_stream: Optional[int] = None) -> None:
        """nvx_div_resident: d_main, d_second and d_out are DeviceBuffers; ordered on hip_stream, not waited for."""
        _check(lib.nvx_div_resident(self._h, d_main.ptr, pitch_main, d_second.ptr, pitch_second, n_in, d_out.ptr, pitch_out, out_first, hip_stream or None),
               "nvx_div_resident")

    def push(self, pair: int, main: np.ndarray, second: np.ndarray) -> np.ndarray:
        """nvx_div_push: one pair's samples ([n, 2] each, in the plan's format) -> int16 [n_targets, n, 2]."""
        a = np.ascontiguousarray(main, dtype=_DTYPES[self.format]).reshape(-1, 2)
        b = np.ascontiguousarray(second, dtype=_DTYPES[self.format]).reshape(-1, 2)
        if a.shape != b.shape:
            raise ValueError(f"main has {a.shape[0]} samples, second {b.shape[0]}")
        n = a.shape[0]
        out = np.empty((self.n_targets * max(n, 1), 2), dtype=np.int16)
        _check(lib.nvx_div_push(self._h, pair, N.as_ptr(a) if a.size else N.as_ptr(out), N.as_ptr(b) if b.size else N.as_ptr(out), n, N.as_ptr(out)),
               "nvx_div_push")
        return out[:self.n_targets * n].reshape(self.n_targets, n, 2)

    def set_freq(self, target: int, step: int, pair: int = -1) -> None:
        """nvx_div_set_freq: the target's phase step from the next call's first sample on; the target starts anew."""
        _check(lib.nvx_div_set_freq(self._h, pair, target, step & 0xffffffff), "nvx_div_set_freq")

    def set(self, target: int, lead: int, w_re: int, w_im: int, pair: int = -1) -> None:
        """nvx_div_set: lead and weight (Q13) from the next call's first sample on."""
        _check(lib.nvx_div_set(self._h, pair, target, lead, w_re, w_im), "nvx_div_set")

    def set_mode(self, target: int, mode: int, pair: int = -1) -> None:
        _check(lib.nvx_div_set_mode(self._h, pair, target, mode), "nvx_div_set_mode")

    def reset(self, pair: int = -1) -> None:
        _check(lib.nvx_div_reset(self._h, pair), "nvx_div_reset")

    def get(self, pair: int = 0, target: int = 0) -> dict:
        """nvx_div_get: lead, the weight (w_re, w_im), the mode, the last reason and its coherence, the window's four sums, the
        step, the counters."""
        s = Status()
        _check(lib.nvx_div_get(self._h, pair, target, C.byref(s)), "nvx_div_get")
        return {"lead": s.lead, "weight": (s.w_re, s.w_im), "mode": s.mode, "last_reason": s.last_reason, "coherence_q14": s.coherence_q14,
                "sums": tuple(s.sums), "step": s.step, "samples": s.samples, "cells_solved": s.cells_solved, "cells_rejected": s.cells_rejected}

    def position(self, pair: int = 0) -> int:
        """Samples consumed by `pair` since its reset."""
        c = C.c_uint64()
        _check(lib.nvx_div_position(self._h, pair, C.byref(c)), "nvx_div_position")
        return c.value

    def timing(self, enable: bool = True) -> None:
        _check(lib.nvx_div_timing(self._h, int(enable)), "nvx_div_timing")

    def time_stats(self, reset: bool = False) -> Tuple[float, int]:
        s, n = C.c_double(), C.c_uint64()
        _check(lib.nvx_div_time_stats(self._h, C.byref(s), C.byref(n), int(reset)), "nvx_div_time_stats")
        return s.value, n.value

    def debug_last_launch(self) -> dict:
        """For tests (nvx_div_debug_last_launch): the shape of the last call as the host handed it over."""
        chunks, tpc, rec, form = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        n = _check(lib.nvx_div_debug_last_launch(self._h, C.byref(chunks), C.byref(tpc), C.byref(rec), C.byref(form)), "nvx_div_debug_last_launch")
        return {"launches": n, "chunks": chunks.value, "tiles_per_chunk": tpc.value, "records": rec.value, "form": form.value}

    def debug_set_position(self, position: int, pair: int = -1) -> None:
        """For tests (nvx_div_debug_set_position)."""
        _check(lib.nvx_div_debug_set_position(self._h, pair, position), "nvx_div_debug_set_position")
