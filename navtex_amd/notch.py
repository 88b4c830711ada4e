"""ctypes binding of libnavtex_amd_notch.so, the tone notch (the C ABI in include/navtex_amd_notch.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _companion, _native as N


BLOCK = 256
MAX_NOTCHES = 4
WIDTH_LOG2_MIN, WIDTH_LOG2_MAX, WIDTH_LOG2_DEFAULT = 2, 6, 5
MAX_PAIRS = 4096
CS16, CU8, CS8, CF32 = 0, 1, 2, 3
BYTES_PER_SAMPLE = {CS16: 4, CU8: 2, CS8: 2, CF32: 8}
_DTYPES = {CS16: np.int16, CU8: np.uint8, CS8: np.int8, CF32: np.float32}


class Config(C.Structure):
    """nvx_notch_config."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("format", C.c_int), ("n_rows", C.c_int), ("n_notches", C.c_int),
                ("width_log2", C.c_int)]


class Status(C.Structure):
    """nvx_notch_status."""
    _fields_ = [("x_re", C.c_int64), ("x_im", C.c_int64), ("pairs", C.c_uint64), ("samples", C.c_uint64), ("step", C.c_uint32),
                ("enabled", C.c_int32)]


def _signatures() -> dict:
    vp, sz, i, u32, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64
    ip, qp = C.POINTER(i), C.POINTER(u64)
    return {
        "nvx_notch_config_default": (None, [C.POINTER(Config)]),
        "nvx_notch_create": (i, [C.POINTER(Config), C.POINTER(vp)]),
        "nvx_notch_destroy": (None, [vp]),
        "nvx_notch_resident": (i, [vp, vp, sz, sz, vp, sz, sz, vp]),
        "nvx_notch_push": (i, [vp, i, vp, sz, vp]),
        "nvx_notch_reset": (i, [vp, i]),
        "nvx_notch_set_freq": (i, [vp, i, i, u32]),
        "nvx_notch_enable": (i, [vp, i, i, i]),
        "nvx_notch_measure": (i, [vp, i, i]),
        "nvx_notch_refine": (i, [vp, i, i, C.POINTER(u32)]),
        "nvx_notch_get": (i, [vp, i, i, C.POINTER(Status)]),
        "nvx_notch_position": (i, [vp, i, qp]),
        "nvx_notch_plan": (i, [vp, ip, ip, ip, ip]),
        "nvx_notch_delay": (C.c_int64, [vp]),
        "nvx_notch_step_from_hz": (u32, [C.c_double, C.c_double]),
        "nvx_notch_hz_from_step": (C.c_double, [u32, C.c_double]),
        "nvx_notch_timing": (i, [vp, i]),
        "nvx_notch_time_stats": (i, [vp, C.POINTER(C.c_double), qp, i]),
        "nvx_notch_last_error": (C.c_char_p, []),
        "nvx_notch_debug_last_launch": (C.c_int64, [vp, ip, ip, ip, ip]),
        "nvx_notch_debug_set_position": (i, [vp, i, u64]),
    }


lib = _companion.load("NAVTEX_AMD_NOTCH_LIB", "libnavtex_amd_notch.so", _signatures())


NotchError, _check = _companion.errors("NotchError", __name__, lib.nvx_notch_last_error)


def step_from_hz(hz: float, rate: float) -> int:
    """nvx_notch_step_from_hz: the 32-bit phase step of a frequency at a sample rate."""
    return lib.nvx_notch_step_from_hz(hz, rate)


def hz_from_step(step: int, rate: float) -> float:
    """nvx_notch_hz_from_step."""
    return lib.nvx_notch_hz_from_step(step, rate)


class Notch(_companion.Handle):
    """nvx_tone_notch wrapper: n_rows rows in `format` -> packed int16 IQ at the same rate, delayed by delay() samples, the
    carriers of each row's enabled notches subtracted."""
    _destroy = lib.nvx_notch_destroy

    def __init__(self, format: int = CS16, n_rows: int = 1, n_notches: int = 1, width_log2: int = WIDTH_LOG2_DEFAULT, device: int = 0):
        cfg = Config()
        lib.nvx_notch_config_default(C.byref(cfg))
        cfg.device, cfg.format, cfg.n_rows, cfg.n_notches, cfg.width_log2 = device, format, n_rows, n_notches, width_log2
        h = C.c_void_p()
        _check(lib.nvx_notch_create(C.byref(cfg), C.byref(h)), "nvx_notch_create")
        self._h = h
        self.device, self.format, self.n_rows, self.n_notches, self.width_log2 = device, format, n_rows, n_notches, width_log2

    def resident(self, d_in, pitch_in: int, n_in: int, d_out, pitch_out: int, out_first: int = 0, hip_stream: Optional[int] = None) -> None:
        """nvx_notch_resident: d_in and d_out are DeviceBuffers; ordered on hip_stream, not waited for."""
        _check(lib.nvx_notch_resident(self._h, d_in.ptr, pitch_in, n_in, d_out.ptr, pitch_out, out_first, hip_stream or None), "nvx_notch_resident")

    def push(self, row: int, samples: np.ndarray) -> np.ndarray:
        """nvx_notch_push: one row's samples ([n, 2], in the plan's format) -> int16 [n, 2]."""
        a = np.ascontiguousarray(samples, dtype=_DTYPES[self.format]).reshape(-1, 2)
        out = np.empty((max(a.shape[0], 1), 2), dtype=np.int16)
        _check(lib.nvx_notch_push(self._h, row, N.as_ptr(a) if a.size else N.as_ptr(out), a.shape[0], N.as_ptr(out)), "nvx_notch_push")
        return out[:a.shape[0]]

    def reset(self, row: int = -1) -> None:
        _check(lib.nvx_notch_reset(self._h, row), "nvx_notch_reset")

    def set_freq(self, notch: int, step: int, row: int = -1) -> None:
        """nvx_notch_set_freq: the notch's step from the next call's first sample on."""
        _check(lib.nvx_notch_set_freq(self._h, row, notch, step & 0xffffffff), "nvx_notch_set_freq")

    def enable(self, notch: int, enable: bool = True, row: int = -1) -> None:
        _check(lib.nvx_notch_enable(self._h, row, notch, int(enable)), "nvx_notch_enable")

    def measure(self, notch: int, row: int = -1) -> None:
        _check(lib.nvx_notch_measure(self._h, row, notch), "nvx_notch_measure")

    def refine(self, notch: int, row: int = 0) -> int:
        """nvx_notch_refine: set_freq to where the offset readout points; the new step."""
        step = C.c_uint32()
        _check(lib.nvx_notch_refine(self._h, row, notch, C.byref(step)), "nvx_notch_refine")
        return step.value

    def get(self, notch: int = 0, row: int = 0) -> dict:
        """nvx_notch_get: X of the offset readout, its pair count, the step, the flag and the row's sample count."""
        s = Status()
        _check(lib.nvx_notch_get(self._h, row, notch, C.byref(s)), "nvx_notch_get")
        return {"x": (s.x_re, s.x_im), "pairs": s.pairs, "step": s.step, "enabled": bool(s.enabled), "samples": s.samples}

    def position(self, row: int = 0) -> int:
        """Samples consumed by `row` since its reset."""
        c = C.c_uint64()
        _check(lib.nvx_notch_position(self._h, row, C.byref(c)), "nvx_notch_position")
        return c.value

    def delay(self) -> int:
        return _check(lib.nvx_notch_delay(self._h), "nvx_notch_delay")

    def timing(self, enable: bool = True) -> None:
        _check(lib.nvx_notch_timing(self._h, int(enable)), "nvx_notch_timing")

    def time_stats(self, reset: bool = False) -> Tuple[float, int]:
        s, n = C.c_double(), C.c_uint64()
        _check(lib.nvx_notch_time_stats(self._h, C.byref(s), C.byref(n), int(reset)), "nvx_notch_time_stats")
        return s.value, n.value

    def debug_last_launch(self) -> dict:
        """For tests (nvx_notch_debug_last_launch): the shape of the last call as the host handed it over."""
        chunks, tpc, rec, form = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        n = _check(lib.nvx_notch_debug_last_launch(self._h, C.byref(chunks), C.byref(tpc), C.byref(rec), C.byref(form)), "nvx_notch_debug_last_launch")
        return {"launches": n, "chunks": chunks.value, "tiles_per_chunk": tpc.value, "records": rec.value, "form": form.value}

    def debug_set_position(self, position: int, row: int = -1) -> None:
        """For tests (nvx_notch_debug_set_position)."""
        _check(lib.nvx_notch_debug_set_position(self._h, row, position), "nvx_notch_debug_set_position")
