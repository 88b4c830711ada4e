"""ctypes binding of libnavtex_amd_blank.so, the impulse noise blanker (the C ABI in include/navtex_amd_blank.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _companion, _native as N


BLOCK = 1024
THR_DEFAULT, HOLD_DEFAULT, FLOOR_DEFAULT = 1024, 32, 64
CS16, CU8, CS8, CF32 = 0, 1, 2, 3
BYTES_PER_SAMPLE = {CS16: 4, CU8: 2, CS8: 2, CF32: 8}
_DTYPES = {CS16: np.int16, CU8: np.uint8, CS8: np.int8, CF32: np.float32}


class Config(C.Structure):
    """nvx_blank_config."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("format", C.c_int), ("n_streams", C.c_int), ("thr_q8", C.c_uint32),
                ("hold", C.c_uint32), ("floor", C.c_uint32)]


def _signatures() -> dict:
    vp, sz, i, u32, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64
    ip, up, qp = C.POINTER(i), C.POINTER(u32), C.POINTER(u64)
    return {
        "nvx_blank_config_default": (None, [C.POINTER(Config)]),
        "nvx_blank_create": (i, [C.POINTER(Config), C.POINTER(vp)]),
        "nvx_blank_destroy": (None, [vp]),
        "nvx_blank_resident": (i, [vp, vp, sz, sz, vp, sz, sz, vp]),
        "nvx_blank_push": (i, [vp, i, vp, sz, vp]),
        "nvx_blank_reset": (i, [vp, i]),
        "nvx_blank_position": (i, [vp, i, qp]),
        "nvx_blank_stats": (i, [vp, i, qp, qp, qp, i]),
        "nvx_blank_plan": (i, [vp, ip, ip, up, up, up]),
        "nvx_blank_timing": (i, [vp, i]),
        "nvx_blank_time_stats": (i, [vp, C.POINTER(C.c_double), qp, i]),
        "nvx_blank_last_error": (C.c_char_p, []),
        "nvx_blank_debug_last_launch": (C.c_int64, [vp, ip, ip, ip, ip]),
        "nvx_blank_debug_set_position": (i, [vp, i, u64]),
    }


lib = _companion.load("NAVTEX_AMD_BLANK_LIB", "libnavtex_amd_blank.so", _signatures())


BlankError, _check = _companion.errors("BlankError", __name__, lib.nvx_blank_last_error)


class Blanker(_companion.Handle):
    """nvx_blanker wrapper: n_streams streams in `format` -> packed int16 IQ at the same rate, impulsive samples zeroed."""
    _destroy = lib.nvx_blank_destroy

    def __init__(self, format: int = CS16, n_streams: int = 1, thr_q8: int = THR_DEFAULT, hold: int = HOLD_DEFAULT, floor: int = FLOOR_DEFAULT,
                 device: int = 0):
        cfg = Config()
        lib.nvx_blank_config_default(C.byref(cfg))
        cfg.device, cfg.format, cfg.n_streams, cfg.thr_q8, cfg.hold, cfg.floor = device, format, n_streams, thr_q8, hold, floor
        h = C.c_void_p()
        _check(lib.nvx_blank_create(C.byref(cfg), C.byref(h)), "nvx_blank_create")
        self._h = h
        self.device, self.format, self.n_streams, self.thr_q8, self.hold, self.floor = device, format, n_streams, thr_q8, hold, floor

    def resident(self, d_in, pitch_in: int, n_in: int, d_out, pitch_out: int, out_first: int = 0, hip_stream: Optional[int] = None) -> None:
        """nvx_blank_resident: d_in and d_out are DeviceBuffers; ordered on hip_stream, not waited for."""
        _check(lib.nvx_blank_resident(self._h, d_in.ptr, pitch_in, n_in, d_out.ptr, pitch_out, out_first, hip_stream or None), "nvx_blank_resident")

    def push(self, stream: int, samples: np.ndarray) -> np.ndarray:
        """nvx_blank_push: one stream's samples ([n, 2] in the plan's format) -> int16 [n, 2]."""
        a = np.ascontiguousarray(samples, dtype=_DTYPES[self.format]).reshape(-1, 2)
        out = np.empty((max(a.shape[0], 1), 2), dtype=np.int16)
        _check(lib.nvx_blank_push(self._h, stream, N.as_ptr(a) if a.size else N.as_ptr(out), a.shape[0], N.as_ptr(out)), "nvx_blank_push")
        return out[:a.shape[0]]

    def reset(self, stream: int = -1) -> None:
        _check(lib.nvx_blank_reset(self._h, stream), "nvx_blank_reset")

    def position(self, stream: int = 0) -> int:
        """Samples consumed by `stream` since its reset."""
        c = C.c_uint64()
        _check(lib.nvx_blank_position(self._h, stream, C.byref(c)), "nvx_blank_position")
        return c.value

    def stats(self, stream: int = 0, reset: bool = False) -> Tuple[int, int, int]:
        """(samples, detections, blanked samples) of `stream`."""
        s, d, g = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib.nvx_blank_stats(self._h, stream, C.byref(s), C.byref(d), C.byref(g), int(reset)), "nvx_blank_stats")
        return s.value, d.value, g.value

    def timing(self, enable: bool = True) -> None:
        _check(lib.nvx_blank_timing(self._h, int(enable)), "nvx_blank_timing")

    def time_stats(self, reset: bool = False) -> Tuple[float, int]:
        s, n = C.c_double(), C.c_uint64()
        _check(lib.nvx_blank_time_stats(self._h, C.byref(s), C.byref(n), int(reset)), "nvx_blank_time_stats")
        return s.value, n.value

    def debug_last_launch(self) -> dict:
        """For tests (nvx_blank_debug_last_launch): the shape of the last kernel launch as the host handed it over."""
        chunks, bpc, pre, form = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        n = _check(lib.nvx_blank_debug_last_launch(self._h, C.byref(chunks), C.byref(bpc), C.byref(pre), C.byref(form)), "nvx_blank_debug_last_launch")
        return {"launches": n, "chunks": chunks.value, "blocks_per_chunk": bpc.value, "preroll_blocks": pre.value, "form": form.value}

    def debug_set_position(self, position: int, stream: int = -1) -> None:
        """For tests (nvx_blank_debug_set_position)."""
        _check(lib.nvx_blank_debug_set_position(self._h, stream, position), "nvx_blank_debug_set_position")
