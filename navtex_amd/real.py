"""ctypes binding of libnavtex_amd_real.so, the real-input converter (the C ABI in include/navtex_amd_real.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _companion, _native as N


K, S = 13, 14
HISTORY = 2 * K + 2
TILE = 4096                              # outputs a workgroup takes per step (navtex_amd/real/nvx_real_plan.h)
S16, U8, S8, F32 = 0, 1, 2, 3
BYTES_PER_SAMPLE = {S16: 2, U8: 1, S8: 1, F32: 4}
_DTYPES = {S16: np.int16, U8: np.uint8, S8: np.int8, F32: np.float32}


class Config(C.Structure):
    """nvx_real_config."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("format", C.c_int), ("n_streams", C.c_int), ("invert", C.c_int)]


def _signatures() -> dict:
    vp, sz, i, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64
    ip, qp = C.POINTER(i), C.POINTER(u64)
    return {
        "nvx_real_config_default": (None, [C.POINTER(Config)]),
        "nvx_real_create": (i, [C.POINTER(Config), C.POINTER(vp)]),
        "nvx_real_destroy": (None, [vp]),
        "nvx_real_resident": (i, [vp, vp, sz, sz, vp, sz, sz, vp]),
        "nvx_real_push": (i, [vp, i, vp, sz, vp, sz, C.POINTER(sz)]),
        "nvx_real_reset": (i, [vp, i]),
        "nvx_real_position": (i, [vp, i, qp, qp]),
        "nvx_real_plan": (i, [vp, ip, ip, ip]),
        "nvx_real_taps": (i, [C.POINTER(C.c_int16), i, ip, ip]),
        "nvx_real_timing": (i, [vp, i]),
        "nvx_real_time_stats": (i, [vp, C.POINTER(C.c_double), qp, i]),
        "nvx_real_last_error": (C.c_char_p, []),
        "nvx_real_debug_last_launch": (C.c_int64, [vp, ip, ip, ip]),
        "nvx_real_debug_set_position": (i, [vp, i, u64]),
    }


lib = _companion.load("NAVTEX_AMD_REAL_LIB", "libnavtex_amd_real.so", _signatures())


RealError, _check = _companion.errors("RealError", __name__, lib.nvx_real_last_error)


def taps() -> Tuple[Tuple[int, ...], int, int]:
    """nvx_real_taps: (A[0 .. K], K, S).  Needs no device."""
    a, k, s = (C.c_int16 * 32)(), C.c_int(), C.c_int()
    n = _check(lib.nvx_real_taps(a, 32, C.byref(k), C.byref(s)), "nvx_real_taps")
    return tuple(a[:n]), k.value, s.value


class Converter(_companion.Handle):
    """nvx_real_converter wrapper: n_streams streams of real samples in `format` -> packed int16 IQ at half the rate, centred
    on a quarter of it."""
    _destroy = lib.nvx_real_destroy

    def __init__(self, format: int = S16, n_streams: int = 1, invert: int = 0, device: int = 0):
        cfg = Config()
        lib.nvx_real_config_default(C.byref(cfg))
        cfg.device, cfg.format, cfg.n_streams, cfg.invert = device, format, n_streams, invert
        h = C.c_void_p()
        _check(lib.nvx_real_create(C.byref(cfg), C.byref(h)), "nvx_real_create")
        self._h = h
        self.device, self.format, self.n_streams, self.invert = device, format, n_streams, invert

    def resident(self, d_in, pitch_in: int, n_in: int, d_out, pitch_out: int, out_first: int = 0, hip_stream: Optional[int] = None) -> None:
        """nvx_real_resident: d_in and d_out are DeviceBuffers; n_in even; ordered on hip_stream, not waited for."""
        _check(lib.nvx_real_resident(self._h, d_in.ptr, pitch_in, n_in, d_out.ptr, pitch_out, out_first, hip_stream or None), "nvx_real_resident")

    def push(self, stream: int, samples: np.ndarray) -> np.ndarray:
        """nvx_real_push: one stream's samples ([n] in the plan's format, any n) -> int16 [outputs, 2]."""
        a = np.ascontiguousarray(samples, dtype=_DTYPES[self.format]).reshape(-1)
        cap = a.shape[0] // 2 + 1
        out = np.empty((cap, 2), dtype=np.int16)
        n = C.c_size_t()
        _check(lib.nvx_real_push(self._h, stream, N.as_ptr(a) if a.size else N.as_ptr(out), a.shape[0], N.as_ptr(out), cap, C.byref(n)), "nvx_real_push")
        return out[:n.value]

    def reset(self, stream: int = -1) -> None:
        _check(lib.nvx_real_reset(self._h, stream), "nvx_real_reset")

    def position(self, stream: int = 0) -> Tuple[int, int]:
        """(samples consumed by `stream` since its reset, outputs produced)."""
        c, p = C.c_uint64(), C.c_uint64()
        _check(lib.nvx_real_position(self._h, stream, C.byref(c), C.byref(p)), "nvx_real_position")
        return c.value, p.value

    def timing(self, enable: bool = True) -> None:
        _check(lib.nvx_real_timing(self._h, int(enable)), "nvx_real_timing")

    def time_stats(self, reset: bool = False) -> Tuple[float, int]:
        s, n = C.c_double(), C.c_uint64()
        _check(lib.nvx_real_time_stats(self._h, C.byref(s), C.byref(n), int(reset)), "nvx_real_time_stats")
        return s.value, n.value

    def debug_last_launch(self) -> dict:
        """For tests (nvx_real_debug_last_launch): the shape of the last call as the host handed it over."""
        chunks, tpc, form = C.c_int(), C.c_int(), C.c_int()
        n = _check(lib.nvx_real_debug_last_launch(self._h, C.byref(chunks), C.byref(tpc), C.byref(form)), "nvx_real_debug_last_launch")
        return {"launches": n, "chunks": chunks.value, "tiles_per_chunk": tpc.value, "form": form.value}

    def debug_set_position(self, position: int, stream: int = -1) -> None:
        """For tests (nvx_real_debug_set_position)."""
        _check(lib.nvx_real_debug_set_position(self._h, stream, position), "nvx_real_debug_set_position")
