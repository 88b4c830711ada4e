"""ctypes binding of libnavtex_amd_zoom.so, the zoom bank (the C ABI in include/navtex_amd_zoom.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _companion, _native as N


GRID, KZ_MIN, KZ_MAX = 4096, -2048, 2047
MAX_ZOOMS, MIN_LOG2, MAX_LOG2 = 8, 1, 6
STAGE_REACH, STAGE_DELAY = 53, 26
BLOCK = 1024                             # input samples a workgroup takes per step (navtex_amd/zoom/nvx_zoom_plan.h)
CS16, CU8, CS8, CF32 = 0, 1, 2, 3
BYTES_PER_SAMPLE = {CS16: 4, CU8: 2, CS8: 2, CF32: 8}
_DTYPES = {CS16: np.int16, CU8: np.uint8, CS8: np.int8, CF32: np.float32}


def history(k: int) -> int:
    """H: the input samples in front of a call its outputs depend on."""
    return STAGE_REACH * ((1 << k) - 1)


def tile(k: int) -> int:
    """T: the outputs of a tile."""
    return BLOCK >> k


class Config(C.Structure):
    """nvx_zoom_config."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("n_inputs", C.c_int), ("n_zooms", C.c_int), ("log2_decim", C.c_int),
                ("format", C.c_int)]


def _signatures() -> dict:
    vp, sz, i, u64, dbl = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_double
    ip, dp, qp = C.POINTER(i), C.POINTER(dbl), C.POINTER(u64)
    return {
        "nvx_zoom_config_default": (None, [C.POINTER(Config)]),
        "nvx_zoom_create": (i, [C.POINTER(Config), C.POINTER(vp)]),
        "nvx_zoom_destroy": (None, [vp]),
        "nvx_zoom_grid": (i, [dbl, dbl, ip, dp]),
        "nvx_zoom_set_shift": (i, [vp, i, i, i]),
        "nvx_zoom_get_shift": (i, [vp, i, i, ip]),
        "nvx_zoom_resident": (i, [vp, vp, sz, sz, vp, sz, sz, C.POINTER(sz), vp]),
        "nvx_zoom_push": (i, [vp, i, vp, sz, vp, sz, C.POINTER(sz)]),
        "nvx_zoom_reset": (i, [vp, i]),
        "nvx_zoom_position": (i, [vp, i, qp, qp]),
        "nvx_zoom_plan": (i, [vp, ip, ip, ip, ip, ip]),
        "nvx_zoom_taps": (i, [C.POINTER(C.c_int16), i, ip, ip]),
        "nvx_zoom_timing": (i, [vp, i]),
        "nvx_zoom_time_stats": (i, [vp, dp, qp, i]),
        "nvx_zoom_last_error": (C.c_char_p, []),
        "nvx_zoom_debug_last_launch": (C.c_int64, [vp, ip, ip, ip, ip, C.POINTER(sz)]),
        "nvx_zoom_debug_set_position": (i, [vp, i, u64]),
    }


lib = _companion.load("NAVTEX_AMD_ZOOM_LIB", "libnavtex_amd_zoom.so", _signatures())


ZoomError, _check = _companion.errors("ZoomError", __name__, lib.nvx_zoom_last_error)


def grid(rate_hz: float, hz: float) -> Tuple[int, float]:
    """nvx_zoom_grid: (kz, applied Hz) of a wanted shift at a rate; needs no device.  The residue hz - applied is the next
    stage's (nvx_ddc_set_shift, nvx_set_carrier)."""
    kz, applied = C.c_int(), C.c_double()
    _check(lib.nvx_zoom_grid(rate_hz, hz, C.byref(kz), C.byref(applied)), "nvx_zoom_grid")
    return kz.value, applied.value


def taps() -> Tuple[Tuple[int, ...], int, int]:
    """nvx_zoom_taps: (A[0 .. 13], a stage's reach, its shift).  Needs no device."""
    a, reach, shift = (C.c_int16 * 32)(), C.c_int(), C.c_int()
    n = _check(lib.nvx_zoom_taps(a, 32, C.byref(reach), C.byref(shift)), "nvx_zoom_taps")
    return tuple(a[:n]), reach.value, shift.value


class Zoom(_companion.Handle):
    """nvx_zoom wrapper: n_inputs inputs in `format` -> n_zooms packed int16 IQ rows each at 1 / 2^log2_decim of the rate."""
    _destroy = lib.nvx_zoom_destroy

    def __init__(self, log2_decim: int, format: int = CS16, n_inputs: int = 1, n_zooms: int = 1, device: int = 0):
        cfg = Config()
        lib.nvx_zoom_config_default(C.byref(cfg))
        cfg.device, cfg.n_inputs, cfg.n_zooms, cfg.log2_decim, cfg.format = device, n_inputs, n_zooms, log2_decim, format
        h = C.c_void_p()
        _check(lib.nvx_zoom_create(C.byref(cfg), C.byref(h)), "nvx_zoom_create")
        self._h = h
        self.device, self.n_inputs, self.n_zooms, self.log2_decim, self.format = device, n_inputs, n_zooms, log2_decim, format
        self.decim = 1 << log2_decim

    def set_step(self, zoom: int, kz: int, input: int = -1) -> None:
        """nvx_zoom_set_shift: the shift as a table step."""
        _check(lib.nvx_zoom_set_shift(self._h, input, zoom, kz), "nvx_zoom_set_shift")

    def set_shift(self, zoom: int, hz: float, rate_hz: float, input: int = -1) -> float:
        """The frequency hz of an input at rate_hz becomes the zoom's centre; returns the grid frequency applied."""
        kz, applied = grid(rate_hz, hz)
        self.set_step(zoom, kz, input)
        return applied

    def get_step(self, zoom: int, input: int = 0) -> int:
        kz = C.c_int()
        _check(lib.nvx_zoom_get_shift(self._h, input, zoom, C.byref(kz)), "nvx_zoom_get_shift")
        return kz.value

    def get_shift(self, zoom: int, rate_hz: float, input: int = 0) -> Tuple[int, float]:
        kz = self.get_step(zoom, input)
        return kz, kz * rate_hz / GRID

    def resident(self, d_in, pitch_in: int, n_in: int, d_out, pitch_out: int, out_first: int = 0, hip_stream: Optional[int] = None) -> int:
        """nvx_zoom_resident: d_in and d_out are DeviceBuffers; n_in a multiple of 2^log2_decim; ordered on hip_stream, not
        waited for.  Returns the number of outputs written per zoom."""
        n = C.c_size_t()
        _check(lib.nvx_zoom_resident(self._h, d_in.ptr, pitch_in, n_in, d_out.ptr, pitch_out, out_first, C.byref(n), hip_stream or None),
               "nvx_zoom_resident")
        return n.value

    def push(self, input: int, samples: np.ndarray) -> np.ndarray:
        """nvx_zoom_push: one input's samples ([n, 2] in the plan's format, any n) -> int16 [n_zooms, n_out, 2]."""
        a = np.ascontiguousarray(samples, dtype=_DTYPES[self.format]).reshape(-1, 2)
        cap = a.shape[0] // self.decim + 1
        out = np.empty((self.n_zooms, cap, 2), dtype=np.int16)
        n = C.c_size_t()
        _check(lib.nvx_zoom_push(self._h, input, N.as_ptr(a) if a.size else N.as_ptr(out), a.shape[0], N.as_ptr(out), cap, C.byref(n)), "nvx_zoom_push")
        return out[:, :n.value]

    def reset(self, input: int = -1) -> None:
        _check(lib.nvx_zoom_reset(self._h, input), "nvx_zoom_reset")

    def position(self, input: int = 0) -> Tuple[int, int]:
        """(input samples consumed, held ones included; outputs produced per zoom) of `input` since its reset."""
        c, p = C.c_uint64(), C.c_uint64()
        _check(lib.nvx_zoom_position(self._h, input, C.byref(c), C.byref(p)), "nvx_zoom_position")
        return c.value, p.value

    def plan(self) -> dict:
        v = [C.c_int() for _ in range(5)]
        _check(lib.nvx_zoom_plan(self._h, *[C.byref(x) for x in v]), "nvx_zoom_plan")
        return {k: x.value for k, x in zip(("format", "n_inputs", "n_zooms", "log2_decim", "history"), v)}

    def timing(self, enable: bool = True) -> None:
        _check(lib.nvx_zoom_timing(self._h, int(enable)), "nvx_zoom_timing")

    def time_stats(self, reset: bool = False) -> Tuple[float, int]:
        s, n = C.c_double(), C.c_uint64()
        _check(lib.nvx_zoom_time_stats(self._h, C.byref(s), C.byref(n), int(reset)), "nvx_zoom_time_stats")
        return s.value, n.value

    def debug_last_launch(self) -> dict:
        """For tests (nvx_zoom_debug_last_launch): the shape of the last call as the host handed it over."""
        v = [C.c_int() for _ in range(4)]
        lds = C.c_size_t()
        n = _check(lib.nvx_zoom_debug_last_launch(self._h, *[C.byref(x) for x in v], C.byref(lds)), "nvx_zoom_debug_last_launch")
        return {"launches": n, **{k: x.value for k, x in zip(("chunks", "tiles_per_chunk", "warm_tiles", "form"), v)}, "lds_bytes": lds.value}

    def debug_set_position(self, position: int, input: int = -1) -> None:
        """For tests (nvx_zoom_debug_set_position)."""
        _check(lib.nvx_zoom_debug_set_position(self._h, input, position), "nvx_zoom_debug_set_position")
