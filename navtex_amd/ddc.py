"""ctypes binding of libnavtex_amd_ddc.so, the down-converter bank (the C ABI in include/navtex_amd_ddc.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _companion, _native as N


OUTPUT_RATE, GRID, SCALE, GUARD_HZ = 252000, 4096, 32767, 25000
CS16, CU8, CS8, CF32 = 0, 1, 2, 3
BYTES_PER_SAMPLE = {CS16: 4, CU8: 2, CS8: 2, CF32: 8}
_DTYPES = {CS16: np.int16, CU8: np.uint8, CS8: np.int8, CF32: np.float32}


class Config(C.Structure):
    """nvx_ddc_config."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("n_inputs", C.c_int), ("n_slices", C.c_int),
                ("input_rate_hz", C.c_uint32), ("format", C.c_int)]


def _signatures() -> dict:
    vp, sz, i, u32, u64, dbl = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64, C.c_double
    ip, dp = C.POINTER(i), C.POINTER(dbl)
    return {
        "nvx_ddc_config_default": (None, [C.POINTER(Config)]),
        "nvx_ddc_create": (i, [C.POINTER(Config), C.POINTER(vp)]),
        "nvx_ddc_destroy": (None, [vp]),
        "nvx_ddc_grid": (i, [u32, dbl, ip, dp]),
        "nvx_ddc_table": (i, [vp, i]),
        "nvx_ddc_set_shift": (i, [vp, i, i, dbl, dp]),
        "nvx_ddc_get_shift": (i, [vp, i, i, ip, dp]),
        "nvx_ddc_resident": (i, [vp, vp, sz, sz, vp, sz, sz, C.POINTER(sz), vp]),
        "nvx_ddc_push": (i, [vp, i, vp, sz, vp, sz, C.POINTER(sz)]),
        "nvx_ddc_reset": (i, [vp, i]),
        "nvx_ddc_position": (i, [vp, i, C.POINTER(u64), C.POINTER(u64)]),
        "nvx_ddc_plan": (i, [vp, ip, ip, ip, ip, ip, ip]),
        "nvx_ddc_timing": (i, [vp, i]),
        "nvx_ddc_time_stats": (i, [vp, dp, C.POINTER(u64), i]),
        "nvx_ddc_last_error": (C.c_char_p, []),
        "nvx_ddc_debug_last_launch": (C.c_int64, [vp, ip, ip, ip, ip, ip, ip, ip, C.POINTER(sz)]),
        "nvx_ddc_debug_set_position": (i, [vp, i, u64]),
    }


lib = _companion.load("NAVTEX_AMD_DDC_LIB", "libnavtex_amd_ddc.so", _signatures())


DdcError, _check = _companion.errors("DdcError", __name__, lib.nvx_ddc_last_error)


def grid(input_rate_hz: int, hz: float) -> Tuple[int, float]:
    """nvx_ddc_grid: (k, applied Hz) of a requested shift; needs no device.  The residue hz - applied is nvx_set_carrier's."""
    k, applied = C.c_int(), C.c_double()
    _check(lib.nvx_ddc_grid(input_rate_hz, hz, C.byref(k), C.byref(applied)), "nvx_ddc_grid")
    return k.value, applied.value


def table() -> np.ndarray:
    """nvx_ddc_table: W as int16 [4096, 2] (c, s)."""
    w = np.empty((GRID, 2), dtype=np.int16)
    assert lib.nvx_ddc_table(N.as_ptr(w), GRID) == GRID
    return w


class Ddc(_companion.Handle):
    """nvx_ddc wrapper: n_inputs inputs at input_rate_hz in `format` -> n_slices packed int16 IQ rows at 252 kS/s each."""
    _destroy = lib.nvx_ddc_destroy

    def __init__(self, input_rate_hz: int, format: int = CU8, n_inputs: int = 1, n_slices: int = 1, device: int = 0):
        cfg = Config()
        lib.nvx_ddc_config_default(C.byref(cfg))
        cfg.device, cfg.n_inputs, cfg.n_slices, cfg.input_rate_hz, cfg.format = device, n_inputs, n_slices, input_rate_hz, format
        h = C.c_void_p()
        _check(lib.nvx_ddc_create(C.byref(cfg), C.byref(h)), "nvx_ddc_create")
        self._h = h
        self.device, self.n_inputs, self.n_slices, self.format, self.input_rate_hz = device, n_inputs, n_slices, format, input_rate_hz
        L, M, T = C.c_int(), C.c_int(), C.c_int()
        _check(lib.nvx_ddc_plan(h, C.byref(L), C.byref(M), C.byref(T), None, None, None), "nvx_ddc_plan")
        self.L, self.M, self.T = L.value, M.value, T.value

    def set_shift(self, slice: int, hz: float, input: int = -1) -> float:
        """nvx_ddc_set_shift: returns the grid frequency applied."""
        applied = C.c_double()
        _check(lib.nvx_ddc_set_shift(self._h, input, slice, hz, C.byref(applied)), "nvx_ddc_set_shift")
        return applied.value

    def get_shift(self, slice: int, input: int = 0) -> Tuple[int, float]:
        k, applied = C.c_int(), C.c_double()
        _check(lib.nvx_ddc_get_shift(self._h, input, slice, C.byref(k), C.byref(applied)), "nvx_ddc_get_shift")
        return k.value, applied.value

    def resident(self, d_in, pitch_in: int, n_in: int, d_out, pitch_out: int, out_first: int = 0, hip_stream: Optional[int] = None) -> int:
        """nvx_ddc_resident: d_in and d_out are DeviceBuffers; ordered on hip_stream, not waited for.  Returns the number of
        outputs written per slice."""
        n = C.c_size_t()
        _check(lib.nvx_ddc_resident(self._h, d_in.ptr, pitch_in, n_in, d_out.ptr, pitch_out, out_first, C.byref(n), hip_stream or None),
               "nvx_ddc_resident")
        return n.value

    def push(self, input: int, samples: np.ndarray) -> np.ndarray:
        """nvx_ddc_push: one input's samples ([n, 2] in the plan's format) -> int16 [n_slices, n_out, 2]."""
        a = np.ascontiguousarray(samples, dtype=_DTYPES[self.format]).reshape(-1, 2)
        consumed, produced = self.position(input)
        cap = -((-(consumed + a.shape[0]) * self.L) // self.M) - produced
        out = np.empty((self.n_slices, max(cap, 1), 2), dtype=np.int16)
        n = C.c_size_t()
        _check(lib.nvx_ddc_push(self._h, input, N.as_ptr(a) if a.size else N.as_ptr(out), a.shape[0], N.as_ptr(out), max(cap, 1), C.byref(n)),
               "nvx_ddc_push")
        return out[:, :n.value]

    def reset(self, input: int = -1) -> None:
        _check(lib.nvx_ddc_reset(self._h, input), "nvx_ddc_reset")

    def position(self, input: int = 0) -> Tuple[int, int]:
        """(input samples consumed, outputs produced per slice) of `input` since its reset."""
        c, p = C.c_uint64(), C.c_uint64()
        _check(lib.nvx_ddc_position(self._h, input, C.byref(c), C.byref(p)), "nvx_ddc_position")
        return c.value, p.value

    def timing(self, enable: bool = True) -> None:
        _check(lib.nvx_ddc_timing(self._h, int(enable)), "nvx_ddc_timing")

    def time_stats(self, reset: bool = False) -> Tuple[float, int]:
        s, n = C.c_double(), C.c_uint64()
        _check(lib.nvx_ddc_time_stats(self._h, C.byref(s), C.byref(n), int(reset)), "nvx_ddc_time_stats")
        return s.value, n.value

    def debug_last_launch(self) -> dict:
        """For tests (nvx_ddc_debug_last_launch): the shape of the last kernel launch as the host handed it over."""
        v = [C.c_int() for _ in range(7)]
        lds = C.c_size_t()
        n = _check(lib.nvx_ddc_debug_last_launch(self._h, *[C.byref(x) for x in v], C.byref(lds)), "nvx_ddc_debug_last_launch")
        names = ("K", "tiles", "tiles_per_chunk", "chunks", "slices", "inputs")
        return {"launches": n, **{k: x.value for k, x in zip(names, v)}, "taps_in_lds": bool(v[6].value), "lds_bytes": lds.value}

    def debug_set_position(self, consumed: int, input: int = -1) -> None:
        """For tests (nvx_ddc_debug_set_position): the input stands at `consumed` with silence in front."""
        _check(lib.nvx_ddc_debug_set_position(self._h, input, consumed), "nvx_ddc_debug_set_position")
