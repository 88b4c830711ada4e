"""ctypes binding of libnavtex_amd_tap.so, the channel tap (the C ABI in include/navtex_amd_tap.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _companion, _native as N


INPUT_RATE = 252000
S = 21
GRID = 4096
IQ, REAL = 0, 1
OUT_BYTES = {IQ: 4, REAL: 2}


class Config(C.Structure):
    """nvx_tap_config."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("n_inputs", C.c_int), ("n_taps", C.c_int), ("output_rate_hz", C.c_uint32),
                ("kind", C.c_int)]


def _signatures() -> dict:
    vp, sz, i, u32, u64, dbl = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64, C.c_double
    ip, qp, zp, dp = C.POINTER(i), C.POINTER(u64), C.POINTER(sz), C.POINTER(dbl)
    return {
        "nvx_tap_config_default": (None, [C.POINTER(Config)]),
        "nvx_tap_create": (i, [C.POINTER(Config), C.POINTER(vp)]),
        "nvx_tap_destroy": (None, [vp]),
        "nvx_tap_design": (i, [u32, i, ip, ip, ip, C.POINTER(C.c_int32), i]),
        "nvx_tap_grid": (i, [u32, i, dbl, ip, dp]),
        "nvx_tap_table": (i, [C.POINTER(C.c_int16), i]),
        "nvx_tap_set_shift": (i, [vp, i, i, dbl, dp]),
        "nvx_tap_get_shift": (i, [vp, i, i, ip, dp]),
        "nvx_tap_set_pitch": (i, [vp, i, i, dbl, dp]),
        "nvx_tap_get_pitch": (i, [vp, i, i, ip, dp]),
        "nvx_tap_resident": (i, [vp, vp, sz, sz, vp, sz, sz, zp, vp]),
        "nvx_tap_push": (i, [vp, i, vp, sz, vp, sz, zp]),
        "nvx_tap_reset": (i, [vp, i]),
        "nvx_tap_position": (i, [vp, i, qp, qp]),
        "nvx_tap_plan": (i, [vp, ip, ip, ip, ip, ip, ip]),
        "nvx_tap_timing": (i, [vp, i]),
        "nvx_tap_time_stats": (i, [vp, dp, qp, i]),
        "nvx_tap_last_error": (C.c_char_p, []),
        "nvx_tap_debug_last_launch": (C.c_int64, [vp, ip, ip, ip, ip, zp]),
        "nvx_tap_debug_set_position": (i, [vp, i, u64]),
    }


lib = _companion.load("NAVTEX_AMD_TAP_LIB", "libnavtex_amd_tap.so", _signatures())


TapError, _check = _companion.errors("TapError", __name__, lib.nvx_tap_last_error)


def design(output_rate_hz: int, kind: int = IQ, taps: bool = True):
    """nvx_tap_design: (L, M, T, taps int32 [L, T] or None).  Needs no device."""
    l, m, t = C.c_int(), C.c_int(), C.c_int()
    n = _check(lib.nvx_tap_design(output_rate_hz, kind, C.byref(l), C.byref(m), C.byref(t), None, 0), "nvx_tap_design")
    if not taps:
        return l.value, m.value, t.value, None
    h = np.zeros(n, dtype=np.int32)
    _check(lib.nvx_tap_design(output_rate_hz, kind, None, None, None, h.ctypes.data_as(C.POINTER(C.c_int32)), n), "nvx_tap_design")
    return l.value, m.value, t.value, h.reshape(l.value, t.value)


def grid(output_rate_hz: int, kind: int, hz: float) -> Tuple[int, float]:
    """nvx_tap_grid: (k, applied Hz).  Needs no device."""
    k, a = C.c_int(), C.c_double()
    _check(lib.nvx_tap_grid(output_rate_hz, kind, hz, C.byref(k), C.byref(a)), "nvx_tap_grid")
    return k.value, a.value


def table() -> np.ndarray:
    """nvx_tap_table: W as int16 [4096, 2] (c, s)."""
    w = np.zeros((GRID, 2), dtype=np.int16)
    _check(lib.nvx_tap_table(w.ctypes.data_as(C.POINTER(C.c_int16)), GRID), "nvx_tap_table")
    return w


def out_count(L: int, M: int, consumed_before: int, n_in: int) -> int:
    """The outputs of a call: ceil((consumed_before + n_in) L / M) - ceil(consumed_before L / M)."""
    after = lambda n: -((-n * L) // M)
    return after(consumed_before + n_in) - after(consumed_before)


class Tap(_companion.Handle):
    """nvx_tap wrapper: n_inputs rows of packed int16 IQ at 252 kS/s -> n_taps narrow signals each at output_rate_hz, as
    packed IQ words (IQ) or int16 audio (REAL)."""
    _destroy = lib.nvx_tap_destroy

    def __init__(self, output_rate_hz: int, kind: int = IQ, n_inputs: int = 1, n_taps: int = 1, device: int = 0):
        cfg = Config()
        lib.nvx_tap_config_default(C.byref(cfg))
        cfg.device, cfg.n_inputs, cfg.n_taps, cfg.output_rate_hz, cfg.kind = device, n_inputs, n_taps, output_rate_hz, kind
        h = C.c_void_p()
        _check(lib.nvx_tap_create(C.byref(cfg), C.byref(h)), "nvx_tap_create")
        self._h = h
        self.device, self.kind, self.n_inputs, self.n_taps, self.rate = device, kind, n_inputs, n_taps, output_rate_hz
        l, m, t = C.c_int(), C.c_int(), C.c_int()
        _check(lib.nvx_tap_plan(h, C.byref(l), C.byref(m), C.byref(t), None, None, None), "nvx_tap_plan")
        self.L, self.M, self.T = l.value, m.value, t.value

    def set_shift(self, tap: int, hz: float, input: int = -1) -> float:
        """nvx_tap_set_shift: returns the applied grid frequency."""
        a = C.c_double()
        _check(lib.nvx_tap_set_shift(self._h, input, tap, hz, C.byref(a)), "nvx_tap_set_shift")
        return a.value

    def get_shift(self, tap: int, input: int = 0) -> Tuple[int, float]:
        k, a = C.c_int(), C.c_double()
        _check(lib.nvx_tap_get_shift(self._h, input, tap, C.byref(k), C.byref(a)), "nvx_tap_get_shift")
        return k.value, a.value

    def set_pitch(self, tap: int, pitch_hz: float, input: int = -1) -> float:
        """nvx_tap_set_pitch: returns the applied grid frequency."""
        a = C.c_double()
        _check(lib.nvx_tap_set_pitch(self._h, input, tap, pitch_hz, C.byref(a)), "nvx_tap_set_pitch")
        return a.value

    def get_pitch(self, tap: int, input: int = 0) -> Tuple[int, float]:
        k, a = C.c_int(), C.c_double()
        _check(lib.nvx_tap_get_pitch(self._h, input, tap, C.byref(k), C.byref(a)), "nvx_tap_get_pitch")
        return k.value, a.value

    def resident(self, d_in, pitch_in: int, n_in: int, d_out, pitch_out: int, out_first: int = 0, hip_stream: Optional[int] = None) -> int:
        """nvx_tap_resident: d_in and d_out are DeviceBuffers; ordered on hip_stream, not waited for.  Returns the outputs per row."""
        n = C.c_size_t()
        _check(lib.nvx_tap_resident(self._h, d_in.ptr, pitch_in, n_in, d_out.ptr, pitch_out, out_first, C.byref(n), hip_stream or None), "nvx_tap_resident")
        return n.value

    def push(self, input: int, iq: np.ndarray) -> np.ndarray:
        """nvx_tap_push: one input's samples (int16 [n, 2]) -> int16 [n_taps, outputs, 2] (IQ) or [n_taps, outputs] (REAL)."""
        a = np.ascontiguousarray(iq, dtype=np.int16).reshape(-1, 2)
        cap = out_count(self.L, self.M, self.position(input)[0], a.shape[0]) + 1
        out = np.empty((self.n_taps, cap, 2) if self.kind == IQ else (self.n_taps, cap), dtype=np.int16)
        n = C.c_size_t()
        _check(lib.nvx_tap_push(self._h, input, N.as_ptr(a) if a.size else N.as_ptr(out), a.shape[0], N.as_ptr(out), cap, C.byref(n)), "nvx_tap_push")
        return out[:, :n.value].copy()

    def reset(self, input: int = -1) -> None:
        _check(lib.nvx_tap_reset(self._h, input), "nvx_tap_reset")

    def position(self, input: int = 0) -> Tuple[int, int]:
        """(input samples consumed by `input` since its reset, outputs produced per tap)."""
        c, p = C.c_uint64(), C.c_uint64()
        _check(lib.nvx_tap_position(self._h, input, C.byref(c), C.byref(p)), "nvx_tap_position")
        return c.value, p.value

    def timing(self, enable: bool = True) -> None:
        _check(lib.nvx_tap_timing(self._h, int(enable)), "nvx_tap_timing")

    def time_stats(self, reset: bool = False) -> Tuple[float, int]:
        s, n = C.c_double(), C.c_uint64()
        _check(lib.nvx_tap_time_stats(self._h, C.byref(s), C.byref(n), int(reset)), "nvx_tap_time_stats")
        return s.value, n.value

    def debug_last_launch(self) -> dict:
        """For tests (nvx_tap_debug_last_launch): the shape of the last call as the host handed it over."""
        tile, tiles, form, waves, lds = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
        n = _check(lib.nvx_tap_debug_last_launch(self._h, C.byref(tile), C.byref(tiles), C.byref(form), C.byref(waves), C.byref(lds)),
                   "nvx_tap_debug_last_launch")
        return {"launches": n, "tile_out": tile.value, "tiles": tiles.value, "form": form.value, "waves": waves.value, "lds_bytes": lds.value}

    def debug_set_position(self, position: int, input: int = -1) -> None:
        """For tests (nvx_tap_debug_set_position)."""
        _check(lib.nvx_tap_debug_set_position(self._h, input, position), "nvx_tap_debug_set_position")
