"""ctypes binding of libnavtex_amd_narrow.so, the narrowband interpolator (the C ABI in include/navtex_amd_narrow.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from fractions import Fraction
from typing import Optional, Tuple

import numpy as np

from . import _companion, _native as N


OUTPUT_RATE = 252000
S = 14
STATE_WORDS = 32
S16, U8, S8, F32 = 0, 1, 2, 3
IQ, REAL = 0, 1
BYTES_PER_SAMPLE = {IQ: {S16: 4, U8: 2, S8: 2, F32: 8}, REAL: {S16: 2, U8: 1, S8: 1, F32: 4}}
_DTYPES = {S16: np.int16, U8: np.uint8, S8: np.int8, F32: np.float32}


class Config(C.Structure):
    """nvx_nb_config."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("n_streams", C.c_int), ("rate_num", C.c_uint32), ("rate_den", C.c_uint32),
                ("format", C.c_int), ("kind", C.c_int)]


def _signatures() -> dict:
    vp, sz, i, u32, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64
    ip, qp, zp = C.POINTER(i), C.POINTER(u64), C.POINTER(sz)
    return {
        "nvx_nb_config_default": (None, [C.POINTER(Config)]),
        "nvx_nb_create": (i, [C.POINTER(Config), C.POINTER(vp)]),
        "nvx_nb_destroy": (None, [vp]),
        "nvx_nb_design": (i, [u32, u32, ip, ip, ip, C.POINTER(C.c_int16), i]),
        "nvx_nb_resident": (i, [vp, vp, sz, sz, vp, sz, sz, zp, vp]),
        "nvx_nb_push": (i, [vp, i, vp, sz, vp, sz, zp]),
        "nvx_nb_reset": (i, [vp, i]),
        "nvx_nb_position": (i, [vp, i, qp, qp]),
        "nvx_nb_plan": (i, [vp, ip, ip, ip, ip, ip, ip]),
        "nvx_nb_timing": (i, [vp, i]),
        "nvx_nb_time_stats": (i, [vp, C.POINTER(C.c_double), qp, i]),
        "nvx_nb_last_error": (C.c_char_p, []),
        "nvx_nb_debug_last_launch": (C.c_int64, [vp, ip, ip, ip, ip, ip, zp]),
        "nvx_nb_debug_set_position": (i, [vp, i, u64]),
    }


lib = _companion.load("NAVTEX_AMD_NARROW_LIB", "libnavtex_amd_narrow.so", _signatures())


NarrowError, _check = _companion.errors("NarrowError", __name__, lib.nvx_nb_last_error)


def design(rate_num: int, rate_den: int = 1, taps: bool = True):
    """nvx_nb_design: (L, M, T, taps int16 [L, T] or None).  Needs no device."""
    l, m, t = C.c_int(), C.c_int(), C.c_int()
    n = _check(lib.nvx_nb_design(rate_num, rate_den, C.byref(l), C.byref(m), C.byref(t), None, 0), "nvx_nb_design")
    if not taps:
        return l.value, m.value, t.value, None
    h = np.zeros(n, dtype=np.int16)
    _check(lib.nvx_nb_design(rate_num, rate_den, None, None, None, h.ctypes.data_as(C.POINTER(C.c_int16)), n), "nvx_nb_design")
    return l.value, m.value, t.value, h.reshape(l.value, t.value)


def out_count(L: int, M: int, consumed_before: int, n_in: int) -> int:
    """The outputs of a call: ceil((consumed_before + n_in) L / M) - ceil(consumed_before L / M)."""
    after = lambda n: -((-n * L) // M)
    return after(consumed_before + n_in) - after(consumed_before)


class Interpolator(_companion.Handle):
    """nvx_nb_interpolator wrapper: n_streams streams at rate_num / rate_den S/s in `format` and `kind` -> packed int16 IQ at
    252 kS/s."""
    _destroy = lib.nvx_nb_destroy

    def __init__(self, rate_num: int, rate_den: int = 1, format: int = S16, kind: int = IQ, n_streams: int = 1, device: int = 0):
        cfg = Config()
        lib.nvx_nb_config_default(C.byref(cfg))
        cfg.device, cfg.n_streams, cfg.rate_num, cfg.rate_den, cfg.format, cfg.kind = device, n_streams, rate_num, rate_den, format, kind
        h = C.c_void_p()
        _check(lib.nvx_nb_create(C.byref(cfg), C.byref(h)), "nvx_nb_create")
        self._h = h
        self.device, self.format, self.kind, self.n_streams = device, format, kind, n_streams
        self.rate = Fraction(rate_num, rate_den)
        l, m, t = C.c_int(), C.c_int(), C.c_int()
        _check(lib.nvx_nb_plan(h, C.byref(l), C.byref(m), C.byref(t), None, None, None), "nvx_nb_plan")
        self.L, self.M, self.T = l.value, m.value, t.value

    def resident(self, d_in, pitch_in: int, n_in: int, d_out, pitch_out: int, out_first: int = 0, hip_stream: Optional[int] = None) -> int:
        """nvx_nb_resident: d_in and d_out are DeviceBuffers; ordered on hip_stream, not waited for.  Returns the outputs per stream."""
        n = C.c_size_t()
        _check(lib.nvx_nb_resident(self._h, d_in.ptr, pitch_in, n_in, d_out.ptr, pitch_out, out_first, C.byref(n), hip_stream or None), "nvx_nb_resident")
        return n.value

    def push(self, stream: int, samples: np.ndarray) -> np.ndarray:
        """nvx_nb_push: one stream's samples (IQ: [n, 2], REAL: [n], in the plan's format) -> int16 [outputs, 2]."""
        a = np.ascontiguousarray(samples, dtype=_DTYPES[self.format])
        a = a.reshape(-1, 2) if self.kind == IQ else a.reshape(-1)
        cap = out_count(self.L, self.M, self.position(stream)[0], a.shape[0]) + 1
        out = np.empty((cap, 2), dtype=np.int16)
        n = C.c_size_t()
        _check(lib.nvx_nb_push(self._h, stream, N.as_ptr(a) if a.size else N.as_ptr(out), a.shape[0], N.as_ptr(out), cap, C.byref(n)), "nvx_nb_push")
        return out[:n.value]

    def reset(self, stream: int = -1) -> None:
        _check(lib.nvx_nb_reset(self._h, stream), "nvx_nb_reset")

    def position(self, stream: int = 0) -> Tuple[int, int]:
        """(input samples consumed by `stream` since its reset, outputs produced)."""
        c, p = C.c_uint64(), C.c_uint64()
        _check(lib.nvx_nb_position(self._h, stream, C.byref(c), C.byref(p)), "nvx_nb_position")
        return c.value, p.value

    def timing(self, enable: bool = True) -> None:
        _check(lib.nvx_nb_timing(self._h, int(enable)), "nvx_nb_timing")

    def time_stats(self, reset: bool = False) -> Tuple[float, int]:
        s, n = C.c_double(), C.c_uint64()
        _check(lib.nvx_nb_time_stats(self._h, C.byref(s), C.byref(n), int(reset)), "nvx_nb_time_stats")
        return s.value, n.value

    def debug_last_launch(self) -> dict:
        """For tests (nvx_nb_debug_last_launch): the shape of the last call as the host handed it over."""
        chunks, tpc, form, windows, parts, lds = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
        n = _check(lib.nvx_nb_debug_last_launch(self._h, C.byref(chunks), C.byref(tpc), C.byref(form), C.byref(windows), C.byref(parts), C.byref(lds)),
                   "nvx_nb_debug_last_launch")
        return {"launches": n, "chunks": chunks.value, "tiles_per_chunk": tpc.value, "form": form.value, "windows": windows.value,
                "parts": parts.value, "lds_bytes": lds.value}

    def debug_set_position(self, position: int, stream: int = -1) -> None:
        """For tests (nvx_nb_debug_set_position)."""
        _check(lib.nvx_nb_debug_set_position(self._h, stream, position), "nvx_nb_debug_set_position")
