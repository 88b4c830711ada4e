"""ctypes binding of libnavtex_amd_resample.so, the resampler (the C ABI in include/navtex_amd_resample.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _companion, _native as N


OUTPUT_RATE, SHIFT = 252000, 15
CS16, CU8, CS8, CF32 = 0, 1, 2, 3
BYTES_PER_SAMPLE = {CS16: 4, CU8: 2, CS8: 2, CF32: 8}
_DTYPES = {CS16: np.int16, CU8: np.uint8, CS8: np.int8, CF32: np.float32}


class Config(C.Structure):
    """nvx_resample_config."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("n_streams", C.c_int), ("input_rate_hz", C.c_uint32),
                ("format", C.c_int)]


def _signatures() -> dict:
    vp, sz, i, u32, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64
    ip = C.POINTER(i)
    return {
        "nvx_resample_config_default": (None, [C.POINTER(Config)]),
        "nvx_resample_create": (i, [C.POINTER(Config), C.POINTER(vp)]),
        "nvx_resample_destroy": (None, [vp]),
        "nvx_resample_design": (i, [u32, ip, ip, ip, ip, vp, i]),
        "nvx_resample_out_count": (C.c_int64, [u32, u64, u64]),
        "nvx_resample_resident": (i, [vp, vp, sz, sz, vp, sz, sz, C.POINTER(sz), vp]),
        "nvx_resample_push": (i, [vp, i, vp, sz, vp, sz, C.POINTER(sz)]),
        "nvx_resample_reset": (i, [vp, i]),
        "nvx_resample_position": (i, [vp, i, C.POINTER(u64), C.POINTER(u64)]),
        "nvx_resample_plan": (i, [vp, ip, ip, ip, ip, ip]),
        "nvx_resample_set_form": (i, [vp, i]),
        "nvx_resample_timing": (i, [vp, i]),
        "nvx_resample_time_stats": (i, [vp, C.POINTER(C.c_double), C.POINTER(u64), i]),
        "nvx_resample_last_error": (C.c_char_p, []),
        "nvx_resample_debug_last_launch": (C.c_int64, [vp, ip, ip, ip, ip, ip, C.POINTER(sz)]),
    }


lib = _companion.load("NAVTEX_AMD_RESAMPLE_LIB", "libnavtex_amd_resample.so", _signatures())


ResampleError, _check = _companion.errors("ResampleError", __name__, lib.nvx_resample_last_error)


def design(input_rate_hz: int) -> Tuple[int, int, int, int, np.ndarray]:
    """nvx_resample_design: (L, M, T, S, taps [L, T] int16) of a rate; needs no device."""
    L, M, T, S = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    n = _check(lib.nvx_resample_design(input_rate_hz, C.byref(L), C.byref(M), C.byref(T), C.byref(S), None, 0), "nvx_resample_design")
    taps = np.empty(n, dtype=np.int16)
    _check(lib.nvx_resample_design(input_rate_hz, None, None, None, None, N.as_ptr(taps), n), "nvx_resample_design")
    return L.value, M.value, T.value, S.value, taps.reshape(L.value, T.value)


def out_count(input_rate_hz: int, consumed_before: int, n_in: int) -> int:
    """nvx_resample_out_count: the outputs a call with n_in samples writes for a stream that has consumed consumed_before."""
    n = lib.nvx_resample_out_count(input_rate_hz, consumed_before, n_in)
    if n < 0:
        raise ResampleError(N.ERR_ARG, "nvx_resample_out_count")
    return n


class Resampler(_companion.Handle):
    """nvx_resampler wrapper: n_streams streams at input_rate_hz in `format` -> packed int16 IQ at 252 kS/s."""
    _destroy = lib.nvx_resample_destroy

    def __init__(self, input_rate_hz: int, format: int = CS16, n_streams: int = 1, device: int = 0):
        cfg = Config()
        lib.nvx_resample_config_default(C.byref(cfg))
        cfg.device, cfg.n_streams, cfg.input_rate_hz, cfg.format = device, n_streams, input_rate_hz, format
        h = C.c_void_p()
        _check(lib.nvx_resample_create(C.byref(cfg), C.byref(h)), "nvx_resample_create")
        self._h = h
        self.device, self.n_streams, self.format, self.input_rate_hz = device, n_streams, format, input_rate_hz
        L, M, T = C.c_int(), C.c_int(), C.c_int()
        _check(lib.nvx_resample_plan(h, C.byref(L), C.byref(M), C.byref(T), None, None), "nvx_resample_plan")
        self.L, self.M, self.T = L.value, M.value, T.value

    def resident(self, d_in, pitch_in: int, n_in: int, d_out, pitch_out: int, out_first: int = 0, hip_stream: Optional[int] = None) -> int:
        """nvx_resample_resident: d_in and d_out are DeviceBuffers; ordered on hip_stream, not waited for.  Returns the
        number of outputs written per stream."""
        n = C.c_size_t()
        _check(lib.nvx_resample_resident(self._h, d_in.ptr, pitch_in, n_in, d_out.ptr, pitch_out, out_first, C.byref(n), hip_stream or None),
               "nvx_resample_resident")
        return n.value

    def push(self, stream: int, samples: np.ndarray) -> np.ndarray:
        """nvx_resample_push: one stream's samples ([n, 2] in the plan's format) -> int16 [n_out, 2], ready for Pipeline.push."""
        a = np.ascontiguousarray(samples, dtype=_DTYPES[self.format]).reshape(-1, 2)
        consumed, _ = self.position(stream)
        cap = out_count(self.input_rate_hz, consumed, a.shape[0])
        out = np.empty((max(cap, 1), 2), dtype=np.int16)
        n = C.c_size_t()
        _check(lib.nvx_resample_push(self._h, stream, N.as_ptr(a) if a.size else N.as_ptr(out), a.shape[0], N.as_ptr(out), cap, C.byref(n)),
               "nvx_resample_push")
        return out[:n.value]

    def reset(self, stream: int = -1) -> None:
        _check(lib.nvx_resample_reset(self._h, stream), "nvx_resample_reset")

    def position(self, stream: int = 0) -> Tuple[int, int]:
        """(input samples consumed, outputs produced) of `stream` since its reset."""
        c, p = C.c_uint64(), C.c_uint64()
        _check(lib.nvx_resample_position(self._h, stream, C.byref(c), C.byref(p)), "nvx_resample_position")
        return c.value, p.value

    def set_form(self, form: int) -> None:
        _check(lib.nvx_resample_set_form(self._h, form), "nvx_resample_set_form")

    def timing(self, enable: bool = True) -> None:
        _check(lib.nvx_resample_timing(self._h, int(enable)), "nvx_resample_timing")

    def time_stats(self, reset: bool = False) -> Tuple[float, int]:
        s, n = C.c_double(), C.c_uint64()
        _check(lib.nvx_resample_time_stats(self._h, C.byref(s), C.byref(n), int(reset)), "nvx_resample_time_stats")
        return s.value, n.value

    def debug_last_launch(self) -> dict:
        """For tests (nvx_resample_debug_last_launch): the shape of the last kernel launch as the host handed it over."""
        K, tiles, tpc, chunks, in_lds, lds = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
        n = _check(lib.nvx_resample_debug_last_launch(self._h, C.byref(K), C.byref(tiles), C.byref(tpc), C.byref(chunks), C.byref(in_lds),
                                                      C.byref(lds)), "nvx_resample_debug_last_launch")
        return {"launches": n, "K": K.value, "tiles": tiles.value, "tiles_per_chunk": tpc.value, "chunks": chunks.value,
                "taps_in_lds": bool(in_lds.value), "lds_bytes": lds.value}
