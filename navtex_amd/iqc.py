"""ctypes binding of libnavtex_amd_iqc.so, the IQ corrector (the C ABI in include/navtex_amd_iqc.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _companion, _native as N


BLOCK = 65536
WINDOW_LOG2_DEFAULT = 4
TRACK, HOLD = 0, 1
CS16, CU8, CS8, CF32 = 0, 1, 2, 3
BYTES_PER_SAMPLE = {CS16: 4, CU8: 2, CS8: 2, CF32: 8}
_DTYPES = {CS16: np.int16, CU8: np.uint8, CS8: np.int8, CF32: np.float32}


class Config(C.Structure):
    """nvx_iqc_config."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("format", C.c_int), ("n_streams", C.c_int), ("window_log2", C.c_int)]


class Status(C.Structure):
    """nvx_iqc_status."""
    _fields_ = [("dI", C.c_int32), ("dQ", C.c_int32), ("c_i", C.c_int32), ("c_q", C.c_int32), ("mode", C.c_int32), ("last_reason", C.c_int32),
                ("sums", C.c_int64 * 5), ("samples", C.c_uint64), ("blocks_solved", C.c_uint64), ("blocks_rejected", C.c_uint64)]


def _signatures() -> dict:
    vp, sz, i, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64
    ip, qp = C.POINTER(i), C.POINTER(u64)
    return {
        "nvx_iqc_config_default": (None, [C.POINTER(Config)]),
        "nvx_iqc_create": (i, [C.POINTER(Config), C.POINTER(vp)]),
        "nvx_iqc_destroy": (None, [vp]),
        "nvx_iqc_resident": (i, [vp, vp, sz, sz, vp, sz, sz, vp]),
        "nvx_iqc_push": (i, [vp, i, vp, sz, vp]),
        "nvx_iqc_reset": (i, [vp, i]),
        "nvx_iqc_set": (i, [vp, i, i, i, i, i]),
        "nvx_iqc_set_mode": (i, [vp, i, i]),
        "nvx_iqc_get": (i, [vp, i, C.POINTER(Status)]),
        "nvx_iqc_position": (i, [vp, i, qp]),
        "nvx_iqc_plan": (i, [vp, ip, ip, ip]),
        "nvx_iqc_timing": (i, [vp, i]),
        "nvx_iqc_time_stats": (i, [vp, C.POINTER(C.c_double), qp, i]),
        "nvx_iqc_last_error": (C.c_char_p, []),
        "nvx_iqc_debug_last_launch": (C.c_int64, [vp, ip, ip, ip, ip]),
        "nvx_iqc_debug_set_position": (i, [vp, i, u64]),
    }


lib = _companion.load("NAVTEX_AMD_IQC_LIB", "libnavtex_amd_iqc.so", _signatures())


IqcError, _check = _companion.errors("IqcError", __name__, lib.nvx_iqc_last_error)


class Corrector(_companion.Handle):
    """nvx_iq_corrector wrapper: n_streams streams in `format` -> packed int16 IQ at the same rate, DC offset and image removed."""
    _destroy = lib.nvx_iqc_destroy

    def __init__(self, format: int = CS16, n_streams: int = 1, window_log2: int = WINDOW_LOG2_DEFAULT, device: int = 0):
        cfg = Config()
        lib.nvx_iqc_config_default(C.byref(cfg))
        cfg.device, cfg.format, cfg.n_streams, cfg.window_log2 = device, format, n_streams, window_log2
        h = C.c_void_p()
        _check(lib.nvx_iqc_create(C.byref(cfg), C.byref(h)), "nvx_iqc_create")
        self._h = h
        self.device, self.format, self.n_streams, self.window_log2 = device, format, n_streams, window_log2

    def resident(self, d_in, pitch_in: int, n_in: int, d_out, pitch_out: int, out_first: int = 0, hip_stream: Optional[int] = None) -> None:
        """nvx_iqc_resident: d_in and d_out are DeviceBuffers; ordered on hip_stream, not waited for."""
        _check(lib.nvx_iqc_resident(self._h, d_in.ptr, pitch_in, n_in, d_out.ptr, pitch_out, out_first, hip_stream or None), "nvx_iqc_resident")

    def push(self, stream: int, samples: np.ndarray) -> np.ndarray:
        """nvx_iqc_push: one stream's samples ([n, 2] in the plan's format) -> int16 [n, 2]."""
        a = np.ascontiguousarray(samples, dtype=_DTYPES[self.format]).reshape(-1, 2)
        out = np.empty((max(a.shape[0], 1), 2), dtype=np.int16)
        _check(lib.nvx_iqc_push(self._h, stream, N.as_ptr(a) if a.size else N.as_ptr(out), a.shape[0], N.as_ptr(out)), "nvx_iqc_push")
        return out[:a.shape[0]]

    def reset(self, stream: int = -1) -> None:
        _check(lib.nvx_iqc_reset(self._h, stream), "nvx_iqc_reset")

    def set(self, dI: int, dQ: int, c_i: int, c_q: int, stream: int = -1) -> None:
        """nvx_iqc_set: the coefficients from the next call's first sample on."""
        _check(lib.nvx_iqc_set(self._h, stream, dI, dQ, c_i, c_q), "nvx_iqc_set")

    def set_mode(self, mode: int, stream: int = -1) -> None:
        _check(lib.nvx_iqc_set_mode(self._h, stream, mode), "nvx_iqc_set_mode")

    def get(self, stream: int = 0) -> dict:
        """nvx_iqc_get: the coefficients (dI, dQ, c_i, c_q), the mode, the last reason, the window's five sums, the counters."""
        s = Status()
        _check(lib.nvx_iqc_get(self._h, stream, C.byref(s)), "nvx_iqc_get")
        return {"coefficients": (s.dI, s.dQ, s.c_i, s.c_q), "mode": s.mode, "last_reason": s.last_reason, "sums": tuple(s.sums),
                "samples": s.samples, "blocks_solved": s.blocks_solved, "blocks_rejected": s.blocks_rejected}

    def position(self, stream: int = 0) -> int:
        """Samples consumed by `stream` since its reset."""
        c = C.c_uint64()
        _check(lib.nvx_iqc_position(self._h, stream, C.byref(c)), "nvx_iqc_position")
        return c.value

    def timing(self, enable: bool = True) -> None:
        _check(lib.nvx_iqc_timing(self._h, int(enable)), "nvx_iqc_timing")

    def time_stats(self, reset: bool = False) -> Tuple[float, int]:
        s, n = C.c_double(), C.c_uint64()
        _check(lib.nvx_iqc_time_stats(self._h, C.byref(s), C.byref(n), int(reset)), "nvx_iqc_time_stats")
        return s.value, n.value

    def debug_last_launch(self) -> dict:
        """For tests (nvx_iqc_debug_last_launch): the shape of the last call as the host handed it over."""
        chunks, tpc, rec, form = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        n = _check(lib.nvx_iqc_debug_last_launch(self._h, C.byref(chunks), C.byref(tpc), C.byref(rec), C.byref(form)), "nvx_iqc_debug_last_launch")
        return {"launches": n, "chunks": chunks.value, "tiles_per_chunk": tpc.value, "records": rec.value, "form": form.value}

    def debug_set_position(self, position: int, stream: int = -1) -> None:
        """For tests (nvx_iqc_debug_set_position)."""
        _check(lib.nvx_iqc_debug_set_position(self._h, stream, position), "nvx_iqc_debug_set_position")
