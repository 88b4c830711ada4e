"""ctypes binding of libnavtex_amd_scan.so, the band scan (the C ABI in include/navtex_amd_scan.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

from . import _companion, _native as N


FFT, BIN_HZ, SLOTS_PER_FRAME = 2048, 30.76171875, 9


class Params(C.Structure):
    """nvx_scan_params."""
    _fields_ = [("struct_size", C.c_uint32), ("band_half", C.c_int), ("floor_half", C.c_int), ("guard_bins", C.c_int),
                ("shadow_bins", C.c_int), ("refine_half", C.c_int), ("refine_iters", C.c_int),
                ("min_score_db", C.c_double), ("shadow_db", C.c_double), ("max_offset_hz", C.c_double),
                ("dc_guard_hz", C.c_double), ("dc_max_shift_hz", C.c_double)]


class Hit(C.Structure):
    """nvx_scan_hit."""
    _fields_ = [("offset_hz", C.c_double), ("score_db", C.c_double), ("shift_hz", C.c_double), ("band_power_db", C.c_double),
                ("bin", C.c_int)]


def _signatures() -> dict:
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    return {
        "nvx_scan_resident": (i, [i, vp, sz, sz, i, i, i, i, vp, vp]),
        "nvx_scan_iq": (i, [i, vp, sz, i, i, vp, C.POINTER(i)]),
        "nvx_scan_set_form": (i, [i]),
        "nvx_scan_timing": (None, [i]),
        "nvx_scan_time_stats": (i, [C.POINTER(C.c_double), C.POINTER(C.c_uint64), i]),
        "nvx_scan_last_error": (C.c_char_p, []),
        "nvx_scan_params_default": (None, [C.POINTER(Params)]),
        "nvx_scan_find": (i, [vp, C.POINTER(Params), C.POINTER(Hit), i]),
        "nvx_scan_debug_last_launch": (C.c_int64, [C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(sz)]),
    }


lib = _companion.load("NAVTEX_AMD_SCAN_LIB", "libnavtex_amd_scan.so", _signatures())


ScanError, _check = _companion.errors("ScanError", __name__, lib.nvx_scan_last_error)


def scan_resident_into(buf, pitch: int, first_frame: int, n_frames: int, n_streams: int, raw_rate: bool, stage0_order: int,
                       power, hip_stream: Optional[int] = None) -> None:
    """nvx_scan_resident: buf and power are DeviceBuffers; ordered on hip_stream, not waited for."""
    _check(lib.nvx_scan_resident(buf.device, buf.ptr, pitch, first_frame, n_frames, n_streams, int(raw_rate), stage0_order,
                                 power.ptr, hip_stream), "nvx_scan_resident")


def scan_resident(buf, pitch: int, first_frame: int, n_frames: int, n_streams: int, raw_rate: bool, stage0_order: int = 1) -> np.ndarray:
    """The power rows [n_streams, 2048] of frames [first_frame, first_frame + n_frames) of the streams in buf."""
    from . import DeviceBuffer
    power = DeviceBuffer(n_streams * FFT * 8, buf.device)
    try:
        scan_resident_into(buf, pitch, first_frame, n_frames, n_streams, raw_rate, stage0_order, power)
        return power.download(n_streams * FFT * 8, dtype=np.float64).reshape(n_streams, FFT)     # the copy waits for the null stream
    finally:
        power.free()


def scan_iq(iq: np.ndarray, raw_rate: bool, stage0_order: int = 1, device: int = 0) -> Tuple[np.ndarray, int]:
    """nvx_scan_iq: (power [2048], frames used) of one stream's int16 [n, 2] samples in host memory."""
    iq = np.ascontiguousarray(iq, dtype=np.int16).reshape(-1, 2)
    power = np.empty(FFT, dtype=np.float64)
    used = C.c_int(0)
    _check(lib.nvx_scan_iq(device, N.as_ptr(iq), iq.shape[0], int(raw_rate), stage0_order, N.as_ptr(power), C.byref(used)), "nvx_scan_iq")
    return power, used.value


def default_params() -> Params:
    p = Params()
    lib.nvx_scan_params_default(C.byref(p))
    return p


def find(power: np.ndarray, params: Optional[Params] = None, cap: int = 64) -> List[dict]:
    """nvx_scan_find: the carriers of one power row, in descending score."""
    power = np.ascontiguousarray(power, dtype=np.float64)
    if power.shape != (FFT,):
        raise ValueError("a power row has 2048 values")
    hits = (Hit * max(cap, 1))()
    n = _check(lib.nvx_scan_find(N.as_ptr(power), C.byref(params) if params is not None else None, hits, cap), "nvx_scan_find")
    return [{f: getattr(hits[k], f) for f, _ in Hit._fields_} for k in range(min(n, cap))]


def set_form(form: int) -> None:
    _check(lib.nvx_scan_set_form(form), "nvx_scan_set_form")


def timing(enable: bool = True) -> None:
    lib.nvx_scan_timing(int(enable))


def time_stats(reset: bool = False) -> Tuple[float, int]:
    s, n = C.c_double(), C.c_uint64()
    _check(lib.nvx_scan_time_stats(C.byref(s), C.byref(n), int(reset)), "nvx_scan_time_stats")
    return s.value, n.value


def debug_last_launch() -> dict:
    """For tests (nvx_scan_debug_last_launch): the form, first grid and scratch of the last launch as the host handed it over."""
    form, gx, gy, scratch = C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
    n = lib.nvx_scan_debug_last_launch(C.byref(form), C.byref(gx), C.byref(gy), C.byref(scratch))
    return dict(launches=n, form=form.value, grid=(gx.value, gy.value), scratch_bytes=scratch.value)
