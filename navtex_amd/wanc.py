"""ctypes binding of libnavtex_amd_wanc.so, the multi-tap antenna noise canceller (the C ABI in include/navtex_amd_wanc.h).

Plumbing only, like the package itself: no signal processing and no fallback -- without the companion library the
import fails.  Device memory comes from the package's DeviceBuffer."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _companion, _native as N


BLOCK = 65536
WINDOW_LOG2_DEFAULT, TAPS_DEFAULT, TAPS_MAX, LOAD_LOG2_DEFAULT = 2, 8, 16, 12
W_ONE, W_MAX, L1_MAX, COHERENCE_ONE = 8192, 32767, 65534, 16384
TRACK, HOLD = 0, 1
CS16, CU8, CS8, CF32 = 0, 1, 2, 3
BYTES_PER_SAMPLE = {CS16: 4, CU8: 2, CS8: 2, CF32: 8}
_DTYPES = {CS16: np.int16, CU8: np.uint8, CS8: np.int8, CF32: np.float32}


class Config(C.Structure):
    """nvx_wanc_config."""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int), ("format", C.c_int), ("n_pairs", C.c_int), ("window_log2", C.c_int),
                ("n_taps", C.c_int), ("load_log2", C.c_int)]


class Status(C.Structure):
    """nvx_wanc_status."""
    _fields_ = [("n_taps", C.c_int32), ("mode", C.c_int32), ("last_reason", C.c_int32), ("coherence_q14", C.c_int32),
                ("w_re", C.c_int32 * TAPS_MAX), ("w_im", C.c_int32 * TAPS_MAX),
                ("r_re", C.c_int64 * TAPS_MAX), ("r_im", C.c_int64 * TAPS_MAX), ("q_re", C.c_int64 * TAPS_MAX), ("q_im", C.c_int64 * TAPS_MAX),
                ("saa", C.c_int64), ("samples", C.c_uint64), ("blocks_solved", C.c_uint64), ("blocks_rejected", C.c_uint64)]


def _signatures() -> dict:
    vp, sz, i, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64
    ip, qp, wp = C.POINTER(i), C.POINTER(u64), C.POINTER(C.c_int32)
    return {
        "nvx_wanc_config_default": (None, [C.POINTER(Config)]),
        "nvx_wanc_create": (i, [C.POINTER(Config), C.POINTER(vp)]),
        "nvx_wanc_destroy": (None, [vp]),
        "nvx_wanc_resident": (i, [vp, vp, sz, vp, sz, sz, vp, sz, sz, vp]),
        "nvx_wanc_push": (i, [vp, i, vp, vp, sz, vp]),
        "nvx_wanc_reset": (i, [vp, i]),
        "nvx_wanc_set": (i, [vp, i, wp, wp]),
        "nvx_wanc_set_mode": (i, [vp, i, i]),
        "nvx_wanc_get": (i, [vp, i, C.POINTER(Status)]),
        "nvx_wanc_position": (i, [vp, i, qp]),
        "nvx_wanc_plan": (i, [vp, ip, ip, ip, ip, ip]),
        "nvx_wanc_timing": (i, [vp, i]),
        "nvx_wanc_time_stats": (i, [vp, C.POINTER(C.c_double), qp, i]),
        "nvx_wanc_last_error": (C.c_char_p, []),
        "nvx_wanc_debug_last_launch": (C.c_int64, [vp, ip, ip, ip, ip]),
        "nvx_wanc_debug_set_position": (i, [vp, i, u64]),
    }


lib = _companion.load("NAVTEX_AMD_WANC_LIB", "libnavtex_amd_wanc.so", _signatures())


WancError, _check = _companion.errors("WancError", __name__, lib.nvx_wanc_last_error)


class Canceller(_companion.Handle):
    """nvx_wide_canceller wrapper: n_pairs pairs of rows (main, sense) in `format` -> packed int16 IQ at the same rate, the main
    row delayed by n_taps / 2 samples less n_taps complex weights on the sense row."""
    _destroy = lib.nvx_wanc_destroy

    def __init__(self, format: int = CS16, n_pairs: int = 1, n_taps: int = TAPS_DEFAULT, window_log2: int = WINDOW_LOG2_DEFAULT,
                 load_log2: int = LOAD_LOG2_DEFAULT, device: int = 0):
        cfg = Config()
        lib.nvx_wanc_config_default(C.byref(cfg))
        cfg.device, cfg.format, cfg.n_pairs, cfg.window_log2, cfg.n_taps, cfg.load_log2 = device, format, n_pairs, window_log2, n_taps, load_log2
        h = C.c_void_p()
        _check(lib.nvx_wanc_create(C.byref(cfg), C.byref(h)), "nvx_wanc_create")
        self._h = h
        self.device, self.format, self.n_pairs, self.n_taps, self.window_log2, self.load_log2 = device, format, n_pairs, n_taps, window_log2, load_log2

    def resident(self, d_main, pitch_main: int, d_sense, pitch_sense: int, n_in: int, d_out, pitch_out: int, out_first: int = 0,
                 hip_stream: Optional[int] = None) -> None:
        """nvx_wanc_resident: d_main, d_sense and d_out are DeviceBuffers; ordered on hip_stream, not waited for."""
        _check(lib.nvx_wanc_resident(self._h, d_main.ptr, pitch_main, d_sense.ptr, pitch_sense, n_in, d_out.ptr, pitch_out, out_first, hip_stream or None),
               "nvx_wanc_resident")

    def push(self, pair: int, main: np.ndarray, sense: np.ndarray) -> np.ndarray:
        """nvx_wanc_push: one pair's samples ([n, 2] each, in the plan's format) -> int16 [n, 2]."""
        a = np.ascontiguousarray(main, dtype=_DTYPES[self.format]).reshape(-1, 2)
        b = np.ascontiguousarray(sense, dtype=_DTYPES[self.format]).reshape(-1, 2)
        if a.shape != b.shape:
            raise ValueError(f"main has {a.shape[0]} samples, sense {b.shape[0]}")
        out = np.empty((max(a.shape[0], 1), 2), dtype=np.int16)
        _check(lib.nvx_wanc_push(self._h, pair, N.as_ptr(a) if a.size else N.as_ptr(out), N.as_ptr(b) if b.size else N.as_ptr(out), a.shape[0],
                                 N.as_ptr(out)), "nvx_wanc_push")
        return out[:a.shape[0]]

    def reset(self, pair: int = -1) -> None:
        _check(lib.nvx_wanc_reset(self._h, pair), "nvx_wanc_reset")

    def set(self, w_re: Sequence[int], w_im: Sequence[int], pair: int = -1) -> None:
        """nvx_wanc_set: the n_taps weights (Q13) from the next call's first sample on."""
        if len(w_re) != self.n_taps or len(w_im) != self.n_taps:
            raise ValueError(f"{self.n_taps} weights wanted, {len(w_re)} and {len(w_im)} given")
        arr = C.c_int32 * self.n_taps
        _check(lib.nvx_wanc_set(self._h, pair, arr(*[int(v) for v in w_re]), arr(*[int(v) for v in w_im])), "nvx_wanc_set")

    def set_mode(self, mode: int, pair: int = -1) -> None:
        _check(lib.nvx_wanc_set_mode(self._h, pair, mode), "nvx_wanc_set_mode")

    def get(self, pair: int = 0) -> dict:
        """nvx_wanc_get: the weights ((w_re ...), (w_im ...)), the mode, the last reason and its coherence, the window's sums in the
        order Re R[0 .. K), Im R, Re Q, Im Q, TAA, and the counters."""
        s = Status()
        _check(lib.nvx_wanc_get(self._h, pair, C.byref(s)), "nvx_wanc_get")
        K = s.n_taps
        return {"weights": (tuple(s.w_re[:K]), tuple(s.w_im[:K])), "mode": s.mode, "last_reason": s.last_reason, "coherence_q14": s.coherence_q14,
                "sums": tuple(s.r_re[:K]) + tuple(s.r_im[:K]) + tuple(s.q_re[:K]) + tuple(s.q_im[:K]) + (s.saa,),
                "samples": s.samples, "blocks_solved": s.blocks_solved, "blocks_rejected": s.blocks_rejected}

    def position(self, pair: int = 0) -> int:
        """Samples consumed by `pair` since its reset."""
        c = C.c_uint64()
        _check(lib.nvx_wanc_position(self._h, pair, C.byref(c)), "nvx_wanc_position")
        return c.value

    def timing(self, enable: bool = True) -> None:
        _check(lib.nvx_wanc_timing(self._h, int(enable)), "nvx_wanc_timing")

    def time_stats(self, reset: bool = False) -> Tuple[float, int]:
        s, n = C.c_double(), C.c_uint64()
        _check(lib.nvx_wanc_time_stats(self._h, C.byref(s), C.byref(n), int(reset)), "nvx_wanc_time_stats")
        return s.value, n.value

    def debug_last_launch(self) -> dict:
        """For tests (nvx_wanc_debug_last_launch): the shape of the last call as the host handed it over."""
        chunks, tpc, rec, form = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        n = _check(lib.nvx_wanc_debug_last_launch(self._h, C.byref(chunks), C.byref(tpc), C.byref(rec), C.byref(form)), "nvx_wanc_debug_last_launch")
        return {"launches": n, "chunks": chunks.value, "tiles_per_chunk": tpc.value, "records": rec.value, "form": form.value}

    def debug_set_position(self, position: int, pair: int = -1) -> None:
        """For tests (nvx_wanc_debug_set_position)."""
        _check(lib.nvx_wanc_debug_set_position(self._h, pair, position), "nvx_wanc_debug_set_position")
