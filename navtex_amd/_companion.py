"""What the ctypes bindings of the companion libraries (scan.py, resample.py, ddc.py) have in common: loading the library,
its error class, and the life of a handle.  Plumbing only: without its library a binding's import fails."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

from . import _native as N


def load(env_var: str, file_name: str, signatures: dict) -> C.CDLL:
    """The library at $env_var, or file_name beside this package, with {name: (restype, argtypes)} applied."""
    path = Path(os.environ.get(env_var) or (Path(__file__).resolve().parent / file_name))
    if not path.exists():
        raise ImportError(f"{path} is missing: build it with `python navtex_amd/build.py` (hipcc, gfx950)")
    lib = C.CDLL(str(path))
    for name, (res, args) in signatures.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def errors(name: str, module: str, last_error):
    """(the library's NvxError subclass, carrying the sentence of its own last_error; the check that raises it for rc < 0)."""
    def __init__(self, code: int, where: str):
        self.code = code
        RuntimeError.__init__(self, f"{where}: error {code}: {last_error().decode(errors='replace')}")

    error = type(name, (N.NvxError,), {"__init__": __init__, "__module__": module})

    def check(rc: int, where: str) -> int:
        if rc < 0:
            raise error(rc, where)
        return rc

    return error, check


class Handle:
    """A handle in self._h that `_destroy` (the library's nvx_*_destroy) releases: once, by close(), a with block or collection."""
    _destroy = None

    def close(self) -> None:
        if getattr(self, "_h", None):
            type(self)._destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()
