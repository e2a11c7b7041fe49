"""ctypes loader for libsharp_hip.so -- the only compute backend of this package.

There is deliberately no fallback: if the HIP library is missing or no gfx950 device
is visible, every entry point raises (the product path must fail loudly, never route
through a CPU path)."""
import ctypes as C
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libsharp_hip.so")
_lib = None
_initialised_device = None


class SharpError(RuntimeError):
    """Raised where the reference would stop(): carries the library's message."""


def so_path():
    return _SO


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise SharpError(
                f"{_SO} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C sharp_amd/csrc` (hipcc, gfx950). There is no CPU fallback.")
        try:  # torch wheels bundle their own libamdhip64: load it first so the process has ONE HIP runtime
            import torch  # noqa: F401
        except Exception:
            pass
        so = C.CDLL(_SO)
        for name, sig in _abi.SIGNATURES.items():
            ret, args = sig.split(":")
            try:
                fn = getattr(so, name)
            except AttributeError:                          # (here, not at the first use of that entry)
                raise SharpError(f"{_SO} does not export {name}, which sharp_amd/_abi.py lists: rebuild the library") from None
            fn.restype = _abi.RETURN[ret]
            fn.argtypes = [_abi.ARGUMENT[a] for a in args]
        _lib = so
    return _lib


def ptr(a, dtype):
    """The address of a numpy array for a pointer argument (None: NULL), after checking that it is what the library will read or write
    there: exactly `dtype`, and one contiguous block."""
    if a is None:
        return None
    if not (isinstance(a, np.ndarray) and a.dtype == dtype and (a.flags.c_contiguous or a.flags.f_contiguous)):
        got = type(a).__name__ if not isinstance(a, np.ndarray) else f"{a.dtype}" if a.dtype != dtype else "a non-contiguous view"
        raise TypeError(f"expected a contiguous numpy array of {np.dtype(dtype).name}, got {got}")
    return a.ctypes.data


def f64(a):
    return ptr(a, np.float64)


def i32(a):
    return ptr(a, np.int32)


def i64(a):
    return ptr(a, np.int64)


def i8(a):
    return ptr(a, np.int8)


def check(rc, allow=0):
    """rc == 0 ok; warning bits in `allow` are returned to the caller; anything else raises."""
    if rc == 0:
        return 0
    if rc & ~allow == 0:
        return rc
    msg = lib().sharp_last_error()
    raise SharpError(msg.decode() if msg else f"libsharp_hip error {rc}")


def init(device=None):
    """Select the GPU (default: LOCAL_RANK or 0) and create the library's stream."""
    global _initialised_device
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    if _initialised_device != device:
        check(lib().sharp_init(int(device)))
        _initialised_device = device
    return device


def shutdown():
    """sharp_shutdown(): the streams of every slot are destroyed (workspaces stay); the next call initialises the library again."""
    global _initialised_device
    check(lib().sharp_shutdown())
    _initialised_device = None


def ensure_init():
    if _initialised_device is None:
        init()


def reload_options():
    """Ask the library to read its SHARP_* environment switches again (it reads them once, at first use)."""
    check(lib().sharp_reload_options())
