"""ctypes binding of ``libfedagg_promote.so`` (the C ABI declared in ``include/fedagg_promote.h``):
the client flat ops of a 16-bit model next to fp64 operands -- torch's type promotion in
``weight_manager``'s increment and weighted sum, one launch per 32 layers.

Loaded lazily, by the first such op (a Scaffold client of a ``model.half()`` /
``model.to(torch.bfloat16)`` model from round 2 on): importing ``substrafl_amd``, fp32 models and
CPU tensors never touch it.  As with ``libfedagg.so`` there is no fallback: a missing library
raises :class:`substrafl_amd._native.NativeLibraryError`.  ``FEDAGG_FLAT_PROMOTE=0`` keeps these
operand sets on the reference's per-layer torch loops (:func:`enabled`).
"""

from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Optional

from ._native import NativeLibraryError

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("FEDAGG_PROMOTE_LIB", str(_HERE / "libfedagg_promote.so")))

c_u64 = ctypes.c_uint64
c_int = ctypes.c_int
c_void = ctypes.c_void_p
P = ctypes.POINTER

# Every symbol include/fedagg_promote.h declares, with its ctypes signature.
SIGNATURES = {
    "fedagg_promote_abi_version": (c_int, []),
    "fedagg_promote_last_error": (ctypes.c_char_p, []),
    "fedagg_promote_tune": (c_int, [ctypes.c_char_p, c_int]),
    "fedagg_promote_wsum": (c_int, [P(c_void), P(c_int), c_int, P(ctypes.c_double), P(c_u64), c_int, c_void, c_void]),
    "fedagg_promote_increment": (c_int, [P(c_void), c_int, P(c_u64), c_int, c_void, ctypes.c_double, c_void]),
}

ABI_VERSION = 1

_lib: Optional[ctypes.CDLL] = None


def enabled() -> bool:
    """Whether ``weight_manager`` sends 16-bit-next-to-fp64 operand sets to this library
    (``FEDAGG_FLAT_PROMOTE=0``: they stay on the torch loops).  Read at every call."""
    return os.environ.get("FEDAGG_FLAT_PROMOTE", "1") != "0"


def loaded() -> bool:
    """Whether this process has loaded the library (fp32 models and CPU tensors never do)."""
    return _lib is not None


def load() -> ctypes.CDLL:
    """Load (once) and return the library; raise loudly if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise NativeLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The promoted flat ops have no fallback; FEDAGG_FLAT_PROMOTE=0 "
            "keeps a 16-bit model's fp64 operands on the torch loops."
        )
    try:
        lib = ctypes.CDLL(str(LIB_PATH))
    except OSError as e:  # pragma: no cover - depends on the box
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.fedagg_promote_abi_version() != ABI_VERSION:
        raise NativeLibraryError("libfedagg_promote ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().fedagg_promote_last_error().decode(errors="replace")
        raise NativeLibraryError(f"{what} failed ({rc}): {msg}")


def tune(vec: int) -> None:
    """``fedagg_promote_tune("vec", vec)``: 0 sends every layer element by element (tests)."""
    check(load().fedagg_promote_tune(b"vec", int(vec)), "promote_tune")
