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

from ._loader import Library, lib_path
from ._native import P, c_int, c_u64, c_void

LIB_PATH = lib_path("FEDAGG_PROMOTE_LIB", "libfedagg_promote.so")

# Every symbol include/fedagg_promote.h declares, with its ctypes signature.
SIGNATURES = {
    "fedagg_promote_abi_version": (c_int, []),
    "fedagg_promote_last_error": (ctypes.c_char_p, []),
    "fedagg_promote_tune": (c_int, [ctypes.c_char_p, c_int]),
    "fedagg_promote_wsum": (c_int, [P(c_void), P(c_int), c_int, P(ctypes.c_double), P(c_u64), c_int, c_void, c_void]),
    "fedagg_promote_increment": (c_int, [P(c_void), c_int, P(c_u64), c_int, c_void, ctypes.c_double, c_void]),
}

ABI_VERSION = 1

_library = Library(globals(), "fedagg_promote_",
                   "The promoted flat ops have no fallback; FEDAGG_FLAT_PROMOTE=0 "
                   "keeps a 16-bit model's fp64 operands on the torch loops.")
load, loaded, check = _library.load, _library.loaded, _library.check  # loaded(): fp32 models and CPU tensors never


def enabled() -> bool:
    """Whether ``weight_manager`` sends 16-bit-next-to-fp64 operand sets to this library
    (``FEDAGG_FLAT_PROMOTE=0``: they stay on the torch loops).  Read at every call."""
    return os.environ.get("FEDAGG_FLAT_PROMOTE", "1") != "0"


def tune(vec: int) -> None:
    """``fedagg_promote_tune("vec", vec)``: 0 sends every layer element by element (tests)."""
    check(load().fedagg_promote_tune(b"vec", int(vec)), "promote_tune")
