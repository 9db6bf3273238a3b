"""ctypes binding of ``libfedagg_robust.so`` (the C ABI declared in ``include/fedagg_robust.h``):
robust FedAvg, the coordinate-wise trimmed mean over K client rows and the median as its limit case.

Loaded lazily, by the first robust call (``AggregationEngine.fedavg_robust``, behind
``FedAvg(..., robust=...)``): importing ``substrafl_amd`` and every other federation never touch it.
There is no fallback: a missing library raises :class:`substrafl_amd._native.NativeLibraryError`.
``FEDAGG_ROBUST_LIB`` names another copy of the library.
"""

from __future__ import annotations

import ctypes
from typing import Tuple

from ._loader import Library, lib_path
from ._native import P, c_int, c_u64, c_void, ptr_array

LIB_PATH = lib_path("FEDAGG_ROBUST_LIB", "libfedagg_robust.so")

# Every symbol include/fedagg_robust.h declares, with its ctypes signature.
SIGNATURES = {
    "fedagg_robust_abi_version": (c_int, []),
    "fedagg_robust_last_error": (ctypes.c_char_p, []),
    "fedagg_robust_blocking": (c_int, [P(c_int), P(c_int), P(c_int)]),
    "fedagg_robust_mean": (c_int, [P(c_void), c_int, c_int, c_int, c_u64, c_void, c_void]),
}

ABI_VERSION = 1
MAX_K = 128  # FEDAGG_ROBUST_MAX_K

_library = Library(globals(), "fedagg_robust_", "Robust FedAvg has no fallback.")
load, loaded, check = _library.load, _library.loaded, _library.check  # loaded(): only a robust call loads it


def blocking() -> Tuple[int, int, int]:
    """``(tile_elems, vec_f32, vec_bf16)``: the sizes at which the kernel changes path."""
    v = [c_int(0) for _ in range(3)]
    check(load().fedagg_robust_blocking(*[ctypes.byref(c) for c in v]), "robust_blocking")
    return tuple(c.value for c in v)


def mean(row_ptrs, kind: int, t: int, M: int, d_out: int, stream: int) -> None:
    """``fedagg_robust_mean`` over K device rows (a list of device addresses) of ``kind``
    (FEDAGG_F32 / FEDAGG_BF16): each element's ``t`` lowest and ``t`` highest values dropped, the
    mean of the rest as M fp32 at ``d_out``."""
    check(load().fedagg_robust_mean(ptr_array(row_ptrs), int(kind), len(row_ptrs), int(t), int(M), d_out,
                                    stream or None), "robust_mean")
